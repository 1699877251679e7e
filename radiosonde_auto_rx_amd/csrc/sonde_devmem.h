// sonde_devmem.h — the one owner of device memory behind the host objects of libsonde_hip, and the two macros their functions return through.
// An object declares `DevMem mem;` as its FIRST member (destroyed last: its destructor may still read device memory) and allocates with
// TRY(mem.dalloc(...)) / TRY(mem.upload(...)); whatever is still held is freed when the object goes.  Pinned host memory: Pinned<T> (sonde_pinned.h).
// Only the HIP host API is needed here, so a plain C++ compiler takes this header (tests/emu/devmem_fake.cpp).
#ifndef SONDE_DEVMEM_H
#define SONDE_DEVMEM_H
#include "../../include/sonde_hip.h"
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstdio>
#include <vector>

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "libsonde_hip: %s failed: %s\n", #x, hipGetErrorString(e_)); return SONDE_E_NOGPU; } } while (0)
#define TRY(x) do { const int rc_ = (x); if (rc_) return rc_; } while (0)

struct DevMem {
    std::vector<void *> held;
    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    ~DevMem() { for (void *p : held) (void)hipFree(p); }        // (never touches a stream: the owner has synchronised its own by now)

    // max(n, 1) elements, registered here; zero: cleared with a synchronous memset.  -> 0 or SONDE_E_NOMEM, *p == nullptr then
    template <class T> int dalloc(T **p, size_t n, bool zero = true) {
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        void *q = nullptr;
        *p = nullptr;
        if (hipMalloc(&q, bytes) != hipSuccess) { (void)hipGetLastError(); return SONDE_E_NOMEM; }
        held.push_back(q);
        if (zero && hipMemset(q, 0, bytes) != hipSuccess) { release(q); return SONDE_E_NOMEM; }
        *p = (T *)q;
        return 0;
    }
    // dalloc + synchronous copy of v (which may be empty); P: T or const T
    template <class P, class T> int upload(P **p, const std::vector<T> &v) {
        T *q = nullptr;
        *p = nullptr;
        TRY(dalloc(&q, v.size(), false));
        if (!v.empty()) HIPCHK(hipMemcpy(q, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        *p = q;
        return 0;
    }
    // frees one buffer now and forgets it (a staging buffer that regrows); the caller has synchronised whatever used it.  A pointer not held is left alone
    void release(void *p) {
        auto it = std::find(held.begin(), held.end(), p);
        if (p && it != held.end()) { (void)hipFree(p); held.erase(it); }
    }
};
#endif
