// devmem_fake.cpp — DevMem (csrc/sonde_devmem.h) and Pinned<T> (csrc/sonde_pinned.h) against a fake HIP allocator on the CPU: the eight HIP
// calls the two headers make are defined HERE, on malloc and a set of live pointers, and no HIP library is linked.  A switch makes the k-th
// allocation fail; a free of a pointer that is not live ends the program with status 3 at once.  tests/test_devmem.py builds this, runs it and
// reads the tallies it prints; every failed check prints a line and the program ends with status 1.
#include "../../radiosonde_auto_rx_amd/csrc/sonde_devmem.h"
#include "../../radiosonde_auto_rx_amd/csrc/sonde_pinned.h"
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>

// ---- the fake -------------------------------------------------------------------------------------------------------------------
static std::map<void *, size_t> g_dev, g_host;             // live pointers -> bytes
static long g_allocs = 0, g_fail_at = -1;                   // allocations asked for so far (device and host together); the one that fails
static long g_dev_allocs = 0, g_dev_frees = 0, g_host_allocs = 0, g_host_frees = 0;
static void *g_memset_ptr = nullptr; static size_t g_memset_bytes = 0; static int g_memsets = 0;

static hipError_t fake_alloc(std::map<void *, size_t> &live, long &tally, void **p, size_t bytes) {
    if (g_allocs++ == g_fail_at) { *p = (void *)(uintptr_t)0xdead; return hipErrorOutOfMemory; }      // (garbage on purpose: the owners must not keep it)
    if (!bytes) { fprintf(stderr, "fake: allocation of 0 bytes\n"); exit(3); }
    *p = malloc(bytes);
    memset(*p, 0xa5, bytes);
    live[*p] = bytes; tally++;
    return hipSuccess;
}
static hipError_t fake_free(std::map<void *, size_t> &live, long &tally, void *p, const char *what) {
    if (!p) return hipSuccess;
    if (!live.count(p)) { fprintf(stderr, "fake: %s of a pointer that is not live\n", what); exit(3); }
    live.erase(p); free(p); tally++;
    return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) { return fake_alloc(g_dev, g_dev_allocs, p, bytes); }
hipError_t hipFree(void *p) { return fake_free(g_dev, g_dev_frees, p, "hipFree"); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { return fake_alloc(g_host, g_host_allocs, p, bytes); }
hipError_t hipHostFree(void *p) { return fake_free(g_host, g_host_frees, p, "hipHostFree"); }
hipError_t hipMemset(void *p, int v, size_t bytes) {
    if (!g_dev.count(p) || g_dev[p] < bytes) { fprintf(stderr, "fake: hipMemset outside a live buffer\n"); exit(3); }
    memset(p, v, bytes); g_memset_ptr = p; g_memset_bytes = bytes; g_memsets++;
    return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind) {
    if (!g_dev.count(dst) || g_dev[dst] < bytes) { fprintf(stderr, "fake: hipMemcpy outside a live buffer\n"); exit(3); }
    memcpy(dst, src, bytes);
    return hipSuccess;
}
const char *hipGetErrorString(hipError_t) { return "fake error"; }
hipError_t hipGetLastError(void) { return hipSuccess; }
}

static int g_bad = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); g_bad++; } } while (0)
static size_t live() { return g_dev.size() + g_host.size(); }

// ---- an object and a create written like the library's: DevMem first, unique_ptr, TRY, early return --------------------------------
enum { N_SLOTS = 7 };
static void *g_seen[N_SLOTS];                               // the object's pointers as its destructor found them
struct Obj {
    DevMem mem;
    float *a = nullptr; int *b = nullptr; Pinned<int> h; double *c = nullptr; const uint8_t *d = nullptr; Pinned<char> h2; short *e = nullptr;
    ~Obj() { void *s[N_SLOTS] = { a, b, h.data(), c, (void *)d, h2.data(), e }; memcpy(g_seen, s, sizeof s); }
};
static int obj_create(Obj **out) {
    std::unique_ptr<Obj> o(new Obj());
    TRY(o->mem.dalloc(&o->a, 100));                                           // slot 0
    TRY(o->mem.upload(&o->b, std::vector<int>{ 1, 2, 3, 4, 5 }));             // slot 1
    if (!o->h.alloc(16)) return SONDE_E_NOMEM;                                // slot 2
    TRY(o->mem.dalloc(&o->c, 7, false));                                      // slot 3
    TRY(o->mem.upload(&o->d, std::vector<uint8_t>()));                        // slot 4
    if (!o->h2.alloc(0, hipHostMallocMapped)) return SONDE_E_NOMEM;           // slot 5
    TRY(o->mem.dalloc(&o->e, 0));                                             // slot 6
    *out = o.release();
    return 0;
}

int main() {
    // 1: mixed allocations, then scope exit
    {
        Obj *o = nullptr;
        CHECK(obj_create(&o) == 0 && o);
        CHECK(g_allocs == N_SLOTS && g_dev.size() == 5 && g_host.size() == 2);
        CHECK(o && o->b[4] == 5 && o->h[15] == 0);
        delete o;
        CHECK(live() == 0);
        printf("case 1: allocations %ld live after %zu\n", g_allocs, live());
    }
    // 2: the k-th allocation fails
    int nomem = 0;
    for (int k = 0; k < N_SLOTS; k++) {
        g_allocs = 0; g_fail_at = k;
        Obj *o = nullptr;
        const int rc = obj_create(&o);
        g_fail_at = -1;
        CHECK(rc == SONDE_E_NOMEM && !o);
        nomem += rc == SONDE_E_NOMEM;
        CHECK(live() == 0);
        for (int i = 0; i < N_SLOTS; i++) CHECK((g_seen[i] != nullptr) == (i < k));      // the failed slot and everything behind it: nullptr
    }
    CHECK(g_dev_allocs == g_dev_frees && g_host_allocs == g_host_frees);
    printf("case 2: failures %d of %d live after %zu\n", nomem, (int)N_SLOTS, live());
    // 3: a staging buffer that regrows: release in the middle, a larger dalloc, scope exit
    {
        const long frees0 = g_dev_frees;
        DevMem mem;
        int *x = nullptr, *z = nullptr; uint8_t *stage = nullptr;
        CHECK(mem.dalloc(&x, 4) == 0 && mem.dalloc(&stage, 1000, false) == 0 && mem.dalloc(&z, 4) == 0);
        void *old = stage;
        mem.release(stage);
        CHECK(g_dev_frees == frees0 + 1 && !g_dev.count(old) && g_dev.size() == 2);
        CHECK(mem.dalloc(&stage, 4000, false) == 0 && g_dev[stage] == 4000);
        mem.release(nullptr); mem.release(&x);                                   // not held: left alone
        CHECK(g_dev_frees == frees0 + 1 && g_dev.size() == 3);
        // a dalloc that fails after a release leaves nullptr, not the stale pointer
        mem.release(stage);
        g_allocs = 0; g_fail_at = 0;
        CHECK(mem.dalloc(&stage, 8000, false) == SONDE_E_NOMEM && stage == nullptr);
        g_fail_at = -1;
    }
    CHECK(live() == 0 && g_dev_allocs == g_dev_frees);
    printf("case 3: live after %zu\n", live());
    // 4: empty upload, zero elements, the whole size to the memset
    {
        DevMem mem;
        float *u = nullptr; double *one = nullptr; int *zr = nullptr;
        CHECK(mem.upload(&u, std::vector<float>()) == 0 && u && g_dev.count(u) && g_dev[u] == sizeof(float));
        const int m0 = g_memsets;
        CHECK(mem.dalloc(&one, 0) == 0 && one && g_dev[one] == sizeof(double) && g_memset_ptr == one && g_memset_bytes == sizeof(double));
        CHECK(mem.dalloc(&zr, 1000) == 0 && g_memset_ptr == zr && g_memset_bytes == 1000 * sizeof(int) && zr[999] == 0 && g_memsets == m0 + 2);
        CHECK(mem.dalloc(&zr, 10, false) == 0 && g_memsets == m0 + 2 && (unsigned char)((char *)zr)[0] == 0xa5);
        Pinned<int> p;
        CHECK(p.alloc(0) && p.data() && p.size() == 0 && p.alloc(8) && p.size() == 8 && g_host.size() == 1);      // (alloc releases what it held)
    }
    CHECK(live() == 0);
    printf("case 4: live after %zu\n", live());
    // 5: a pointer that was assigned, not registered (a group's rows of its owner's ring) is never freed
    {
        void *owner_rows = nullptr;
        CHECK(hipMalloc(&owner_rows, 64) == hipSuccess);
        {
            Obj *o = nullptr;
            CHECK(obj_create(&o) == 0 && o);
            if (o) o->a = (float *)owner_rows + 4;
            delete o;
        }
        CHECK(live() == 1 && g_dev.count(owner_rows));
        (void)hipFree(owner_rows);
    }
    CHECK(live() == 0);
    printf("case 5: live after %zu\n", live());
    printf("device allocations %ld frees %ld host allocations %ld frees %ld failed checks %d\n", g_dev_allocs, g_dev_frees, g_host_allocs, g_host_frees, g_bad);
    return g_bad ? 1 : 0;
}
