// sonde_lms6_rs.hip — RS(255,223) of LMS6-403 / LMS-X blocks on the device (include/sonde_hip.h: sonde_lms6_rs_device, sonde_engine_set_family_lms6_rs /
// _fetch_family_lms6_rs; include/sonde_fsk.h: sonde_softin_dev_set_lms6_rs): rs_decode under each hypothesis proc_frame can ask for, per block record, over the
// block bytes where k_lms6_hits (sonde_lms6_hits.hip) or k_softin_lms6 (sonde_softin_dev.hip) left them in device memory.  What sonde_lms6_dec_block_bytes did per
// block on one host thread — 32 syndromes over 255 bytes, Euclid, Chien and Forney at t = 16 — the host decoder now takes from a 120-byte record
// (sonde_lms6_dec_block_rs).
//   k_lms6_rs: one wavefront per block record, a grid-stride loop over the records [start, end).  An engine's launch reads the range as k_lms6_hits does, from the
//   frame counter and a {done, ticket} pair of its own, so that it covers exactly the records the k_lms6_hits launch in front of it has written; a consumer's
//   launch covers [0, min(*count, cap)); the direct entry [0, n).  The wave functions are sonde_rs223_dev.h, which the CPU wave emulator compiles as well; the
//   static LDS is Lms6RsLds (1408 B) and nothing else (tests/test_lms6_rs_resources.py).
#include <cstddef>
#include <cstring>
#include <vector>
#include "../../include/sonde_hip.h"
#include "../../include/sonde_ecc.h"
#include "sonde_dev.h"
#include "sonde_devmem.h"
#include "sonde_host.h"
#include "sonde_rs223_dev.h"
#include "sonde_family_hits_dev.h"                                     // family_wave_ticket

// the range of a launch: count != null: end = *count, else end = n; done != null: start = done[0] and the ticket hand-over behind the loop (an engine's ring),
// else start = 0 and end <= max_frames (records beyond the buffer were dropped by the kernel that counted them)
struct Lms6RsRange { const unsigned *count; unsigned *done; unsigned n; };

__global__ __launch_bounds__(64)
void k_lms6_rs(const Lms6RsArgs a, const Lms6RsRange r, const uint8_t *tab) {
    __shared__ __attribute__((aligned(16))) Lms6RsLds s_l;
    const int lane = threadIdx.x;
    unsigned end = r.count ? *r.count : r.n, start = 0;
    if (r.done) start = r.done[0];
    else if (end > (unsigned)a.max_frames) end = (unsigned)a.max_frames;
    lms6_rs_wave_tables(&s_l, tab, lane);
    lms6_rs_wave_records(a, start, end, (int)blockIdx.x, (int)gridDim.x, &s_l, lane);
    if (r.done) {
        __threadfence();
        family_wave_ticket(r.done, end, (int)gridDim.x, lane);
    }
}

// exp[512] | log[256] of GF(256) / 0x187 into device memory owned by mem: the tables of the host codec (sonde_ecc.cpp), not a second generator
int sonde_lms6_rs_tables(DevMem &mem, const uint8_t **tab) {
    uint8_t *d = nullptr;
    TRY(mem.dalloc(&d, 768, false));
    sonde_ecc_t *c = sonde_ecc_create(SONDE_ECC_RS255CCSDS);
    const uint8_t *e = nullptr, *l = nullptr;
    if (!c || sonde_ecc_tables(c, &e, &l)) { sonde_ecc_destroy(c); return SONDE_E_ARG; }
    const bool ok = hipMemcpy(d, e, 512, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d + 512, l, 256, hipMemcpyHostToDevice) == hipSuccess;
    sonde_ecc_destroy(c);
    if (!ok) { (void)hipGetLastError(); return SONDE_E_NOGPU; }
    *tab = d;
    return 0;
}

// records of `stride` bytes with their block bytes / blen / decoded (off_decoded < 0: none) at these offsets; max_frames = slots of recs and out; grid >= 1
extern "C" void sonde_launch_lms6_rs(const void *recs, long long stride, int off_bytes, int off_blen, int off_decoded, int max_frames, const unsigned *count,
                                     unsigned *done, unsigned n, const uint8_t *tab, sonde_lms6_rs_t *out, int grid, hipStream_t s) {
    const Lms6RsArgs a{(const uint8_t *)recs, stride, off_bytes, off_blen, off_decoded, max_frames, out};
    const Lms6RsRange r{count, done, n};
    hipLaunchKernelGGL(k_lms6_rs, dim3(grid), dim3(64), 0, s, a, r, tab);
}

namespace { struct DirectRec { int32_t blen; uint8_t bytes[LMS6_RS_BB]; }; }

extern "C" int sonde_lms6_rs_device(const uint8_t *bytes, int64_t stride, const int32_t *blen, int32_t n, sonde_lms6_rs_t *out) {
    if (!bytes || !blen || !out || n < 0 || stride < LMS6_RS_BB) return SONDE_E_ARG;
    for (int i = 0; i < n; i++) if (blen[i] < 0 || blen[i] > 300) return SONDE_E_ARG;
    if (n == 0) return 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); return SONDE_E_NOGPU; }
    std::vector<DirectRec> h((size_t)n);
    for (int i = 0; i < n; i++) { h[(size_t)i].blen = blen[i]; memcpy(h[(size_t)i].bytes, bytes + (size_t)i * (size_t)stride, LMS6_RS_BB); }
    DevMem mem;                                                        // one-shot temporaries of this call: freed on every path
    DirectRec *d_rec = nullptr; sonde_lms6_rs_t *d_out = nullptr; const uint8_t *d_tab = nullptr;
    TRY(mem.dalloc(&d_rec, (size_t)n, false));
    TRY(mem.dalloc(&d_out, (size_t)n, false));
    TRY(sonde_lms6_rs_tables(mem, &d_tab));
    HIPCHK(hipMemcpy(d_rec, h.data(), (size_t)n * sizeof(DirectRec), hipMemcpyHostToDevice));
    sonde_launch_lms6_rs(d_rec, (long long)sizeof(DirectRec), (int)offsetof(DirectRec, bytes), (int)offsetof(DirectRec, blen), -1, n, nullptr, nullptr, (unsigned)n,
                         d_tab, d_out, n < 1024 ? n : 1024, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, d_out, (size_t)n * sizeof(sonde_lms6_rs_t), hipMemcpyDeviceToHost));
    return 0;
}
