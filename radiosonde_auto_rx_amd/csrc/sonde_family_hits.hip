// sonde_family_hits.hip — the block codes of a generic engine's header hits on the device (include/sonde_hip.h: sonde_engine_set_family / _fetch_family,
// sonde_family_decode_device): Meisei BCH(63,51), iMet-54 Hamming(8,4) and check sums, MTS01 CRC-16, RS92 RS(255,231), per hit record behind the frame sync.
// What FamilyDecoder.hit -> sonde_<kind>_dec_frame did per frame on one host thread inside the fetch, from 1048 .. 2340 float soft bits a hit copied to the host,
// now runs over the records a process call has queued, on the same stream; 300 bytes a hit cross to the host.
//   k_family_hits<K>: one wavefront per hit record, a grid-stride loop over the ring records [*done, *fcount), the {done, ticket} hand-over of k_dfm_hits
//   (sonde_softin_dev.hip).  The wave functions are sonde_family_hits_dev.h, which the CPU wave emulator compiles as well; the static LDS of a kernel is the LDS
//   struct of the kind's soft-bit consumer and nothing else (tests/test_family_hits_resources.py).
// (no contraction: the reference is plain C on x86-64 — every product and sum rounded on its own)
#pragma clang fp contract(off)
#include "../../include/sonde_hip.h"
#include "sonde_dev.h"
#include "sonde_devmem.h"
#include "sonde_host.h"
#include "sonde_family_hits_dev.h"
#include <vector>

// frames: the engine's hit records (nbytes = valid soft bits of the hit); null: the direct entry, hit i with nbits_direct[i] bits, channel i, no header score
struct FamilyRecs {
    const FrameRec *frames; const int *nbits_direct;
    __device__ __forceinline__ FamilyHitIn operator()(const unsigned slot) const {
        FamilyHitIn h;
        if (frames) { const FrameRec &r = frames[slot]; h.channel = r.channel; h.nv = r.nbytes; h.mv_pos = r.mv_pos; h.mv = r.mv; }
        else { h.channel = (int32_t)slot; h.nv = nbits_direct[slot]; h.mv_pos = 0u; h.mv = 0.f; }
        return h;
    }
};

template <class K>
__global__ __launch_bounds__(64)
void k_family_hits(const FamilyArgs a, const FamilyRecs recs, const unsigned *fcount, unsigned *done) {
    __shared__ __attribute__((aligned(16))) typename K::Lds s_l;
    const int lane = threadIdx.x;
    const unsigned end = *fcount, start = done[0];
    family_wave_records<K>(a, recs, start, end, (int)blockIdx.x, (int)gridDim.x, &s_l, lane);
    __threadfence();
    family_wave_ticket(done, end, (int)gridDim.x, lane);
}

// kind is one of the four (the callers have checked); grid >= 1
extern "C" void sonde_launch_family_hits(int kind, int ecc, const FrameRec *frames, const int *nbits_direct, const float *soft, long long stride, int max_frames,
                                         const unsigned *fcount, unsigned *done, const uint32_t *tab, const uint8_t *gf, sonde_family_hit_t *out, int grid, hipStream_t s) {
    const FamilyArgs a{soft, stride, ecc, max_frames, tab, gf, out};
    const FamilyRecs r{frames, nbits_direct};
    switch (kind) {
        case SONDE_MEISEI: hipLaunchKernelGGL(k_family_hits<FamilyMeisei>, dim3(grid), dim3(64), 0, s, a, r, fcount, done); break;
        case SONDE_IMET54: hipLaunchKernelGGL(k_family_hits<FamilyImet54>, dim3(grid), dim3(64), 0, s, a, r, fcount, done); break;
        case SONDE_MTS01:  hipLaunchKernelGGL(k_family_hits<FamilyMts01>, dim3(grid), dim3(64), 0, s, a, r, fcount, done); break;
        case SONDE_RS92:   hipLaunchKernelGGL(k_family_hits<FamilyRs92>, dim3(grid), dim3(64), 0, s, a, r, fcount, done); break;
        default: break;
    }
}

// what a kind's kernel reads besides the hits: iMet-54's contribution words, RS92's GF tables (null for the others)
int sonde_family_tables(DevMem &mem, int kind, const uint32_t **tab, const uint8_t **gf) {
    *tab = nullptr; *gf = nullptr;
    if (kind == SONDE_IMET54) {
        std::vector<uint32_t> t((size_t)IMET54_TAB_N);
        imet54_crc_table(t.data());
        TRY(mem.upload(tab, t));
    }
    if (kind == SONDE_RS92) {
        std::vector<uint8_t> g(768);
        memcpy(g.data(), sonde::gf_exp_table(), 512); memcpy(g.data() + 512, sonde::gf_log_table(), 256);
        TRY(mem.upload(gf, g));
    }
    return 0;
}

extern "C" int sonde_family_decode_device(int32_t kind, int32_t ecc, const float *soft, int64_t stride, const int32_t *nbits, int32_t n, sonde_family_hit_t *out) {
    const int NB = family_kind_bits(kind);
    if (!NB || !soft || !nbits || !out || n < 0 || stride < NB || (kind == SONDE_RS92 && !ecc)) return SONDE_E_ARG;
    for (int i = 0; i < n; i++) if (nbits[i] < 0 || nbits[i] > stride) return SONDE_E_ARG;
    if (n == 0) return 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); return SONDE_E_NOGPU; }
    DevMem mem;                                                        // one-shot temporaries of this call: freed on every path
    float *d_soft = nullptr; int *d_nb = nullptr; unsigned *d_cnt = nullptr; sonde_family_hit_t *d_out = nullptr;
    const uint32_t *d_tab = nullptr; const uint8_t *d_gf = nullptr;
    TRY(mem.dalloc(&d_soft, (size_t)n * (size_t)stride, false));
    TRY(mem.dalloc(&d_nb, (size_t)n, false));
    TRY(mem.dalloc(&d_cnt, 3));                                        // {fcount, done, ticket}
    TRY(mem.dalloc(&d_out, (size_t)n, false));
    TRY(sonde_family_tables(mem, kind, &d_tab, &d_gf));
    const unsigned cnt[3] = { (unsigned)n, 0u, 0u };
    HIPCHK(hipMemcpy(d_soft, soft, (size_t)n * (size_t)stride * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_nb, nbits, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_cnt, cnt, sizeof cnt, hipMemcpyHostToDevice));
    sonde_launch_family_hits(kind, ecc, nullptr, d_nb, d_soft, (long long)stride, n, d_cnt, d_cnt + 1, d_tab, d_gf, d_out, n < 1024 ? n : 1024, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, d_out, (size_t)n * sizeof(sonde_family_hit_t), hipMemcpyDeviceToHost));
    return 0;
}
