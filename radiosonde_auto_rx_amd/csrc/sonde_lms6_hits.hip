// sonde_lms6_hits.hip — the LMS6-403 / LMS-X hits of a generic engine on the device (include/sonde_hip.h: sonde_engine_set_family_lms6 / _fetch_family_lms6,
// sonde_lms6_decode_device): the raw-bit sign alternation, the K = 7 Viterbi decoder, deconv and bits2bytes per hit record, behind the frame sync that queued it on
// the same stream.  What FamilyDecoder.hit -> sonde_lms6_dec_block did per hit on one host thread inside the fetch, from 4096 or 4720 float soft bits copied to
// the host; 348 bytes a hit cross now, and the channel's host decoder goes on from block_bytes (sonde_lms6_dec_block_bytes).
//   k_lms6_hits: one wavefront per hit record, a grid-stride loop over the ring records [*done, *fcount), the {done, ticket} hand-over of k_family_hits.  The wave
//   functions are sonde_lms6_hits_dev.h, which the CPU wave emulator compiles as well; the static LDS is the soft-bit consumer's Lms6Lds and nothing else, four
//   one-wave workgroups to a CU (tests/test_lms6_hits_resources.py).
#include "../../include/sonde_hip.h"
#include "sonde_dev.h"
#include "sonde_devmem.h"
#include "sonde_host.h"
#include "sonde_lms6_hits_dev.h"

// frames: the engine's hit records (nbytes = valid soft bits of the hit); null: the direct entry, hit i with nbits_direct[i] bits and the score mv_direct[i], channel i
struct Lms6Recs {
    const FrameRec *frames; const int *nbits_direct; const float *mv_direct;
    __device__ __forceinline__ FamilyHitIn operator()(const unsigned slot) const {
        FamilyHitIn h;
        if (frames) { const FrameRec &r = frames[slot]; h.channel = r.channel; h.nv = r.nbytes; h.mv_pos = r.mv_pos; h.mv = r.mv; }
        else { h.channel = (int32_t)slot; h.nv = nbits_direct[slot]; h.mv_pos = 0u; h.mv = mv_direct[slot]; }
        return h;
    }
};

__global__ __launch_bounds__(64)
void k_lms6_hits(const Lms6HitsArgs a, const Lms6Recs recs, const unsigned *fcount, unsigned *done) {
    __shared__ __attribute__((aligned(16))) Lms6Lds s_l;
    const int lane = threadIdx.x;
    const unsigned end = *fcount, start = done[0];
    lms6_wave_records(a, recs, start, end, (int)blockIdx.x, (int)gridDim.x, &s_l, lane);
    __threadfence();
    family_wave_ticket(done, end, (int)gridDim.x, lane);
}

// vit is 1 or 2 and nb 4096 or 4720 <= stride (the callers have checked); grid >= 1
extern "C" void sonde_launch_lms6_hits(int vit, int nb, const FrameRec *frames, const int *nbits_direct, const float *mv_direct, const float *soft, long long stride,
                                       int max_frames, const unsigned *fcount, unsigned *done, sonde_lms6_hit_t *out, int grid, hipStream_t s) {
    const Lms6HitsArgs a{soft, stride, vit, nb, max_frames, out};
    const Lms6Recs r{frames, nbits_direct, mv_direct};
    hipLaunchKernelGGL(k_lms6_hits, dim3(grid), dim3(64), 0, s, a, r, fcount, done);
}

extern "C" int sonde_lms6_decode_device(int32_t vit, const float *soft, int64_t stride, const int32_t *nbits, const float *mv, int32_t n, sonde_lms6_hit_t *out) {
    if ((vit != 1 && vit != 2) || !soft || !nbits || !mv || !out || n < 0 || (stride != LMS6_HIT_BITS6 && stride != LMS6_HIT_BITSX)) return SONDE_E_ARG;
    for (int i = 0; i < n; i++) if (nbits[i] < 0 || nbits[i] > stride) return SONDE_E_ARG;
    if (n == 0) return 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); return SONDE_E_NOGPU; }
    DevMem mem;                                                        // one-shot temporaries of this call: freed on every path
    float *d_soft = nullptr, *d_mv = nullptr; int *d_nb = nullptr; unsigned *d_cnt = nullptr; sonde_lms6_hit_t *d_out = nullptr;
    TRY(mem.dalloc(&d_soft, (size_t)n * (size_t)stride, false));
    TRY(mem.dalloc(&d_nb, (size_t)n, false));
    TRY(mem.dalloc(&d_mv, (size_t)n, false));
    TRY(mem.dalloc(&d_cnt, 3));                                        // {fcount, done, ticket}
    TRY(mem.dalloc(&d_out, (size_t)n, false));
    const unsigned cnt[3] = { (unsigned)n, 0u, 0u };
    HIPCHK(hipMemcpy(d_soft, soft, (size_t)n * (size_t)stride * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_nb, nbits, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_mv, mv, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_cnt, cnt, sizeof cnt, hipMemcpyHostToDevice));
    sonde_launch_lms6_hits(vit, (int)stride, nullptr, d_nb, d_mv, d_soft, (long long)stride, n, d_cnt, d_cnt + 1, d_out, n < 1024 ? n : 1024, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, d_out, (size_t)n * sizeof(sonde_lms6_hit_t), hipMemcpyDeviceToHost));
    return 0;
}
