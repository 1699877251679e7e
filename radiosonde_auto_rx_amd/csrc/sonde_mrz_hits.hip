// sonde_mrz_hits.hip — the MRZ (Meteo-Radiy MP3-H1) hits of a generic engine on the device (include/sonde_hip.h: sonde_engine_set_family(SONDE_MRZ) /
// _set_family_mrz / _fetch_family, sonde_mrz_decode_device): bits, bytes and the CRC-16 under both frame lengths per hit record, behind the frame sync that queued
// it on the same stream.  What FamilyDecoder.hit -> sonde_mrz_dec_frame did per hit on one host thread inside the fetch, from 386 float soft bits copied to the
// host; 300 bytes a hit cross now, and the channel's host decoder takes the verdict of the length its state asks for.
//   k_mrz_hits: one wavefront per hit record, a grid-stride loop over the ring records [*done, *fcount), the {done, ticket} hand-over of k_family_hits.  The wave
//   functions are sonde_mrz_hits_dev.h, which the CPU wave emulator compiles as well; the static LDS is the soft-bit consumer's SoftinMrzLds and nothing else
//   (tests/test_mrz_hits_resources.py).
#include "../../include/sonde_hip.h"
#include "sonde_dev.h"
#include "sonde_devmem.h"
#include "sonde_host.h"
#include "sonde_mrz_hits_dev.h"

// frames: the engine's hit records (nbytes = valid soft bits of the hit); null: the direct entry, hit i with nbits_direct[i] bits, channel i, no header score
struct MrzRecs {
    const FrameRec *frames; const int *nbits_direct;
    __device__ __forceinline__ FamilyHitIn operator()(const unsigned slot) const {
        FamilyHitIn h;
        if (frames) { const FrameRec &r = frames[slot]; h.channel = r.channel; h.nv = r.nbytes; h.mv_pos = r.mv_pos; h.mv = r.mv; }
        else { h.channel = (int32_t)slot; h.nv = nbits_direct[slot]; h.mv_pos = 0u; h.mv = 0.f; }
        return h;
    }
};

__global__ __launch_bounds__(64)
void k_mrz_hits(const MrzHitsArgs a, const MrzRecs recs, const unsigned *fcount, unsigned *done) {
    __shared__ __attribute__((aligned(16))) SoftinMrzLds s_l;
    const int lane = threadIdx.x;
    const unsigned end = *fcount, start = done[0];
    mrz_wave_records(a, recs, start, end, (int)blockIdx.x, (int)gridDim.x, &s_l, lane);
    __threadfence();
    family_wave_ticket(done, end, (int)gridDim.x, lane);
}

// bits_ofs is 0 .. 64 (the callers have checked); grid >= 1
extern "C" void sonde_launch_mrz_hits(int bits_ofs, const FrameRec *frames, const int *nbits_direct, const float *soft, long long stride, int max_frames,
                                      const unsigned *fcount, unsigned *done, sonde_family_hit_t *out, int grid, hipStream_t s) {
    const MrzHitsArgs a{soft, stride, bits_ofs, max_frames, out};
    const MrzRecs r{frames, nbits_direct};
    hipLaunchKernelGGL(k_mrz_hits, dim3(grid), dim3(64), 0, s, a, r, fcount, done);
}

extern "C" int sonde_mrz_decode_device(int32_t bits_ofs, const float *soft, int64_t stride, const int32_t *nbits, int32_t n, sonde_family_hit_t *out) {
    if (bits_ofs < 0 || bits_ofs > 64 || !soft || !nbits || !out || n < 0 || stride < MRZ_HIT_BITS) return SONDE_E_ARG;
    for (int i = 0; i < n; i++) if (nbits[i] < 0 || nbits[i] > stride) return SONDE_E_ARG;
    if (n == 0) return 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); return SONDE_E_NOGPU; }
    DevMem mem;                                                        // one-shot temporaries of this call: freed on every path
    float *d_soft = nullptr; int *d_nb = nullptr; unsigned *d_cnt = nullptr; sonde_family_hit_t *d_out = nullptr;
    TRY(mem.dalloc(&d_soft, (size_t)n * (size_t)stride, false));
    TRY(mem.dalloc(&d_nb, (size_t)n, false));
    TRY(mem.dalloc(&d_cnt, 3));                                        // {fcount, done, ticket}
    TRY(mem.dalloc(&d_out, (size_t)n, false));
    const unsigned cnt[3] = { (unsigned)n, 0u, 0u };
    HIPCHK(hipMemcpy(d_soft, soft, (size_t)n * (size_t)stride * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_nb, nbits, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_cnt, cnt, sizeof cnt, hipMemcpyHostToDevice));
    sonde_launch_mrz_hits(bits_ofs, nullptr, d_nb, d_soft, (long long)stride, n, d_cnt, d_cnt + 1, d_out, n < 1024 ? n : 1024, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, d_out, (size_t)n * sizeof(sonde_family_hit_t), hipMemcpyDeviceToHost));
    return 0;
}
