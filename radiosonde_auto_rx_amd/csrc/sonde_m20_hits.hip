// sonde_m20_hits.hip — the M20 hits of a base-rate or mixed engine on the device (include/sonde_hip.h: sonde_engine_fetch_m20 / _m20_lagged,
// sonde_m20_decode_device): differential decoding into the channel's persistent bit characters, bits2bytes, frame and block checksum per hit record, behind the
// frame sync that queued it on the same stream.  What sonde_engine_fetch_m20 did per hit on one host thread from a 596-byte record and 1320 float soft bits copied
// to the host; 208 bytes a hit cross now.
//   k_m20_hits: 64 threads, grid = min(n_channels, 1024); the ring records [*done, *fcount) in order, a channel's by the workgroup channel % grid; the
//   {done, ticket} hand-over of k_m10_hits (sonde_softin_dev.hip).  The wave functions are sonde_m20_hits_dev.h, which the CPU wave emulator compiles as well.
#include "../../include/sonde_hip.h"
#include "sonde_dev.h"
#include "sonde_devmem.h"
#include "sonde_host.h"
#include "sonde_m20_hits_dev.h"

// frames: the engine's hit records (nbytes = valid bits of the hit); null: the direct entry, hit i = 165 bytes at bits + 165 i with nbits[i], channel[i], mv[i]
struct M20Recs {
    const FrameRec *frames; const uint8_t *bits; const int *nbits, *channel; const float *mv;
    __device__ __forceinline__ M20HitIn operator()(const unsigned slot) const {
        M20HitIn h;
        if (frames) { const FrameRec &r = frames[slot]; h.channel = r.channel; h.nv = r.nbytes; h.mv_pos = r.mv_pos; h.mv = r.mv; h.bits = r.frame; }
        else { h.channel = channel[slot]; h.nv = nbits[slot]; h.mv_pos = 0u; h.mv = mv ? mv[slot] : 0.f; h.bits = bits + (size_t)slot * M20_NBYTES; }
        return h;
    }
};

__global__ __launch_bounds__(64)
void k_m20_hits(const M20HitsArgs a, const M20Recs recs, const unsigned *fcount, unsigned *done) {
    __shared__ unsigned char s_fr[M20_REC_BYTES];
    const int lane = threadIdx.x;
    const unsigned end = *fcount, start = done[0];
    m20_wave_records(a, recs, start, end, (int)blockIdx.x, (int)gridDim.x, s_fr, lane);
    __threadfence();
    m20_wave_ticket(done, end, (int)gridDim.x, lane);
}

// grid >= 1
extern "C" void sonde_launch_m20_hits(const FrameRec *frames, int n_channels, int max_frames, const unsigned *fcount, unsigned *done, char *chan_bits,
                                      sonde_m20_frame_t *out, int grid, hipStream_t s) {
    const M20HitsArgs a{n_channels, max_frames, chan_bits, out};
    const M20Recs r{frames, nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(k_m20_hits, dim3(grid), dim3(64), 0, s, a, r, fcount, done);
}

extern "C" int sonde_m20_decode_device(const uint8_t *bits, const int32_t *nbits, const int32_t *channel, const float *mv, int32_t n, int32_t n_channels,
                                       sonde_m20_frame_t *out, char *chars_out) {
    if (!bits || !nbits || !channel || !out || n < 0 || n_channels < 1) return SONDE_E_ARG;
    for (int i = 0; i < n; i++) if (nbits[i] < 0 || nbits[i] > M20_NBITS || channel[i] < 0 || channel[i] >= n_channels) return SONDE_E_ARG;
    if (n == 0 && !chars_out) return 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); return SONDE_E_NOGPU; }
    DevMem mem;                                                        // one-shot temporaries of this call: freed on every path
    uint8_t *d_bits = nullptr; int *d_nb = nullptr, *d_ch = nullptr; float *d_mv = nullptr; unsigned *d_cnt = nullptr; char *d_chars = nullptr; sonde_m20_frame_t *d_out = nullptr;
    const size_t chars = (size_t)n_channels * M20_CHAN_CHARS;
    TRY(mem.dalloc(&d_chars, chars));                                  // zero, as at an engine's create
    TRY(mem.dalloc(&d_cnt, 3));                                        // {fcount, done, ticket}
    if (n > 0) {
        TRY(mem.dalloc(&d_bits, (size_t)n * M20_NBYTES, false));
        TRY(mem.dalloc(&d_nb, (size_t)n, false));
        TRY(mem.dalloc(&d_ch, (size_t)n, false));
        if (mv) TRY(mem.dalloc(&d_mv, (size_t)n, false));
        TRY(mem.dalloc(&d_out, (size_t)n, false));
        const unsigned cnt[3] = { (unsigned)n, 0u, 0u };
        HIPCHK(hipMemcpy(d_bits, bits, (size_t)n * M20_NBYTES, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_nb, nbits, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_ch, channel, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
        if (mv) HIPCHK(hipMemcpy(d_mv, mv, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_cnt, cnt, sizeof cnt, hipMemcpyHostToDevice));
        const M20HitsArgs a{n_channels, n, d_chars, d_out};
        const M20Recs r{nullptr, d_bits, d_nb, d_ch, d_mv};
        hipLaunchKernelGGL(k_m20_hits, dim3(n_channels < 1024 ? n_channels : 1024), dim3(64), 0, nullptr, a, r, d_cnt, d_cnt + 1);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpy(out, d_out, (size_t)n * sizeof(sonde_m20_frame_t), hipMemcpyDeviceToHost));
    }
    if (chars_out) HIPCHK(hipMemcpy(chars_out, d_chars, chars, hipMemcpyDeviceToHost));
    return 0;
}
