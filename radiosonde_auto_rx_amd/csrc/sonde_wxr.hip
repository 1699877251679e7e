// sonde_wxr.hip — k_wxr_slice: the bit slicer of the reference's weathex/weathex301d.c (read_bits_fsk :171, read_rawbit :200, the frame loop
// of main :649-707) on the FM samples of many channels, one wavefront per channel.
//
// The reference is a state machine from frame to frame, but each of its two phases is data-parallel over a stretch of samples:
//  - search (no -b frame open): 64 samples at a time.  Sign bits by ballot, sign changes = ends of runs, every change lane computes its
//    run's length in bits with the reference's float division; the wave then takes the few runs of the tile in order, and for each the lanes
//    test together the 40-bit window behind every bit of the run (the header ring as two 64-bit masks: values, and positions that hold a bit
//    at all — an 'x' does not), first match by ballot.  Bits behind an open header are written to the frame by the lanes of the run.
//  - -b (integrate-and-dump behind a header): one lane per bit, 64 bits a pass, each lane sums its bit's samples in reading order between
//    ceil((i-1) spb) and ceil(i spb) — bitgrenze accumulates a float in double, which is exact for the 512 bits of a frame.
// All state of the machine is wave-uniform (kept in scalar registers through readfirstlane); WxrChan carries it from call to call, so the
// frames do not depend on how a stream is cut into calls.  frame_bits lives in LDS during a call and in device memory between calls, and is
// never cleared: a frame that the end of the input cuts short keeps the previous frame's tail, as the reference's does.
#include "sonde_wxr_dev.h"

namespace {

typedef unsigned long long u64;
constexpr u64 M40 = (1ULL << WXR_HEADLEN) - 1;

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ u64 uni64(u64 v) {
    return ((u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

// f32read_signed_sample (:139-167): 8-bit unsigned and 16-bit signed PCM scaled to +-1, float as it is
__device__ __forceinline__ float load_sample(const WxrArgs &a, const char *row, int i) {
    const uint32_t k = (a.first + (uint32_t)i) & a.mask;
    if (a.kind == WXR_IN_S16) return (float)((const int16_t *)row)[k] / 32768.0f;
    if (a.kind == WXR_IN_U8) return (float)((int)((const uint8_t *)row)[k] - 128) / 128.0f;
    return ((const float *)row)[k];
}

// the ring after k more bits of value b (buf[] of main, newest bit lowest)
__device__ __forceinline__ void push_bits(u64 &hist, u64 &valid, int k, int b) {
    if (k >= WXR_HEADLEN) { hist = b ? M40 : 0; valid = M40; return; }
    const u64 ones = (1ULL << k) - 1;
    hist = ((hist << k) | (b ? ones : 0)) & M40;
    valid = ((valid << k) | ones) & M40;
}

__device__ void emit_frame(const WxrArgs &a, int c, const uint8_t *fb, u64 t_hdr, int lane) {
    __syncthreads();
    int idx = 0;
    if (lane == 0) idx = atomicAdd(a.q_count, 1);
    idx = uni(__shfl(idx, 0));
    if (idx < a.q_cap) {                                   // a full queue drops the frame; the host sees the count and reports it
        WxrFrame *f = a.q + idx;
        if (lane == 0) { f->channel = c; f->nbits = WXR_BITS; f->sample = t_hdr; }
        for (int j = lane; j < WXR_BITS; j += 64) f->bits[j] = fb[j];
    }
    __syncthreads();
}

__global__ __launch_bounds__(64) void k_wxr_slice(WxrArgs a) {
    __shared__ uint8_t fb[WXR_STRIDE];
    const int c = blockIdx.x, lane = threadIdx.x;
    uint8_t *fbg = a.frames + (size_t)c * WXR_STRIDE;
    for (int j = lane; j < WXR_STRIDE; j += 64) fb[j] = fbg[j];
    const WxrChan st0 = a.chan[c];
    const u64 total = uni64(st0.total);
    u64 t_hdr = uni64(st0.t_hdr), hist = uni64(st0.hist), valid = uni64(st0.valid);
    int n_run = uni((int)st0.n_run), scount = uni((int)st0.scount), par = uni(st0.par), found = uni(st0.found), bit_count = uni(st0.bit_count);
    int raw = uni(st0.raw), raw_i = uni(st0.raw_i);
    float sum = __int_as_float(uni(__float_as_int(st0.sum)));
    const char *row = (const char *)a.in + (size_t)c * (size_t)a.ch_stride * (a.kind == WXR_IN_S16 ? 2 : a.kind == WXR_IN_U8 ? 1 : 4);
    const double spb = (double)a.spb;
    __syncthreads();

    int pos = 0;
    while (pos < a.n) {
        if (raw) {
            // read_rawbit for the bits the frame still lacks: bit i (1-based since bitstart) ends with the first scount >= i * spb
            const int need = WXR_BITS - bit_count;
            const int S = scount + (a.n - pos);                          // scount at the end of this call's samples
            int done = 0, cut = 0;
            float psum = 0.f;
            for (int k = 0; k < need && !cut; k += 64) {
                const int i = raw_i + 1 + k + lane;
                const bool act = k + lane < need;
                const int b0 = (int)ceil((double)(i - 1) * spb), b1 = (int)ceil((double)i * spb);
                const int s0 = b0 > scount ? b0 : scount, s1 = b1 < S ? b1 : S;
                float acc = (k + lane == 0) ? sum : 0.f;
                if (act) for (int s = s0; s < s1; s++) acc += load_sample(a, row, pos + (s - scount));
                const bool full = act && b1 <= S;
                if (full) fb[bit_count + k + lane] = (uint8_t)((acc >= 0.f ? 1 : 0) ^ a.inv);
                const u64 mf = __ballot(full), mi = __ballot(act && !full);
                done += __popcll(mf);
                if (mi) { cut = 1; psum = __shfl(acc, __ffsll((long long)mi) - 1); }
            }
            done = uni(done);
            if (!cut) {                                                  // the frame is complete
                pos += (int)ceil((double)(raw_i + need) * spb) - scount;
                emit_frame(a, c, fb, t_hdr, lane);
                raw = 0; found = 0; bit_count = 0; raw_i = 0; scount = 0; sum = 0.f;
            } else {                                                     // the call ends inside bit raw_i + done + 1
                raw_i += done; bit_count += done; scount = S;
                sum = __int_as_float(uni(__float_as_int(psum)));
                pos = a.n;
            }
            continue;
        }
        // read_bits_fsk on 64 samples: a run ends with the first sample of the other sign, which is counted into it
        const int i = pos + lane;
        const bool v = i < a.n;
        const float x = v ? load_sample(a, row, i) : 0.f;
        const u64 V = __ballot(v), Sg = __ballot(v && x >= 0.f);
        const u64 P = (Sg << 1) | (par > 0 ? 1ULL : 0ULL);               // sign of the sample before
        const u64 Cm = (Sg ^ P) & V;
        const u64 below = Cm & ((1ULL << lane) - 1);
        const int nr = below ? lane - (63 - __clzll((long long)below)) : lane + 1 + n_run;
        const float lf = __fdiv_rn((float)nr, a.spb);
        const int len_v = (int)((double)lf + 0.5);
        const int bit_v = (int)((P >> lane) & 1) ^ a.inv;
        const int nvalid = __popcll(V);
        int consumed = nvalid, to_raw = 0;
        u64 rest = Cm;
        while (rest) {
            const int l = __ffsll((long long)rest) - 1;
            rest &= rest - 1;
            const int len = uni(__shfl(len_v, l)), b = uni(__shfl(bit_v, l));
            if (len == 0) {                                              // an 'x' goes into the ring, no bit
                hist = (hist << 1) & M40; valid = (valid << 1) & M40;
                continue;
            }
            int rem = len;
            while (rem > 0) {
                if (!found) {
                    // the window behind bit j of the run, for all j at once; behind 40 equal bits no header can end
                    const int t = rem < WXR_HEADLEN ? rem : WXR_HEADLEN;
                    bool hit = false;
                    if (lane < t) {
                        u64 h = hist, vv = valid;
                        push_bits(h, vv, lane + 1, b);
                        hit = h == a.hdr && vv == M40;
                    }
                    const u64 hm = __ballot(hit);
                    if (hm) {
                        const int j = __ffsll((long long)hm) - 1;
                        push_bits(hist, valid, j + 1, b);
                        rem -= j + 1;
                        found = 1;
                        t_hdr = total + (u64)(pos + l + 1);
                        __syncthreads();
                        if (lane < WXR_HEADLEN) fb[lane] = (uint8_t)((a.hdr >> (WXR_HEADLEN - 1 - lane)) & 1);
                        bit_count += WXR_HEADLEN;
                    } else {
                        push_bits(hist, valid, rem, b);
                        rem = 0;
                    }
                } else {
                    const int room = WXR_BITS - bit_count;
                    const int k = rem < room ? rem : room;
                    for (int j = lane; j < k; j += 64) fb[bit_count + j] = (uint8_t)b;
                    push_bits(hist, valid, k, b);
                    bit_count += k; rem -= k;
                }
                if (bit_count >= WXR_BITS) {
                    emit_frame(a, c, fb, t_hdr, lane);
                    bit_count = 0; found = 0;
                }
            }
            if (found && a.opt_b) {                                      // bitstart: the -b loop takes over behind this sample
                raw = 1; raw_i = 0; scount = 0; sum = 0.f;
                consumed = l + 1; to_raw = 1;
                break;
            }
        }
        par = ((Sg >> (consumed - 1)) & 1) ? 1 : -1;
        if (to_raw) n_run = 0;
        else n_run = Cm ? (nvalid - 1) - (63 - __clzll((long long)Cm)) : n_run + nvalid;
        pos += consumed;
    }

    __syncthreads();
    for (int j = lane; j < WXR_STRIDE; j += 64) fbg[j] = fb[j];
    if (lane == 0) {
        WxrChan st;
        st.total = total + (u64)a.n; st.t_hdr = t_hdr; st.hist = hist; st.valid = valid;
        st.n_run = (uint32_t)n_run; st.scount = (uint32_t)scount; st.sum = sum;
        st.par = par; st.found = found; st.bit_count = bit_count; st.raw = raw; st.raw_i = raw_i;
        a.chan[c] = st;
    }
}

}  // namespace

extern "C" int sonde_launch_wxr(const WxrArgs *a, hipStream_t s) {
    if (a->n_ch < 1 || a->n < 1) return 0;
    hipLaunchKernelGGL(k_wxr_slice, dim3(a->n_ch), dim3(64), 0, s, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
