// sonde_drop.hip — k_drop_slice: the bit slicer of the reference's dropsonde/rd94rd41drop.c (read_bits_fsk :207, read_rawbit :242, the
// frame loop of main :1399-1446) on the integer FM samples of many channels, one wavefront per channel, and the completion of a finished
// frame on the device (drop_complete_frame: Manchester pairs -> bytes -> both check masks).
//
// The reference is a state machine from frame to frame, but each of its two phases is data-parallel over a stretch of samples:
//  - search (no -b frame open): 64 samples at a time.  Sign bits (sample >= 0) by ballot, sign changes = ends of runs, every change lane
//    computes its run's length in raw bits with the reference's float division; the wave then takes the few runs of the tile in order, and
//    for each the lanes test together the 40-bit window behind every bit of the run (the header ring as two 64-bit masks: values, and
//    positions that hold a bit at all).  A run of 0 bits leaves no trace.  Bits behind an open header are written to the frame by the
//    lanes of the run.
//  - -b (integrate-and-dump behind a header): one lane per raw bit, 64 bits a pass, each lane sums its bit's samples as integers in
//    reading order.  Bit i (from 1) ends with the sample that makes sample_count >= bitgrenze = sc0 - 1 + i * spb; counted from the
//    sample behind the run's last, those are the samples [ceil((i-1) spb) - 1, ceil(i spb) - 1), the first bit starting at 0.  i * spb
//    is exact in double (12 x 24 bits), and so is the reference's accumulation for sample counts below 2^33, so the two agree there.
//    The bits also enter the ring: after a full frame it holds the frame's last 40 raw bits.
// All state of the machine is wave-uniform (kept in scalar registers through readfirstlane); DropChan carries it from call to call, so the
// frames do not depend on how a stream is cut into calls.  frame_rawbits lives in LDS during a call and in device memory between calls.
// With a.finish set (end of the input, n = 0) a -b frame whose header is open is completed with '0' bits (print_bitframe :1253).
#include "sonde_drop_dev.h"

namespace {

typedef unsigned long long u64;
constexpr u64 M40 = (1ULL << DROP_HEADLEN) - 1;

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ u64 uni64(u64 v) {
    return ((u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

// read_signed_sample (:179-202): 16-bit signed, 8-bit unsigned minus 128; the ring through fwrite_fm_blk's 16-bit conversion of iq_dec
// (x *= 128; x *= 256; (short)x — truncation, wrapping as the x86 conversion does)
__device__ __forceinline__ int load_sample(const DropArgs &a, const char *row, int i) {
    const uint32_t k = (a.first + (uint32_t)i) & a.mask;
    if (a.kind == DROP_IN_S16) return (int)((const int16_t *)row)[k];
    if (a.kind == DROP_IN_U8) return (int)((const uint8_t *)row)[k] - 128;
    float v = ((const float *)row)[k] * 128.0f;
    v *= 256.0f;
    return (int)(int16_t)(int)v;
}

// the ring after k more bits of value b (buf[] of main, newest bit lowest)
__device__ __forceinline__ void push_bits(u64 &hist, u64 &valid, int k, int b) {
    if (k >= DROP_HEADLEN) { hist = b ? M40 : 0; valid = M40; return; }
    const u64 ones = (1ULL << k) - 1;
    hist = ((hist << k) | (b ? ones : 0)) & M40;
    valid = ((valid << k) | ones) & M40;
}

__global__ __launch_bounds__(64) void k_drop_slice(DropArgs a) {
    __shared__ uint8_t fb[DROP_RAWBITS];
    __shared__ uint8_t by[128];
    const int c = blockIdx.x, lane = threadIdx.x;
    uint8_t *fbg = a.frames + (size_t)c * DROP_RAWBITS;
    for (int j = lane; j < DROP_RAWBITS; j += 64) fb[j] = fbg[j];
    const DropChan st0 = a.chan[c];
    const u64 total = uni64(st0.total);
    u64 t_hdr = uni64(st0.t_hdr), hist = uni64(st0.hist), valid = uni64(st0.valid);
    int n_run = uni((int)st0.n_run), scount = uni((int)st0.scount), par = uni(st0.par), found = uni(st0.found), bit_count = uni(st0.bit_count);
    int raw = uni(st0.raw), raw_i = uni(st0.raw_i), sum = uni(st0.sum);
    const char *row = (const char *)a.in + (size_t)c * (size_t)a.ch_stride * (a.kind == DROP_IN_S16 ? 2 : a.kind == DROP_IN_U8 ? 1 : 4);
    const double spb = (double)a.spb;
    __syncthreads();

    int pos = 0;
    while (pos < a.n) {
        if (raw) {
            // read_rawbit for the bits the frame still lacks; scount = samples read since bitstart
            const int need = DROP_RAWBITS - bit_count;
            const int S = scount + (a.n - pos);                          // scount at the end of this call's samples
            int done = 0, cut = 0, psum = 0;
            for (int k = 0; k < need && !cut; k += 64) {
                const int i = raw_i + 1 + k + lane;
                const bool act = k + lane < need;
                const int e0 = (int)ceil((double)(i - 1) * spb) - 1, b1 = (int)ceil((double)i * spb) - 1;
                const int b0 = e0 > 0 ? e0 : 0;
                const int s0 = b0 > scount ? b0 : scount, s1 = b1 < S ? b1 : S;
                int acc = (k + lane == 0) ? sum : 0;
                if (act) for (int s = s0; s < s1; s++) acc += load_sample(a, row, pos + (s - scount));
                const bool full = act && b1 <= S;
                if (full) fb[bit_count + k + lane] = (uint8_t)((acc >= 0 ? 1 : 0) ^ a.inv);
                const u64 mf = __ballot(full), mi = __ballot(act && !full);
                done += __popcll(mf);
                if (mi) { cut = 1; psum = __shfl(acc, __ffsll((long long)mi) - 1); }
            }
            done = uni(done);
            if (!cut) {                                                  // the frame is complete
                pos += (int)ceil((double)(raw_i + need) * spb) - 1 - scount;
                drop_complete_frame(fb, DROP_RAWBITS, by, a.q, a.q_count, a.q_cap, c, t_hdr, 1, lane);
                const u64 tail = __ballot(lane < DROP_HEADLEN && fb[DROP_RAWBITS - DROP_HEADLEN + lane]);
                hist = uni64(__brevll(tail) >> 24); valid = M40;
                raw = 0; found = 0; bit_count = DROP_HEADLEN; raw_i = 0; scount = 0; sum = 0;
            } else {                                                     // the call ends inside bit raw_i + done + 1
                raw_i += done; bit_count += done; scount = S;
                sum = uni(psum);
                pos = a.n;
            }
            continue;
        }
        // read_bits_fsk on 64 samples: a run ends with the first sample of the other sign, which is counted into it
        const int i = pos + lane;
        const bool v = i < a.n;
        const int x = v ? load_sample(a, row, i) : 0;
        const u64 V = __ballot(v), Sg = __ballot(v && x >= 0);
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
            int rem = len;                                               // len == 0: `continue` in main, nothing enters the ring
            while (rem > 0) {
                if (!found) {
                    // the window behind bit j of the run, for all j at once; behind 40 equal bits no header can end
                    const int t = rem < DROP_HEADLEN ? rem : DROP_HEADLEN;
                    bool hit = false;
                    if (lane < t) {
                        u64 h = hist, vv = valid;
                        push_bits(h, vv, lane + 1, b);
                        hit = h == DROP_HDR40 && vv == M40;
                    }
                    const u64 hm = __ballot(hit);
                    if (hm) {
                        const int j = __ffsll((long long)hm) - 1;
                        push_bits(hist, valid, j + 1, b);
                        rem -= j + 1;
                        found = 1;
                        t_hdr = total + (u64)(pos + l + 1);
                        bit_count = DROP_HEADLEN;                        // fb[0..40) holds the header from the start
                    } else {
                        push_bits(hist, valid, rem, b);
                        rem = 0;
                    }
                } else {
                    const int room = DROP_RAWBITS - bit_count;
                    const int k = rem < room ? rem : room;
                    for (int j = lane; j < k; j += 64) fb[bit_count + j] = (uint8_t)b;
                    push_bits(hist, valid, k, b);
                    bit_count += k; rem -= k;
                    if (bit_count >= DROP_RAWBITS) {
                        drop_complete_frame(fb, DROP_RAWBITS, by, a.q, a.q_count, a.q_cap, c, t_hdr, 1, lane);
                        bit_count = DROP_HEADLEN; found = 0;
                    }
                }
            }
            if (found && a.opt_b) {                                      // bitstart: the -b loop takes over behind this sample
                raw = 1; raw_i = 0; scount = 0; sum = 0;
                consumed = l + 1; to_raw = 1;
                break;
            }
        }
        par = ((Sg >> (consumed - 1)) & 1) ? 1 : -1;
        if (to_raw) n_run = 0;
        else n_run = Cm ? (nvalid - 1) - (63 - __clzll((long long)Cm)) : n_run + nvalid;
        pos += consumed;
    }

    if (a.finish && found && a.opt_b) {                                  // EOF inside read_rawbit: break, print_bitframe(pos)
        drop_complete_frame(fb, bit_count, by, a.q, a.q_count, a.q_cap, c, t_hdr, 0, lane);
        found = 0; raw = 0; bit_count = DROP_HEADLEN;
    }
    __syncthreads();
    for (int j = lane; j < DROP_RAWBITS; j += 64) fbg[j] = fb[j];
    if (lane == 0) {
        DropChan st;
        st.total = total + (u64)a.n; st.t_hdr = t_hdr; st.hist = hist; st.valid = valid;
        st.n_run = (uint32_t)n_run; st.scount = (uint32_t)scount; st.sum = sum;
        st.par = par; st.found = found; st.bit_count = bit_count; st.raw = raw; st.raw_i = raw_i;
        a.chan[c] = st;
    }
}

}  // namespace

extern "C" int sonde_launch_drop(const DropArgs *a, hipStream_t s) {
    if (a->n_ch < 1 || (a->n < 1 && !a->finish)) return 0;
    hipLaunchKernelGGL(k_drop_slice, dim3(a->n_ch), dim3(64), 0, s, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
