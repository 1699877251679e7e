// sonde_slice_dev.h — the FM bit slicer that k_wxr_slice (sonde_wxr.hip) and k_drop_slice (sonde_drop.hip) instantiate: read_bits_fsk,
// read_rawbit and the frame loop of main of the reference's weathex301d.c and rd94rd41drop.c, on the FM samples of many channels, one
// wavefront per channel.  The records are shared with the host engines (sonde_wxr.cpp, sonde_drop.cpp).
//
// The reference is a state machine from frame to frame, but each of its two phases is data-parallel over a stretch of samples:
//  - search (no -b frame open): 64 samples at a time.  Sign bits (sample >= 0) by ballot, sign changes = ends of runs, every change lane
//    computes its run's length in bits with the reference's float division; the wave then takes the few runs of the tile in order, and for
//    each the lanes test together the 40-bit window behind every bit of the run (the header ring as two 64-bit masks: values, and positions
//    that hold a bit at all), first match by ballot.  Bits behind an open header are written to the frame by the lanes of the run.
//  - -b (integrate-and-dump behind a header): one lane per bit, 64 bits a pass, each lane sums its bit's samples in reading order.  Bit i
//    (from 1, counted from the sample behind the run's last) takes the samples [ceil((i-1) spb) - EDGE, ceil(i spb) - EDGE), the first bit
//    starting at 0.  i * spb is exact in double (12 x 24 bits), and so is the reference's accumulation of a float in double for the bits of
//    a frame, so the two agree.
// All state of the machine is wave-uniform (kept in scalar registers through readfirstlane); SliceChan carries it from call to call, so the
// frames do not depend on how a stream is cut into calls.  The frame's bits live in LDS during a call and in device memory between calls,
// and are never cleared: a frame that the end of the input cuts short keeps the previous frame's tail, as the reference's does.
//
// What differs between the two decoders is a traits struct T:
//   sample_t, Args            float / int samples; SliceArgs<sample_t, frame record>
//   load_sample, sample_bytes the input kinds
//   BITS, STRIDE              bits of a frame, and of a channel's frame in LDS and device memory
//   EDGE                      the bit-boundary offset above
//   ZERO_RUN_X                a run of 0 bits shifts a position without a bit ('x') into the ring / leaves no trace
//   HDR_PRESET                bit_count runs from 40 and the frame keeps the header in front from the start / runs from 0, and a match
//                             writes the header into the frame
//   RAW_INTO_RING             after a -b frame the ring holds the frame's last 40 bits / is as the header match left it
//   FINISH                    a.finish (end of the input, n = 0) completes a -b frame whose header is open
//   header(a)                 the 40 header bits, first bit highest
//   complete(...)             hands a frame to the queue; called by the whole wavefront
#ifndef SONDE_SLICE_DEV_H
#define SONDE_SLICE_DEV_H
#include <hip/hip_runtime.h>
#include <cstdint>

#define SLICE_HEADLEN 40

// per-channel state between calls: the globals and main() locals of the reference that outlive a sample
template <class S> struct SliceChan {
    unsigned long long total;          // sample_count
    unsigned long long t_hdr;          // sample_count when the open header matched
    unsigned long long hist, valid;    // buf[40]: bit values, and which positions hold a bit at all ('x' and the initial bytes do not)
    uint32_t n_run;                    // read_bits_fsk's n of the run in progress
    uint32_t scount;                   // read_rawbit: samples since bitstart
    S sum;                             // read_rawbit: sum of the bit in progress
    int32_t par, found, bit_count, raw, raw_i;   // raw: inside the -b loop; raw_i: bits it has finished since bitstart
};
static_assert(sizeof(SliceChan<float>) == 64 && sizeof(SliceChan<int32_t>) == 64, "the state record lives in device memory between calls");

template <class S, class Frame> struct SliceArgs {
    SliceChan<S> *chan;
    uint8_t *frames;                   // [n_ch][STRIDE]: the frame bits of every channel between calls
    Frame *q;
    int *q_count;
    const void *in;
    unsigned long long hdr;            // the 40 header bits, first bit highest: WxR, which has two; unused by the dropsonde (DROP_HDR40)
    long long ch_stride;               // samples between two channels of `in`
    uint32_t first, mask;              // sample i of the call is in[(first + i) & mask]
    int q_cap, n_ch, n, kind, inv, opt_b, finish;
    float spb;
    // channels handed out at run time (the RT form of slice(); unused, and behind every field the other form reads, otherwise)
    int *active;                       // 0: the channel's workgroup returns before it reads anything
    int ch0;                           // workgroup b works on channel ch0 + b (a launch for one channel: its finish)
};

#ifdef __HIPCC__
namespace sonde_slice {

typedef unsigned long long u64;
constexpr u64 M40 = (1ULL << SLICE_HEADLEN) - 1;

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uni(float v) { return __int_as_float(uni(__float_as_int(v))); }
__device__ __forceinline__ u64 uni64(u64 v) {
    return ((u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

// the ring after k more bits of value b (buf[] of main, newest bit lowest)
__device__ __forceinline__ void push_bits(u64 &hist, u64 &valid, int k, int b) {
    if (k >= SLICE_HEADLEN) { hist = b ? M40 : 0; valid = M40; return; }
    const u64 ones = (1ULL << k) - 1;
    hist = ((hist << k) | (b ? ones : 0)) & M40;
    valid = ((valid << k) | ones) & M40;
}

// (a by value, as the kernel gets it; the register counts of both forms are in profiles/wxr_rocprofv3.txt and profiles/drop_rocprofv3.txt)
// RT: the engine's channels are handed out at run time — the active mask, and a launch that starts at channel a.ch0 (one channel finished on its own).  RT = false
// is the slicer as it was before run-time channels, instruction for instruction.
template <class T, bool RT = false> __device__ __forceinline__ void slice(const typename T::Args a) {
    typedef typename T::sample_t S;
    constexpr int BIT0 = T::HDR_PRESET ? SLICE_HEADLEN : 0;              // bit_count while no header is open
    __shared__ uint8_t fb[T::STRIDE];
    const int c = RT ? (int)blockIdx.x + a.ch0 : (int)blockIdx.x, lane = threadIdx.x;
    if (RT && !a.active[c]) return;                                      // a released channel: nothing read, nothing written
    uint8_t *fbg = a.frames + (size_t)c * T::STRIDE;
    for (int j = lane; j < T::STRIDE; j += 64) fb[j] = fbg[j];
    const SliceChan<S> st0 = a.chan[c];
    const u64 total = uni64(st0.total);
    u64 t_hdr = uni64(st0.t_hdr), hist = uni64(st0.hist), valid = uni64(st0.valid);
    int n_run = uni((int)st0.n_run), scount = uni((int)st0.scount), par = uni(st0.par), found = uni(st0.found), bit_count = uni(st0.bit_count);
    int raw = uni(st0.raw), raw_i = uni(st0.raw_i);
    S sum = uni(st0.sum);
    const char *row = (const char *)a.in + (size_t)c * (size_t)a.ch_stride * T::sample_bytes(a.kind);
    const double spb = (double)a.spb;
    __syncthreads();

    int pos = 0;
    while (pos < a.n) {
        if (raw) {
            // read_rawbit for the bits the frame still lacks; scount = samples read since bitstart
            const int need = T::BITS - bit_count;
            const int S1 = scount + (a.n - pos);                         // scount at the end of this call's samples
            int done = 0, cut = 0;
            S psum = 0;
            for (int k = 0; k < need && !cut; k += 64) {
                const int i = raw_i + 1 + k + lane;
                const bool act = k + lane < need;
                int b0 = (int)ceil((double)(i - 1) * spb) - T::EDGE;
                const int b1 = (int)ceil((double)i * spb) - T::EDGE;
                if (T::EDGE && b0 < 0) b0 = 0;
                const int s0 = b0 > scount ? b0 : scount, s1 = b1 < S1 ? b1 : S1;
                S acc = (k + lane == 0) ? sum : (S)0;
                if (act) for (int s = s0; s < s1; s++) acc += T::load_sample(a, row, pos + (s - scount));
                const bool full = act && b1 <= S1;
                if (full) fb[bit_count + k + lane] = (uint8_t)((acc >= (S)0 ? 1 : 0) ^ a.inv);
                const u64 mf = __ballot(full), mi = __ballot(act && !full);
                done += __popcll(mf);
                if (mi) { cut = 1; psum = __shfl(acc, __ffsll((long long)mi) - 1); }
            }
            done = uni(done);
            if (!cut) {                                                  // the frame is complete
                pos += (int)ceil((double)(raw_i + need) * spb) - T::EDGE - scount;
                T::complete(a, c, fb, T::BITS, t_hdr, 1, lane);
                if (T::RAW_INTO_RING) {
                    const u64 tail = __ballot(lane < SLICE_HEADLEN && fb[T::BITS - SLICE_HEADLEN + lane]);
                    hist = uni64(__brevll(tail) >> 24); valid = M40;
                }
                raw = 0; found = 0; bit_count = BIT0; raw_i = 0; scount = 0; sum = 0;
            } else {                                                     // the call ends inside bit raw_i + done + 1
                raw_i += done; bit_count += done; scount = S1;
                sum = uni(psum);
                pos = a.n;
            }
            continue;
        }
        // read_bits_fsk on 64 samples: a run ends with the first sample of the other sign, which is counted into it
        const int i = pos + lane;
        const bool v = i < a.n;
        const S x = v ? T::load_sample(a, row, i) : (S)0;
        const u64 V = __ballot(v), Sg = __ballot(v && x >= (S)0);
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
            if (T::ZERO_RUN_X && len == 0) { hist = (hist << 1) & M40; valid = (valid << 1) & M40; continue; }
            int rem = len;
            while (rem > 0) {
                if (!found) {
                    // the window behind bit j of the run, for all j at once; behind 40 equal bits no header can end
                    const int t = rem < SLICE_HEADLEN ? rem : SLICE_HEADLEN;
                    bool hit = false;
                    if (lane < t) {
                        u64 h = hist, vv = valid;
                        push_bits(h, vv, lane + 1, b);
                        hit = h == T::header(a) && vv == M40;
                    }
                    const u64 hm = __ballot(hit);
                    if (hm) {
                        const int j = __ffsll((long long)hm) - 1;
                        push_bits(hist, valid, j + 1, b);
                        rem -= j + 1;
                        found = 1;
                        t_hdr = total + (u64)(pos + l + 1);
                        if (!T::HDR_PRESET) {
                            __syncthreads();
                            if (lane < SLICE_HEADLEN) fb[lane] = (uint8_t)((T::header(a) >> (SLICE_HEADLEN - 1 - lane)) & 1);
                        }
                        bit_count = SLICE_HEADLEN;
                    } else {
                        push_bits(hist, valid, rem, b);
                        rem = 0;
                    }
                } else {
                    const int room = T::BITS - bit_count;
                    const int k = rem < room ? rem : room;
                    for (int j = lane; j < k; j += 64) fb[bit_count + j] = (uint8_t)b;
                    push_bits(hist, valid, k, b);
                    bit_count += k; rem -= k;
                    if (bit_count >= T::BITS) {
                        T::complete(a, c, fb, T::BITS, t_hdr, 1, lane);
                        bit_count = BIT0; found = 0;
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

    if (T::FINISH && a.finish && found && a.opt_b) {                     // EOF inside read_rawbit: the frame as far as it got
        T::complete(a, c, fb, bit_count, t_hdr, 0, lane);
        found = 0; raw = 0; bit_count = BIT0;
    }
    __syncthreads();
    for (int j = lane; j < T::STRIDE; j += 64) fbg[j] = fb[j];
    if (lane == 0) {
        SliceChan<S> st;
        st.total = total + (u64)a.n; st.t_hdr = t_hdr; st.hist = hist; st.valid = valid;
        st.n_run = (uint32_t)n_run; st.scount = (uint32_t)scount; st.sum = sum;
        st.par = par; st.found = found; st.bit_count = bit_count; st.raw = raw; st.raw_i = raw_i;
        a.chan[c] = st;
    }
}

}  // namespace sonde_slice
#endif
#endif
