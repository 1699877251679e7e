// sonde_imet4.hip — the iMet-4 / iMet-1-RS receiver on the device (include/sonde_imet4.h): k_imet4_afsk, one wavefront per channel.
//
// Per channel the reference (imet/imet4iq.c) is one sample loop: front end f32_sample :445-578 (IQ-dc removal of f32read_cblock :305-350,
// LUT mixer, --dc rotation, IF low-pass, FM discriminator, FM low-pass, --dc subtraction of FM audio), the AFC of :541-571 (a float running
// sum over M = 32 sps samples; once per second, at (sample_in + pre_pos) % sr == 0, Df += 0.5 * sr * dc / 1.6 and the IF tap set switches
// at |dDf| = 2 kHz), the two-tone sliding DFT :1550-1573 and the slicer :1575-1636.  The slicer re-phases the AFC schedule (pre_pos) at
// every header, so the chain is causal across all of it.  The wave walks its chunk in tiles of at most 64 samples (one per lane):
//   - a tile never crosses an AFC update point or an IQ-dc block end, so Df, the tap set and the IQ-dc average are constant inside it;
//   - lanes run the front end and D = X - X0 of both tones (the per-sample double sincos) in parallel; the float xsum recursion, the
//     IQ-dc sums and F += D are exact in-order ladders over the lanes (readlane), as the reference adds them;
//   - |F2| - |F1| per lane, the decisions ballot into a 64-bit mask, and the slicer runs over the mask as wave-uniform code;
//   - the tile is committed up to its last sample, or up to a header: a header moves the next update point, and the samples behind it
//     are computed again in the next tile under the schedule it implies.  Rings hold history by absolute sample index, so samples a
//     truncated tile computed ahead are simply overwritten; the AFC's M-entry ring is written only for committed samples.
// Complete 1000-bit frames go to a device queue.  With decM > 1, k_imet4_decim produces the IF samples first.
// Input is 8-bit unsigned, 16-bit signed or float32 (taken as it is, imet4iq.c:235-237, 265-270, 329-332); a.bits is uniform over the launch.
// Both kernels have two instantiations, picked per launch (a.rt): see k_imet4_afsk.
// Channels are handed out at run time: a.active[c] == 0 ends a channel's workgroup before it reads anything, k_imet4_restart makes a channel
// what create builds (sonde_imet4_restart_channel), and a channel's input row starts at c * a.ch_stride samples.
//
// Floating-point contraction is off in this file: the reference is plain C on x86-64 (every product and sum rounded on its own).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <cstdint>
#include "sonde_imet4_dev.h"

namespace {

constexpr double kTwoPi = 6.2831853071795864769252867665590;
constexpr double kPi = 3.1415926535897932384626433832795;

__device__ __forceinline__ float rl(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }
__device__ __forceinline__ double rl(double v, int k) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffLL), k), hi = __builtin_amdgcn_readlane((int)(b >> 32), k);
    return __longlong_as_double(((long long)(unsigned)lo) | ((long long)hi << 32));
}

// lowpass() / re_lowpass() of the reference: buffer slot n holds the newest sample m <= s with m % T == n, weight ws[T - (s+1) % T + n]
// of the duplicated table; summed over n in slot order.  Samples before the stream start are the zeroed buffer.
__device__ __forceinline__ void fir_c(const float2 *ring, unsigned long long s, int T, const float *ws2, unsigned long long mask, float &wr, float &wi) {
    const int r = (int)(s % (unsigned long long)T), S = T - (int)((s + 1) % (unsigned long long)T);
    float ar = 0.f, ai = 0.f;
    for (int n = 0; n < T; n++) {
        const int back = (r - n + T) % T;
        float2 z = make_float2(0.f, 0.f);
        if ((unsigned long long)back <= s) z = ring[(s - back) & mask];
        const float w = ws2[S + n];
        ar = ar + z.x * w;
        ai = ai + z.y * w;
    }
    wr = ar; wi = ai;
}
__device__ __forceinline__ float fir_r(const float *ring, uint32_t s, int T, const float *ws2, uint32_t mask) {
    const int r = (int)(s % (uint32_t)T), S = T - (int)((s + 1) % (uint32_t)T);
    float a = 0.f;
    for (int n = 0; n < T; n++) {
        const int back = (r - n + T) % T;
        const float x = ((uint32_t)back <= s) ? ring[(s - back) & mask] : 0.f;
        a = a + x * ws2[S + n];
    }
    return a;
}

__device__ __forceinline__ void emit(const Imet4Args &a, int c, Imet4Chan &st, uint8_t *frame, uint32_t sc) {
    __syncthreads();                                   // frame bits written by lane 0
    __shared__ int slot;
    if (threadIdx.x == 0) slot = atomicAdd(a.q_count, 1);
    __syncthreads();
    const int q = slot;
    if (q < a.q_cap) {
        Imet4Frame *f = a.q + q;
        for (int i = threadIdx.x; i < IMET4_FRAME_BITS; i += 64) f->bits[i] = frame[i];
        if (threadIdx.x == 0) { f->channel = c; f->nbits = IMET4_FRAME_BITS; f->sample = st.sample_hi + sc; }
    }
    __syncthreads();
}

}  // namespace

// RT: the engine's channels are handed out at run time or its samples are float32 — the active mask, the row stride and the float loads.
// The launch picks RT = false where none of that is in use (8- / 16-bit samples, every channel active, rows n apart): that instantiation is
// the kernel as it was before run-time channels, instruction for instruction.
template <bool RT> __global__ __launch_bounds__(64) void k_imet4_afsk(const Imet4Args a) {
    const int c = blockIdx.x, lane = threadIdx.x;
    if (RT && !a.active[c]) return;                                    // a released channel: nothing read, nothing written
    Imet4Chan st = a.chan[c];
    const uint32_t rmask = (uint32_t)a.ring - 1;
    float2 *zring = a.zring + (size_t)c * a.ring;
    float *fmring = a.fmring + (size_t)c * a.ring;
    float *xring = a.xring + (size_t)c * a.ring;
    const float2 *ifin = a.ifbuf + (size_t)c * a.if_stride;
    float *bufs = a.bufs + (size_t)c * a.M;
    uint8_t *frame = a.frames + (size_t)c * IMET4_FRAME_STRIDE;
    const size_t in_stride = (RT ? (size_t)a.ch_stride : (size_t)a.n) * (a.iq ? 2 : 1);
    const uint8_t *in8 = (const uint8_t *)a.in + (a.bits == 8 ? in_stride * c : 0);
    const int16_t *in16 = (const int16_t *)a.in + (a.bits == 16 ? in_stride * c : 0);
    const float *in32 = (const float *)a.in + (RT && a.bits == 32 ? in_stride * c : 0);
    const double bitlen = a.bitlen;
    const int nlag = (int)bitlen;

    int done = 0;
    while (done < a.n) {
        const uint32_t s0 = st.sample;
        // the tile ends at the next AFC update point (inclusive) and at the end of the IQ-dc block in progress
        const uint32_t du = a.dc ? ((s0 + st.pre_pos) % (uint32_t)a.sr ? (uint32_t)a.sr - (s0 + st.pre_pos) % (uint32_t)a.sr : 0u) : 0xffffffffu;
        const uint32_t left = (a.iq && !a.pre) ? st.maxcnt - st.cnt : 0xffffffffu;
        int L = min(64, a.n - done);
        if (du < (uint32_t)L) L = (int)du + 1;
        if (left < (uint32_t)L) L = (int)left;
        const bool upd = du == (uint32_t)(L - 1), blk = left == (uint32_t)L;
        const bool act = lane < L;
        const uint32_t s = s0 + (uint32_t)lane;
        const size_t ix = (size_t)done + lane;

        // ---- front end
        float v = 0.f, zr = 0.f, zi = 0.f;
        float xin = 0.f, yin = 0.f;
        if (a.iq) {
            if (a.pre) {                                               // IF samples of k_imet4_decim (IQ-dc, mixer, decimator done)
                if (act) { const float2 z = ifin[ix]; zr = z.x; zi = z.y; }
            } else {
                if (act) {
                    if (RT && a.bits == 32) { const float2 z = ((const float2 *)in32)[ix]; xin = z.x; yin = z.y; }   // float32: as it is (imet4iq.c:265-270)
                    else if (a.bits == 16) { xin = (float)(in16[2 * ix] / 32768.0); yin = (float)(in16[2 * ix + 1] / 32768.0); }
                    else { xin = (float)((in8[2 * ix] - 128) / 128.0); yin = (float)((in8[2 * ix + 1] - 128) / 128.0); }
                }
                const float br = xin - st.avgx, bi = yin - st.avgy;
                // LUT mixer: ex[sample % lut_len] = (float complex)cexp(2 pi i f0 n)
                const uint32_t k = s % (uint32_t)st.lut_len;
                double sn, cs;
                sincos((st.f0 * (double)k) * kTwoPi, &sn, &cs);
                const float er = (float)cs, ei = (float)sn;
                zr = br * er - bi * ei;
                zi = br * ei + bi * er;
            }
            if (a.dc) {
                const double t = s / (double)a.sr;
                double sn, cs;
                sincos(((-t) * kTwoPi) * st.Df, &sn, &cs);
                const double dr = (double)zr, di = (double)zi;
                zr = (float)(dr * cs - di * sn);
                zi = (float)(dr * sn + di * cs);
            }
            if (a.lp_iq) {
                if (act) zring[s & rmask] = make_float2(zr, zi);
                __syncthreads();
                const float *ws2 = (a.dc && !st.locked) ? a.ws_iq0 : a.ws_iq1;
                if (act) fir_c(zring, s, a.taps_iq, ws2, rmask, zr, zi);
            }
            float pr = __shfl_up(zr, 1), pi_ = __shfl_up(zi, 1);
            if (lane == 0) { pr = st.prevr; pi_ = st.previ; }
            // w = z * conj(z0): conj() is the double function, so the reference forms the product in double (the float products are exact
            // there) and rounds each part once to float (:505-507); float products rounded one by one differ from that in the last bit
            const float wr = (float)((double)zr * (double)pr + (double)zi * (double)pi_);
            const float wi = (float)((double)zi * (double)pr - (double)zr * (double)pi_);
            v = (float)(0.8 * atan2((double)wi, (double)wr) / kPi);
        } else if (act) {
            if (RT && a.bits == 32) v = in32[ix];                                                              // imet4iq.c:235-237
            else if (a.bits == 16) v = (float)((float)(in16[ix] / 128.0) / 256.0);
            else v = (float)((in8[ix] - 128) / 128.0);
        }
        if (a.lp_fm) {
            if (act) fmring[s & rmask] = v;
            __syncthreads();
            if (act) v = fir_r(fmring, s, a.taps_fm, a.ws_fm, rmask);
        }
        if (a.dc && !a.iq) v = (float)(v - st.dc * 0.4);

        // ---- AFC running sum: xsum += bufs[s % M] - bufs[(s+1) % M] (the slot of sample s + 1 - M), in order
        const float xalt = act ? bufs[(s + 1) % (uint32_t)a.M] : 0.f;
        const float dx = v - xalt;
        float xs = st.xsum, my_xs = 0.f;
        double sx = st.sumx, sy = st.sumy, my_sx = 0, my_sy = 0;
        for (int k = 0; k < L; k++) {
            xs = xs + rl(dx, k);
            if (a.iq && !a.pre) { sx = sx + (double)rl(xin, k); sy = sy + (double)rl(yin, k); }
            if (lane == k) { my_xs = xs; my_sx = sx; my_sy = sy; }
        }

        // ---- two-tone sliding DFT: F += X - X0, X0 = X of sample s - floor(bitlen) (the zeroed ring before the start)
        if (act) xring[s & rmask] = v;
        __syncthreads();
        const float x0 = (act && s >= (uint32_t)nlag) ? xring[(s - nlag) & rmask] : 0.f;
        const double t = s / (double)a.sr, tn = (uint32_t)(s - (uint32_t)nlag) / (double)a.sr;
        double d1r, d1i, d2r, d2i;
        {
            double sn, cs, sn0, cs0;
            const double x = v, xo = x0;
            sincos((-t) * a.w1, &sn, &cs); sincos((-tn) * a.w1, &sn0, &cs0);
            d1r = x * cs - xo * cs0; d1i = x * sn - xo * sn0;
            sincos((-t) * a.w2, &sn, &cs); sincos((-tn) * a.w2, &sn0, &cs0);
            d2r = x * cs - xo * cs0; d2i = x * sn - xo * sn0;
        }
        double f1r = st.F1r, f1i = st.F1i, f2r = st.F2r, f2i = st.F2i;
        double m1r = 0, m1i = 0, m2r = 0, m2i = 0;
        for (int k = 0; k < L; k++) {
            f1r = f1r + rl(d1r, k); f1i = f1i + rl(d1i, k);
            f2r = f2r + rl(d2r, k); f2i = f2i + rl(d2i, k);
            if (lane == k) { m1r = f1r; m1i = f1i; m2r = f2r; m2i = f2i; }
        }
        const double xbit = sqrt(m2r * m2r + m2i * m2i) - sqrt(m1r * m1r + m1i * m1i);
        const float sb = (float)(xbit / bitlen);
        const unsigned long long mask = __ballot(act && !(sb < 0));

        // ---- slicer over the mask (wave-uniform)
        int stop = L - 1;
        for (int k = 0; k < L; k++) {
            const uint32_t sc = s0 + (uint32_t)k;
            const int bit = (int)((mask >> k) & 1ULL);
            bool hit = false;
            const uint32_t b3 = sc % 3;
            if (b3 == 0) st.bb0 = bit; else if (b3 == 1) st.bb1 = bit; else st.bb2 = bit;
            if (st.hf) {
                if ((double)sc - st.pos_bit > bitlen + bitlen / 5 + 3) {
                    const int b = (st.bb0 + st.bb1 + st.bb2 > 1.5) ? 1 : 0;
                    if (lane == 0) frame[st.bitpos] = (uint8_t)b;
                    st.bitpos++;
                    if (st.bitpos >= IMET4_FRAME_BITS) { emit(a, c, st, frame, sc); st.bitpos = 0; st.hf = 0; }
                    st.pos_bit += bitlen;
                }
            } else if (bit != st.bit0) {
                const int pos0 = st.pos;
                st.pos = (int)sc;
                const int len = (int)((st.pos - pos0) / bitlen + 0.5);
                for (int i = 0; i < len; i++) {
                    if (!st.hf && i >= 1) {                    // pushes of one character after the first cannot complete the header
                        const int r = len - i;
                        st.hreg = r >= 32 ? (st.bit0 ? 0xffffffffu : 0u) : ((st.hreg << r) | (st.bit0 ? ((1u << r) - 1u) : 0u));
                        st.hcount = min(st.hcount + r, 64);
                        break;
                    }
                    st.hreg = (st.hreg << 1) | (uint32_t)st.bit0;
                    st.hcount = min(st.hcount + 1, 64);
                    if (!st.hf) {
                        if (st.hcount >= 30 && (st.hreg & 0x3fffffffu) == IMET4_HEADER_PAT) {
                            st.hf = 1;
                            st.bitpos = 10;
                            st.pos_bit = st.pos;
                            if (lane == 0) frame[st.bitpos] = (uint8_t)bit;
                            st.bitpos++;
                            const uint32_t mv = sc + 1;                       // dsp.sample_in
                            const float pf = (float)mv - a.head_sps;         // mv_pos - HEADLEN * sps, in float
                            uint32_t pp = (uint32_t)(long long)pf;
                            if (pp > mv) pp = 0;
                            st.pre_pos = pp;
                            hit = true;
                        }
                    } else {
                        if (lane == 0) frame[st.bitpos] = (uint8_t)st.bit0;
                        st.bitpos++;
                        if (st.bitpos >= IMET4_FRAME_BITS) { emit(a, c, st, frame, sc); st.bitpos = 0; st.hf = 0; }
                    }
                }
                st.bit0 = bit;
            }
            if (hit) { stop = k; break; }
        }

        // ---- commit up to sample s0 + stop
        if (lane <= stop) bufs[s % (uint32_t)a.M] = v;
        st.xsum = rl(my_xs, stop);
        st.F1r = rl(m1r, stop); st.F1i = rl(m1i, stop); st.F2r = rl(m2r, stop); st.F2i = rl(m2i, stop);
        if (a.iq) {
            st.prevr = rl(zr, stop); st.previ = rl(zi, stop);
        }
        if (a.iq && !a.pre) {
            st.sumx = rl(my_sx, stop); st.sumy = rl(my_sy, stop);
            st.cnt += (uint32_t)(stop + 1);
            if (blk && stop == L - 1) {
                st.avgx = (float)(st.sumx / (double)(float)st.maxcnt);
                st.avgy = (float)(st.sumy / (double)(float)st.maxcnt);
                st.sumx = 0; st.sumy = 0; st.cnt = 0;
                if (st.maxcnt < st.maxlim) st.maxcnt *= 2;
            }
        }
        if (upd && stop == L - 1) {
            st.dc = st.xsum / (double)a.M;
            const double dDf = (double)a.sr * st.dc / 1.6;
            st.Df += dDf * 0.5;
            if (a.iq) {
                if (fabs(dDf) > 2e3) { if (st.locked) st.locked = 0; }
                else if (st.locked == 0) st.locked = 1;
            }
        }
        if (st.sample + (uint32_t)(stop + 1) < st.sample) st.sample_hi += 0x100000000ULL;
        st.sample += (uint32_t)(stop + 1);
        done += stop + 1;
        __syncthreads();
    }
    if (lane == 0) a.chan[c] = st;
}

// The decimating front end (decM > 1, f32read_cblock + the LUT mixer + lowpass(decXbuffer, ...) of f32_sample :468-489): per channel one
// wavefront; base-rate samples in tiles of at most 64 (split at the IQ-dc block ends, whose double sums are in-order ladders), mixed and
// written to a base ring by absolute index; then each lane one IF output, the decimator FIR over the ring in the reference's slot order.
template <bool RT> __global__ __launch_bounds__(64) void k_imet4_decim(const Imet4Args a) {
    const int c = blockIdx.x, lane = threadIdx.x;
    if (RT && !a.active[c]) return;
    Imet4Chan st = a.chan[c];
    const unsigned long long bmask = (unsigned long long)a.bring_len - 1;
    float2 *ring = a.bring + (size_t)c * a.bring_len;
    float2 *out = a.ifbuf + (size_t)c * a.if_stride;
    const int D = a.decM;
    const size_t in_stride = RT ? (size_t)a.ch_stride * 2 : (size_t)a.n * D * 2;
    const uint8_t *in8 = (const uint8_t *)a.in + (a.bits == 8 ? in_stride * c : 0);
    const int16_t *in16 = (const int16_t *)a.in + (a.bits == 16 ? in_stride * c : 0);
    const float2 *in32 = (const float2 *)a.in + (RT && a.bits == 32 ? (size_t)a.ch_stride * c : 0);
    for (int t0 = 0; t0 < a.n; t0 += 64) {
        const int nI = min(64, a.n - t0);
        const long long nb = (long long)nI * D;
        for (long long j0 = 0; j0 < nb; ) {
            int L = (int)min(64LL, nb - j0);
            const uint32_t left = st.maxcnt - st.cnt;
            if (left < (uint32_t)L) L = (int)left;
            const bool act = lane < L;
            const unsigned long long b = st.base + (unsigned long long)lane;
            const size_t ix = (size_t)t0 * D + (size_t)j0 + lane;
            float x = 0.f, y = 0.f;
            if (act) {
                if (RT && a.bits == 32) { const float2 z = in32[ix]; x = z.x; y = z.y; }                       // imet4iq.c:329-332
                else if (a.bits == 16) { x = (float)(in16[2 * ix] / 32768.0); y = (float)(in16[2 * ix + 1] / 32768.0); }
                else { x = (float)((in8[2 * ix] - 128) / 128.0); y = (float)((in8[2 * ix + 1] - 128) / 128.0); }
                const float br = x - st.avgx, bi = y - st.avgy;
                double sn, cs;
                sincos((st.f0 * (double)(b % (unsigned long long)st.lut_len)) * kTwoPi, &sn, &cs);
                const float er = (float)cs, ei = (float)sn;
                ring[b & bmask] = make_float2(br * er - bi * ei, br * ei + bi * er);
            }
            double sx = st.sumx, sy = st.sumy;
            for (int k = 0; k < L; k++) { sx = sx + (double)rl(x, k); sy = sy + (double)rl(y, k); }
            st.sumx = sx; st.sumy = sy;
            st.cnt += (uint32_t)L;
            if (st.cnt == st.maxcnt) {
                st.avgx = (float)(st.sumx / (double)(float)st.maxcnt);
                st.avgy = (float)(st.sumy / (double)(float)st.maxcnt);
                st.sumx = 0; st.sumy = 0; st.cnt = 0;
                if (st.maxcnt < st.maxlim) st.maxcnt *= 2;
            }
            st.base += (unsigned long long)L;
            j0 += L;
        }
        __syncthreads();
        if (lane < nI) {
            const unsigned long long s = st.base - (unsigned long long)nb + (unsigned long long)(lane + 1) * D - 1;
            float wr, wi;
            fir_c(ring, s, a.taps_dec, a.ws_dec, bmask, wr, wi);
            out[t0 + lane] = make_float2(wr, wi);
        }
        __syncthreads();
    }
    if (lane == 0) {
        Imet4Chan *o = a.chan + c;
        o->sumx = st.sumx; o->sumy = st.sumy; o->avgx = st.avgx; o->avgy = st.avgy;
        o->cnt = st.cnt; o->maxcnt = st.maxcnt; o->base = st.base;
    }
}

// Channel restart: the channel's record, rings, AFC buffer, IF row and frame bits become what create builds, and the channel is marked active.
// Grid-stride over the longest of the rows; every index is checked against its own row length, so nothing outside channel c is written.
__global__ __launch_bounds__(256) void k_imet4_restart(const Imet4Args a, const int c, const Imet4Chan fresh) {
    const size_t step = (size_t)gridDim.x * blockDim.x;
    const size_t ring = (size_t)a.ring, bring = (size_t)a.bring_len, nif = a.pre ? (size_t)a.if_stride : 1, M = (size_t)a.M;
    float2 *zring = a.zring + (size_t)c * ring, *br = a.bring + (size_t)c * bring, *ifb = a.ifbuf + (size_t)c * nif;
    float *fmring = a.fmring + (size_t)c * ring, *xring = a.xring + (size_t)c * ring, *bufs = a.bufs + (size_t)c * M;
    uint8_t *frame = a.frames + (size_t)c * IMET4_FRAME_STRIDE;
    size_t top = ring > bring ? ring : bring;
    if (nif > top) top = nif;
    if (M > top) top = M;
    if ((size_t)IMET4_FRAME_STRIDE > top) top = IMET4_FRAME_STRIDE;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < top; i += step) {
        if (i < ring) { zring[i] = make_float2(0.f, 0.f); fmring[i] = 0.f; xring[i] = 0.f; }
        if (i < bring) br[i] = make_float2(0.f, 0.f);
        if (i < nif) ifb[i] = make_float2(0.f, 0.f);
        if (i < M) bufs[i] = 0.f;
        if (i < (size_t)IMET4_FRAME_STRIDE) frame[i] = (i == 1 || i == 9) ? 1 : 0;      // bitframe's initial SOH character, imet4iq.c:847
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { a.chan[c] = fresh; a.active[c] = 1; }
}

extern "C" int sonde_launch_imet4_restart(const Imet4Args *a, int c, const Imet4Chan *fresh, hipStream_t s) {
    hipLaunchKernelGGL(k_imet4_restart, dim3(16), dim3(256), 0, s, *a, c, *fresh);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int sonde_launch_imet4(const Imet4Args *a, hipStream_t s) {
    if (a->rt) {
        if (a->pre) hipLaunchKernelGGL(k_imet4_decim<true>, dim3(a->n_ch), dim3(64), 0, s, *a);
        hipLaunchKernelGGL(k_imet4_afsk<true>, dim3(a->n_ch), dim3(64), 0, s, *a);
    } else {
        if (a->pre) hipLaunchKernelGGL(k_imet4_decim<false>, dim3(a->n_ch), dim3(64), 0, s, *a);
        hipLaunchKernelGGL(k_imet4_afsk<false>, dim3(a->n_ch), dim3(64), 0, s, *a);
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
