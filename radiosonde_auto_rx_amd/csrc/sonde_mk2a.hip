// sonde_mk2a.hip — the LMS6-1680 / MkIIa receiver on the device (include/sonde_mk2a.h): the reference's mk2a/mk2a1680mod.c.
//
// k_mk2a_mix  what does not depend on the AFC: IQ-dc removal in blocks (f32read_cblock :643-688), the LUT mixer (:817, :1199-1231) and, with
//             decM > 1, the decimating low-pass (:823-826).  One workgroup per channel; IF samples of the call go to ifbuf.
// k_mk2a      the rest of the chain, one workgroup per channel walking the reference's state machine (main :2370-2430, find_header :1505):
//             search -> correlation window every K-4 output samples counted from the end of the previous frame -> maybe header -> bits
//             until CA CA CA CA or 1760 bits -> search with k = 0.  Df and the IF tap set change only at a window (:1526-1543), so between
//             two windows the front end (f32buf_sample :785-948: AFC rotation with t in double, IF low-pass, discriminator, --IQ tone
//             correlator, FM / IQFM low-pass on every decFM-th sample) is data-parallel: all lanes fill the stretch up to the next window,
//             phase by phase over rings indexed by absolute sample.  Inside a frame Df cannot change, so the front end runs a tile ahead
//             of the slicer; what it computed behind the end of the frame is what the search would have computed.
//             A window is getCorrDFT (:331-480) with the reference's own 8192-point transform (sonde_fft_dev.h) in LDS: X = rdft(xn),
//             with --dc X[0] = 0 and xn replaced by the transform back, Z = X Fm, arg-max of re(cx)^2, norm, the header's dc over the
//             preamble part of fm_buffer, and for --IQ while unlocked the second correlation on fm_buffer.  headcmp, read_softbit2p
//             (one bit per lane) and findsync follow.  Finished frames go to a device queue: hard bits, mv, mv_pos, Df, polarity.
//
// Floating-point contraction is off in this file: the reference is plain C on x86-64 (every product and sum rounded on its own).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <cstdint>
#include "sonde_mk2a_dev.h"
#define FFT_THREADS MK2A_THREADS
#include "sonde_fft_dev.h"
static_assert(SC_N == MK2A_M, "the window transform is the 8192-point one");

namespace {

constexpr double kTwoPi = 6.2831853071795864769252867665590;
constexpr double kPi = 3.1415926535897932384626433832795;
constexpr int NW = MK2A_THREADS / 64;
typedef unsigned long long u64;

// lowpass() / re_lowpass() of the reference: buffer slot n holds the newest sample m <= s with m % T == n, weight ws[T - (s+1) % T + n]
// of the duplicated table; summed over n in slot order.  Samples before the stream start are the zeroed buffer.
__device__ __forceinline__ float2 fir_c(const float2 *ring, u64 s, int T, const float *ws2, u64 mask) {
    const int r = (int)(s % (u64)T), S = T - (int)((s + 1) % (u64)T);
    float ar = 0.f, ai = 0.f;
    for (int n = 0; n < T; n++) {
        const int back = (r - n + T) % T;
        float2 z = make_float2(0.f, 0.f);
        if ((u64)back <= s) z = ring[(s - back) & mask];
        const float w = ws2[S + n];
        ar = ar + z.x * w;
        ai = ai + z.y * w;
    }
    return make_float2(ar, ai);
}
__device__ __forceinline__ float fir_r(const float *ring, u64 s, int T, const float *ws2, u64 mask) {
    const int r = (int)(s % (u64)T), S = T - (int)((s + 1) % (u64)T);
    float a = 0.f;
    for (int n = 0; n < T; n++) {
        const int back = (r - n + T) % T;
        const float x = ((u64)back <= s) ? ring[(s - back) & mask] : 0.f;
        a = a + x * ws2[S + n];
    }
    return a;
}

struct Red {                       // the workgroup's reduction scratch
    double d[2 * NW];
    float f[NW];
    int i[NW];
    int flag;
};

__device__ __forceinline__ double block_sum(double v, double *sm) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0;
    for (int w = 0; w < NW; w++) s += sm[w];
    return s;
}
__device__ __forceinline__ float block_sum(float v, Red &r) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) r.f[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0;
    for (int w = 0; w < NW; w++) s += r.f[w];
    return s;
}
__device__ __forceinline__ int block_min(int v, Red &r) {
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) r.i[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = r.i[0];
    for (int w = 1; w < NW; w++) s = min(s, r.i[w]);
    return s;
}

// one correlation of getCorrDFT on `src` (bufs or fm_buffer) at sample_out = pos.  Returns mp (the peak index), -4 for an edge value or -5 when
// not one value is above zero; mx = re(cx[mp]) / (xnorm N).
__device__ int corr_window(const Mk2aArgs &a, const float *src, float2 *Xg, uint32_t pos, float2 *x, const float2 *tws, Red &red, float &mx_out) {
    const int tid = threadIdx.x, K = a.K, L = a.L, N = MK2A_M, wl = K + L;
    const uint32_t start = pos - (uint32_t)(wl - 1), mask = MK2A_M - 1;
    for (int i = tid; i < N; i += MK2A_THREADS) {
        const float v = i < wl ? src[(start + (uint32_t)i) & mask] : 0.f;
        x[XI(brev13(i))] = make_float2(v, 0.f);
    }
    __syncthreads();
    dft_ref<2>(x, tws, a.tws, tid);                                              // X = rdft(xn) (:355)
    if (a.dc) {                                                                  // X[0] = 0; kept for xn = re(Nidft(X)) / N (:371-373)
        if (tid == 0) x[XI(0)] = make_float2(0.f, 0.f);
        __syncthreads();
        for (int i = tid; i < N; i += MK2A_THREADS) Xg[i] = x[XI(i)];
        __syncthreads();
    }
    // Z = X * Fm (:376); Nidft() transforms conj(Z): conjugate and swap into bit-reversed order for the same network
    const float2 *FmR = a.Fm + N;
    for (int i = tid; i < N; i += MK2A_THREADS) {
        const int r = brev13(i);
        if (r < i) continue;
        const float2 zi = cmul(x[XI(i)], a.Fm[i]), zr = cmul(x[XI(r)], FmR[i]);
        x[XI(r)] = make_float2(zi.x, -zi.y);
        x[XI(i)] = make_float2(zr.x, -zr.y);
    }
    __syncthreads();
    dft_ref<2>(x, tws, a.tws, tid);                                              // cx = Nidft(Z)
    // arg-max of re(cx)^2 over [L-1, K+L), the first maximum wins (:386-394)
    float best = 0.f, bestc = 0.f; int bidx = -1;
    for (int i = tid; i < wl; i += MK2A_THREADS) {
        if (i < L - 1) continue;
        const float c = x[XI(i)].x, c2 = c * c;
        if (c2 > best) { best = c2; bidx = i; bestc = c; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off), oc = __shfl_xor(bestc, off); const int oi = __shfl_xor(bidx, off);
        if (oi >= 0 && (ob > best || (ob == best && (bidx < 0 || oi < bidx)))) { best = ob; bidx = oi; bestc = oc; }
    }
    __syncthreads();
    if ((tid & 63) == 0) { red.f[tid >> 6] = best; red.i[tid >> 6] = bidx; red.d[tid >> 6] = (double)bestc; }
    __syncthreads();
    int mp = -1; float mx = 0.f;
    {
        float b = 0.f;
        for (int w = 0; w < NW; w++) {
            const float ob = red.f[w]; const int oi = red.i[w];
            if (oi >= 0 && (ob > b || (ob == b && (mp < 0 || oi < mp)))) { b = ob; mp = oi; mx = (float)red.d[w]; }
        }
    }
    __syncthreads();
    if (mp < 0) { mx_out = 0.f; return -5; }
    if (mp == L - 1 || mp == wl - 1) { mx_out = 0.f; return -4; }                // edge value (:395)
    // xnorm over xn[mp - i], i < L (:400-402)
    float e = 0.f;
    if (a.dc) {
        for (int i = tid; i < N; i += MK2A_THREADS) { const float2 v = Xg[i]; x[XI(brev13(i))] = make_float2(v.x, -v.y); }
        __syncthreads();
        dft_ref<2>(x, tws, a.tws, tid);
        for (int k = tid; k < L; k += MK2A_THREADS) { const float v = x[XI(mp - k)].x / (float)N; e += v * v; }
    } else {
        for (int k = tid; k < L; k += MK2A_THREADS) { const int i = mp - k; const float v = i < wl ? src[(start + (uint32_t)i) & mask] : 0.f; e += v * v; }
    }
    const float xnorm = sqrtf(block_sum(e, red));
    mx_out = mx / (xnorm * (float)N);
    return mp;
}

__constant__ uint8_t kHdr[MK2A_HDRLEN] = {0,0,1,0,1,0,0,1,1,1, 0,0,1,0,1,0,0,1,1,1, 0,0,1,0,1,0,0,1,1,1, 0,0,0,1,0,0,1,0,0,1, 0,0,1,0,0,1,0,1,0,1};   // CA CA CA 24 52 in 8N1

__device__ __forceinline__ uint32_t sc_end(int b, float sps) {                  // consumed-sample count behind bit b (read_softbit2p :1031-1094)
    const double bg = (b == 0 ? 0.0 : (double)((float)b * sps)) + (double)sps;
    return (uint32_t)ceil(bg);
}

}  // namespace

__global__ __launch_bounds__(MK2A_THREADS) void k_mk2a(const Mk2aArgs a) {
    extern __shared__ __attribute__((aligned(16))) float2 smem_mk[];
    float2 *x = smem_mk;                          // [SC_XN] padded (XI)
    float2 *tws = smem_mk + SC_XN;                // [SC_TW_LDS + 1] twiddles of stages 0..8
    __shared__ Red red;
    const int c = blockIdx.x, tid = threadIdx.x;
    Mk2aChan st = a.chan[c];
    const u64 rm = (u64)a.ring - 1;
    const uint32_t mm = MK2A_M - 1;
    float2 *zrot = a.zrot + (size_t)c * a.ring, *zlp = a.zlp + (size_t)c * a.ring;
    float *fmr = a.fmr + (size_t)c * a.ring, *sraw = a.sraw + (size_t)c * a.ring;
    float *bufs = a.bufs + (size_t)c * MK2A_M, *fmbuf = a.fmbuf + (size_t)c * MK2A_M;
    float2 *Xg = a.Xg + (size_t)c * MK2A_M;
    const float2 *ifin = a.ifbuf + (size_t)c * a.if_stride;
    uint8_t *frame = a.frames + (size_t)c * MK2A_FRAME_STRIDE;
    for (int k = tid; k < SC_TW_LDS; k += MK2A_THREADS) tws[k] = a.tws[k];
    __syncthreads();
    const u64 U0 = st.U, Uend = st.U + (u64)a.n_if;
    const int d = a.decFM;
    const bool iq5 = a.opt_iq == 5;
    const double dcbit = (a.dc && !iq5) ? 1.0 : 0.0;        // read_bufbit / read_softbit2p subtract dsp->dc only for --iq (:960, :1038)

    // the front end over IF samples [st.U, U1)
    auto produce = [&](u64 U1) {
        while (st.U < U1) {
            const u64 Ua = st.U, Ub = min(U1, Ua + (u64)MK2A_TILE);
            for (u64 u = Ua + tid; u < Ub; u += MK2A_THREADS) {
                float2 z = ifin[u - U0];
                if (a.dc) {                                                        // z *= cexp(-t 2 pi Df i), t in double (:803, :830-832)
                    const double t = (uint32_t)u / (double)a.sr;
                    double sn, cs;
                    sincos(((-t) * kTwoPi) * st.Df, &sn, &cs);
                    const double dr = (double)z.x, di = (double)z.y;
                    z = make_float2((float)(dr * cs - di * sn), (float)(dr * sn + di * cs));
                }
                zrot[u & rm] = z;
            }
            __syncthreads();
            if (a.lp & MK2A_LP_IQ) {
                const float *ws2 = (a.dc && !st.locked) ? a.ws_iq0 : a.ws_iq1;
                for (u64 u = Ua + tid; u < Ub; u += MK2A_THREADS) zlp[u & rm] = fir_c(zrot, u, a.taps_iq, ws2, rm);
            } else {
                for (u64 u = Ua + tid; u < Ub; u += MK2A_THREADS) zlp[u & rm] = zrot[u & rm];
            }
            __syncthreads();
            for (u64 u = Ua + tid; u < Ub; u += MK2A_THREADS) {
                const float2 z = zlp[u & rm];
                const float2 z0 = u ? zlp[(u - 1) & rm] : make_float2(0.f, 0.f);
                // w = z * conj(z0): conj() is the double function, so the reference forms the product in double (the float products are
                // exact there) and rounds each part once to float (:842-844); float products rounded one by one flip the sign of a
                // cancelling imaginary part, and with it the discriminator from -0.8 to +0.8
                const float wr = (float)((double)z.x * (double)z0.x + (double)z.y * (double)z0.y);
                const float wi = (float)((double)z.y * (double)z0.x - (double)z.x * (double)z0.y);
                fmr[u & rm] = (float)(0.8 * atan2((double)wi, (double)wr) / kPi);
                if (iq5) {                                                          // tone correlator over the middle of the bit (:881-907)
                    float x1r = 0.f, x1i = 0.f, x2r = 0.f, x2i = 0.f;
                    for (int j = 0; j < a.n_tone; j++) {
                        const Mk2aTone tn = a.tone[j];
                        const float2 zz = (u64)tn.n <= u ? zlp[(u - tn.n) & rm] : make_float2(0.f, 0.f);
                        const double zr = zz.x, zi = zz.y;
                        x1r = (float)((double)x1r + (zr * tn.e1r - zi * tn.e1i)); x1i = (float)((double)x1i + (zr * tn.e1i + zi * tn.e1r));
                        x2r = (float)((double)x2r + (zr * tn.e2r - zi * tn.e2i)); x2i = (float)((double)x2i + (zr * tn.e2i + zi * tn.e2r));
                    }
                    const double xbit = hypot((double)x2r, (double)x2i) - hypot((double)x1r, (double)x1i);
                    sraw[u & rm] = (float)(xbit / (double)a.tone_sps);
                }
            }
            __syncthreads();
            // output samples whose last IF sample n d + d - 1 lies in [Ua, Ub)
            const u64 na = Ua / (u64)d, nb = Ub / (u64)d;
            for (u64 n = na + tid; n < nb; n += MK2A_THREADS) {
                const u64 ul = n * (u64)d + (u64)d - 1;
                const float sfm = (a.lp & MK2A_LP_FM) ? fir_r(fmr, ul, a.taps_fm, a.ws_fm, rm) : fmr[ul & rm];
                float s = sfm;
                if (iq5) s = (a.lp & MK2A_LP_IQFM) ? fir_r(sraw, ul, a.taps_iqfm, a.ws_iqfm, rm) : sraw[ul & rm];
                bufs[(uint32_t)n & mm] = s;
                fmbuf[(uint32_t)n & mm] = sfm;
            }
            __syncthreads();
            st.U = Ub;
            st.N = Ub / (u64)d;
        }
    };

    for (;;) {
        if (st.mode == 0) {
            // ---- find_header: the next window is evaluated when k reaches K-4
            const u64 nw = st.n_start + (u64)(a.K - 4);
            produce(min(Uend, nw * (u64)d));
            if (st.N < nw) break;
            st.n_start = nw;
            const uint32_t pos = (uint32_t)(nw - 1) - (uint32_t)a.delay;          // sample_out
            const uint32_t mvpos0 = st.mv_pos;
            float mv = 0.f, mv2 = 0.f; uint32_t mv2_pos = 0;
            st.dc = 0.0;
            bool full = false;                                                    // getCorrDFT ran to its end (dDf set)
            uint32_t mpos = 0;
            if (pos >= (uint32_t)a.L) {
                float mx;
                int mp = corr_window(a, bufs, Xg, pos, x, tws, red, mx);
                if (mp != -4) {
                    mpos = mp == -5 ? pos - (uint32_t)(a.K + a.L - 1) - 1u : pos - (uint32_t)(a.K + a.L - 1) + (uint32_t)mp;
                    mv = mx; st.mv_pos = mpos;
                    st.buffered0 = (int32_t)(pos - mpos);
                    full = true;
                    if (a.dc && iq5 && !st.locked) {                              // second correlation on fm_buffer (:415-454)
                        __syncthreads();
                        mp = corr_window(a, fmbuf, Xg, pos, x, tws, red, mx);
                        if (mp == -4) full = false;
                        else { mpos = mp == -5 ? pos - (uint32_t)(a.K + a.L - 1) - 1u : pos - (uint32_t)(a.K + a.L - 1) + (uint32_t)mp; mv2 = mx; mv2_pos = mpos; }
                    }
                }
            }
            if (full) {
                double dc = 0.0;
                if (a.dc) {                                                       // header dc over the preamble part 2L/5 .. L (:460-471)
                    const int ofs = (iq5 && mv2_pos == 0) ? a.mp_ofs : 0;
                    double p = 0.0;
                    for (int i = 2 * a.L / 5 + tid; i < a.L; i += MK2A_THREADS) p += (double)fmbuf[((uint32_t)ofs + mpos - (uint32_t)i) & mm];
                    dc = block_sum(p, red.d) / ((float)a.L * 3 / 5.0);
                }
                st.dc = dc;
                st.dDf = a.sr * dc / (2.0 * 0.8);
            }
            st.mv = mv;
            bool found = false;
            if (mv > a.thres || mv < -a.thres || mv2 > a.thres || mv2 < -a.thres) {
                if (a.dc) {
                    st.Df += st.dDf * 0.5;
                    if (fabs(st.dDf) > 20 * 1e3) st.locked = 0; else st.locked = 1;
                }
                if (st.mv_pos > mvpos0) {                                         // headcmp (:992-1015), one header bit per lane
                    int err = 0;
                    if (tid < MK2A_HDRLEN) {
                        double g = (double)((float)tid * a.sps);
                        uint32_t rc = (uint32_t)ceil(g);
                        g += a.sps;
                        const uint32_t mvp = st.mv_pos + 1u - (uint32_t)a.L;
                        double sum = 0.0;
                        do { sum += (double)bufs[(rc + mvp) & mm] - st.dc * dcbit; rc++; } while (rc < g);
                        const int bit = sum >= 0 ? 1 : 0;
                        err = (bit ^ (mv < 0 ? 1 : 0)) != kHdr[tid];
                    }
                    const int herrs = __syncthreads_count(err);
                    found = herrs <= 1;
                }
            }
            if (found) {
                if ((double)mv * (0.5 - st.inv) < 0) { st.inv ^= 1; }             // wrong polarity: dropped, the option flips (:2383-2386)
                else { st.mode = 1; st.bitpos = 0; st.n_hdr = nw; }
            }
        } else {
            // ---- frame: bits whose samples exist, one per lane (read_softbit2p), then findsync
            const uint32_t first = st.mv_pos + 1u + (uint32_t)a.bitofs;
            bool ended = false;
            for (;;) {
                const int b = st.bitpos + tid;
                const uint32_t q1 = sc_end(b, a.sps);
                const long long need = (long long)st.n_hdr + max(0LL, (long long)q1 - (long long)st.buffered0);
                const bool can = tid < a.slice_cap && b < MK2A_MAX_BITS - MK2A_FRMSTART && need <= (long long)st.N;
                const int nbits = __syncthreads_count(can);
                if (nbits == 0) break;
                if (can) {
                    const double bg = b == 0 ? 0.0 : (double)((float)b * a.sps);
                    const double mid = bg + (a.sps - 1) / 2.0;
                    const uint32_t q0 = b == 0 ? 0u : sc_end(b - 1, a.sps);
                    double sum = 0.0;
                    for (uint32_t q = q0; q < q1; q++) {
                        float smp = bufs[(first + q) & mm];
                        smp = (float)((double)smp - st.dc * dcbit);
                        if (a.bl < 0 || (mid - a.bl < q && q < mid + a.bl)) sum += smp;
                    }
                    frame[MK2A_FRMSTART + b] = (uint8_t)((sum >= 0 ? 1 : 0) ^ st.inv);
                }
                __syncthreads();
                // the loop of main ends at the first pos with findsync(pos) or pos = 1760 (:2394)
                int endpos = 1 << 30;
                if (tid < nbits) {
                    const int pos = MK2A_FRMSTART + st.bitpos + tid + 1;
                    bool sync = pos >= 40;
                    for (int i = 0; sync && i < 40; i++) sync = frame[pos - 40 + i] == kHdr[i % 10];
                    if (sync || pos >= MK2A_MAX_BITS) endpos = pos;
                }
                endpos = block_min(endpos, red);
                if (endpos < (1 << 30)) {
                    const uint32_t Q = sc_end(endpos - MK2A_FRMSTART - 1, a.sps);
                    const u64 n_after = st.n_hdr + (u64)max(0LL, (long long)Q - (long long)st.buffered0);
                    if (tid == 0) red.flag = atomicAdd(a.q_count, 1);
                    __syncthreads();
                    const int qi = red.flag;
                    if (qi < a.q_cap) {
                        Mk2aFrame *f = a.q + qi;
                        for (int i = tid; i < endpos; i += MK2A_THREADS) f->bits[i] = frame[i];
                        if (tid == 0) { f->channel = c; f->nbits = endpos; f->inv = st.inv; f->mv = st.mv; f->Df = st.Df; f->mv_pos = st.mv_pos; f->sample = n_after; }
                    }
                    __syncthreads();
                    st.mode = 0; st.n_start = n_after; st.bitpos = 0;
                    ended = true;
                    break;
                }
                st.bitpos += nbits;
            }
            if (!ended) {
                if (st.U >= Uend) break;
                produce(min(Uend, st.U + (u64)MK2A_TILE));
            }
        }
    }
    if (tid == 0) {
        Mk2aChan *o = a.chan + c;
        o->Df = st.Df; o->dDf = st.dDf; o->dc = st.dc; o->U = st.U; o->N = st.N; o->n_start = st.n_start; o->n_hdr = st.n_hdr;
        o->mv = st.mv; o->mv_pos = st.mv_pos; o->locked = st.locked; o->mode = st.mode; o->inv = st.inv; o->buffered0 = st.buffered0; o->bitpos = st.bitpos;
    }
}

// IQ-dc removal, LUT mixer and decimator.  The IQ-dc sums are sums of multiples of 2^-15 (2^-7), far fewer than 2^37 of them: exact in
// double in any order, so the workgroup adds them as a tree.
__global__ __launch_bounds__(MK2A_THREADS) void k_mk2a_mix(const Mk2aArgs a) {
    __shared__ double sm[2 * NW];
    const int c = blockIdx.x, tid = threadIdx.x;
    Mk2aChan *o = a.chan + c;
    double sumx = o->sumx, sumy = o->sumy; float avgx = o->avgx, avgy = o->avgy;
    uint32_t cnt = o->cnt, maxcnt = o->maxcnt; const uint32_t maxlim = o->maxlim;
    u64 base = o->base; const double f0 = o->f0; const u64 lut = (u64)o->lut_len;
    const int D = a.decM;
    const u64 bmask = (u64)a.bring_len - 1;
    float2 *ring = a.bring + (size_t)c * a.bring_len;
    float2 *out = a.ifbuf + (size_t)c * a.if_stride;
    const size_t in_stride = (size_t)a.n_base * 2;
    const uint8_t *in8 = (const uint8_t *)a.in + (a.bits == 8 ? in_stride * c : 0);
    const int16_t *in16 = (const int16_t *)a.in + (a.bits == 16 ? in_stride * c : 0);
    const int G = D > 1 ? 256 : MK2A_THREADS;                   // IF outputs per group
    for (int t0 = 0; t0 < a.n_if; t0 += G) {
        const int nI = min(G, a.n_if - t0);
        const long long nb = (long long)nI * D;
        for (long long j0 = 0; j0 < nb; ) {
            int Ln = (int)min((long long)MK2A_THREADS, nb - j0);
            const uint32_t left = maxcnt - cnt;
            if (left < (uint32_t)Ln) Ln = (int)left;
            const bool act = tid < Ln;
            const u64 b = base + (u64)tid;
            const size_t ix = (size_t)t0 * D + (size_t)j0 + tid;
            float xv = 0.f, yv = 0.f;
            if (act) {
                if (a.bits == 16) { xv = (float)(in16[2 * ix] / 32768.0); yv = (float)(in16[2 * ix + 1] / 32768.0); }
                else { xv = (float)((in8[2 * ix] - 128) / 128.0); yv = (float)((in8[2 * ix + 1] - 128) / 128.0); }
                const float br = xv - avgx, bi = yv - avgy;
                double sn, cs;
                sincos((f0 * (double)(b % lut)) * kTwoPi, &sn, &cs);
                const float er = (float)cs, ei = (float)sn;
                const float2 z = make_float2(br * er - bi * ei, br * ei + bi * er);
                if (D > 1) ring[b & bmask] = z; else out[t0 + (int)j0 + tid] = z;
            }
            sumx += block_sum((double)xv, sm);
            sumy += block_sum((double)yv, sm + NW);
            cnt += (uint32_t)Ln;
            if (cnt == maxcnt) {
                avgx = (float)(sumx / (double)(float)maxcnt);
                avgy = (float)(sumy / (double)(float)maxcnt);
                sumx = 0; sumy = 0; cnt = 0;
                if (maxcnt < maxlim) maxcnt *= 2;
            }
            base += (u64)Ln;
            j0 += Ln;
        }
        __syncthreads();
        if (D > 1 && tid < nI) {
            const u64 s = base - (u64)nb + (u64)(tid + 1) * D - 1;
            out[t0 + tid] = fir_c(ring, s, a.taps_dec, a.ws_dec, bmask);
        }
        __syncthreads();
    }
    if (tid == 0) { o->sumx = sumx; o->sumy = sumy; o->avgx = avgx; o->avgy = avgy; o->cnt = cnt; o->maxcnt = maxcnt; o->base = base; }
}

extern "C" int sonde_launch_mk2a(const Mk2aArgs *a, hipStream_t s) {
    const size_t lds = (size_t)(SC_XN + SC_TW_LDS + 1) * sizeof(float2);
    static int attr_dev = -1;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -2;
    if (attr_dev != dev) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_mk2a), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -2;
        attr_dev = dev;
    }
    hipLaunchKernelGGL(k_mk2a_mix, dim3(a->n_ch), dim3(MK2A_THREADS), 0, s, *a);
    hipLaunchKernelGGL(k_mk2a, dim3(a->n_ch), dim3(MK2A_THREADS), lds, s, *a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
