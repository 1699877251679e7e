// sonde_fm_front_dev.h — iq_dec's chain at decM = 1 on float32 IQ, one wavefront per channel, every channel on a sample clock of its own:
// `iq_dec --FM --lpFM --iq fq - <sr> 32` where iq_dec does not decimate.  Behaviour reproduced (not code), per sample and in the reference's
// order of operations (demod/mod/iq_dec.c):
//   f32read_cblock :337-382  x - avg in float; the sums in double, in reading order; avg = sum / (float)maxcnt when cnt == maxcnt; maxcnt from sr / 32,
//                            doubled up to sr (:752-758)
//   if_fm :571-573           z * ex[n % lut_len], ex[n] = cexp(2 pi i f0 n) with f0 n kept in double (:704-707): evaluated per sample as the other kernels do
//                            (the fraction of f0 n in double, rounded to float, into the hardware's sine and cosine of revolutions)
//   if_fm :593-596           w = z * conj(z0) formed in double (conj() is the double function) and rounded once, s = (float)(gain * carg(w) / pi), gain the float 0.8
//   if_fm :599-604           lpFM_buf[n % taps] = s; re_lowpass(lpFM_buf, n + 1, taps, ws): a float sum over the buffer in slot order
// A channel's clock (sample count, IQ-dc block, table index, filter slot) lives in its FmFrontChan and starts at its restart, so a segment edge falls anywhere
// inside a call: the wave walks the call in tiles of at most 64 samples (one per lane) and ends a tile at the end of the IQ-dc block in progress.  The
// unfiltered FM samples of the last `rring` samples are a ring by the channel's own sample count, in LDS during a call and in device memory between calls, so
// any cutting of a stream into calls gives the same samples, calls shorter than the tap count included.  The low-passed sample i of the call goes to
// fm[(first + i) & fmask]: the ring k_drop_slice reads (DROP_IN_RING).
//
// Compiled twice, like the soft-bit consumers: by hipcc into k_fm_front (sonde_fm_front.hip, floating-point contraction off) and by g++ under
// tests/emu/wave_emu.h (tests/emu/fm_front_emu.cpp, -ffp-contract=off).  Control flow around every rsw_* call is wave-uniform.
#ifndef SONDE_FM_FRONT_DEV_H
#define SONDE_FM_FRONT_DEV_H
#include <stdint.h>
#include <math.h>

#define FMF_RING_MAX 1024                                             // floats of the unfiltered ring in LDS: taps + 128 <= it
#define FMF_TAPS_MAX 448                                              // the duplicated tap table (2 taps + 1) fits FMF_RING_MAX floats

struct alignas(8) FmfIQ { float x, y; };

// a channel between calls
struct FmFrontChan {
    double sumx, sumy;                 // IQdc.sumIQx / sumIQy
    double f0;                         // the snapped mixer frequency, cycles per sample (design_mixer)
    unsigned long long count;          // samples since the restart
    uint32_t cnt, maxcnt, maxlim;      // IQdc.cnt / maxcnt / maxlim
    uint32_t lut_len, lut_pos;         // the table's period; count % lut_len
    uint32_t fir_pos;                  // count % taps
    float avgx, avgy;                  // IQdc.avgIQx / avgIQy
    float z0r, z0i;                    // if_fm's z0
    uint32_t pad[2];
};
static_assert(sizeof(FmFrontChan) == 80, "the record lives in device memory between calls and is a kernel argument of the restart");

struct FmFrontArgs {
    FmFrontChan *chan;
    const FmfIQ *in;                   // channel c's row at c * ch_stride samples
    long long ch_stride;
    float *fm;                         // [n_ch][ring]: the low-passed FM samples
    float *raw;                        // [n_ch][rring]: the unfiltered FM samples by the channel's own sample count
    const float *ws2;                  // the taps twice in a row (dup_taps)
    int *active;                       // 0: the channel's workgroup returns before it reads anything
    uint32_t first;                    // sample i of the call goes to fm[(first + i) & (ring - 1)]
    int n_ch, n, taps, ring, rring;
};

struct FmFrontLds {
    float hist[FMF_RING_MAX];
    float w[FMF_RING_MAX];
    float xs[64], ys[64], zr[64], zi[64];
};

// The device body: only for the file that instantiates the kernel (sonde_fm_front.hip defines SONDE_FM_FRONT_BODY, under contract(off)) and for the
// emulator.  The host engines and the slicer's translation unit (sonde_drop_dev.h) read the records above only.
#if defined(SONDE_FM_FRONT_BODY) || defined(SONDE_RS_EMU)
#include "sonde_rs_dev.h"                                             // the rsw_* primitives
#ifndef SONDE_RS_EMU
static RSW_DEV float fmf_cos_rev(float fr) { return __builtin_amdgcn_cosf(fr); }
static RSW_DEV float fmf_sin_rev(float fr) { return __builtin_amdgcn_sinf(fr); }
static RSW_DEV double fmf_fract(double v) { return __builtin_amdgcn_fract(v); }
#else
static inline float fmf_cos_rev(float fr) { return (float)cos(6.2831853071795864769252867665590 * (double)fr); }
static inline float fmf_sin_rev(float fr) { return (float)sin(6.2831853071795864769252867665590 * (double)fr); }
static inline double fmf_fract(double v) { return v - floor(v); }
#endif

// One channel, one call: n samples at `in`.  raw_row has rring floats (a power of two, taps + 128 <= rring <= FMF_RING_MAX), ws2 2 * taps + 1.
static RSW_DEV void fm_front_channel(FmFrontChan *stp, const FmfIQ *in, const int n, float *fm_row, const uint32_t first, const uint32_t fmask,
                                     float *raw_row, const int rring, const float *ws2, const int taps, FmFrontLds *L, const int lane) {
    FmFrontChan st = *stp;
    const uint32_t rmask = (uint32_t)rring - 1;
    for (int j = lane; j < rring; j += 64) L->hist[j] = raw_row[j];
    for (int j = lane; j < 2 * taps + 1; j += 64) L->w[j] = ws2[j];
    rsw_syncthreads();
    int done = 0;
    while (done < n) {
        int Lt = n - done < 64 ? n - done : 64;
        const uint32_t left = st.maxcnt - st.cnt;                      // the tile ends with the IQ-dc block in progress
        if (left < (uint32_t)Lt) Lt = (int)left;
        const bool act = lane < Lt;
        float x = 0.f, y = 0.f;
        if (act) { const FmfIQ v = in[(size_t)done + lane]; x = v.x; y = v.y; }
        const float br = x - st.avgx, bi = y - st.avgy;
        const uint32_t k = (st.lut_pos + (uint32_t)lane) % st.lut_len;
        const float fr = (float)fmf_fract(st.f0 * (double)k);
        const float er = fmf_cos_rev(fr), ei = fmf_sin_rev(fr);
        const float zr = br * er - bi * ei, zi = br * ei + bi * er;
        L->xs[lane] = x; L->ys[lane] = y; L->zr[lane] = zr; L->zi[lane] = zi;
        rsw_syncthreads();
        const float pr = lane ? L->zr[lane ? lane - 1 : 0] : st.z0r, pi_ = lane ? L->zi[lane ? lane - 1 : 0] : st.z0i;
        const float wr = (float)((double)zr * (double)pr + (double)zi * (double)pi_);
        const float wi = (float)((double)zi * (double)pr - (double)zr * (double)pi_);
        const float v = (float)(((double)0.8f * atan2((double)wi, (double)wr)) / 3.1415926535897932384626433832795);
        const uint32_t s = (uint32_t)st.count + (uint32_t)lane;       // the rings are powers of two: the low bits of the count index them
        if (act) L->hist[s & rmask] = v;
        rsw_syncthreads();
        if (act) {
            // re_lowpass: slot m holds the newest sample <= s whose count is m modulo taps, weight ws[taps - (s + 1) % taps + m]; samples before the restart are 0
            const int r = (int)((st.fir_pos + (uint32_t)lane) % (uint32_t)taps), S = taps - (r + 1) % taps;
            const unsigned long long sc = st.count + (unsigned long long)lane;
            float acc = 0.f;
            for (int m = 0; m < taps; m++) {
                const int back = r - m < 0 ? r - m + taps : r - m;
                const float h = (unsigned long long)back <= sc ? L->hist[(s - (uint32_t)back) & rmask] : 0.f;
                acc = acc + h * L->w[S + m];
            }
            fm_row[(first + (uint32_t)done + (uint32_t)lane) & fmask] = acc;
        }
        double sx = st.sumx, sy = st.sumy;                             // the reference's sums, in reading order (the same on every lane)
        for (int j = 0; j < Lt; j++) { sx = sx + (double)L->xs[j]; sy = sy + (double)L->ys[j]; }
        st.sumx = sx; st.sumy = sy;
        st.cnt += (uint32_t)Lt;
        if (st.cnt == st.maxcnt) {
            st.avgx = (float)(st.sumx / (double)(float)st.maxcnt);
            st.avgy = (float)(st.sumy / (double)(float)st.maxcnt);
            st.sumx = 0; st.sumy = 0; st.cnt = 0;
            if (st.maxcnt < st.maxlim) st.maxcnt *= 2;
        }
        st.z0r = L->zr[Lt - 1]; st.z0i = L->zi[Lt - 1];
        st.count += (unsigned long long)Lt;
        st.lut_pos = (st.lut_pos + (uint32_t)Lt) % st.lut_len;
        st.fir_pos = (st.fir_pos + (uint32_t)Lt) % (uint32_t)taps;
        done += Lt;
        rsw_syncthreads();
    }
    for (int j = lane; j < rring; j += 64) raw_row[j] = L->hist[j];
    if (lane == 0) *stp = st;
}
#endif
#endif
