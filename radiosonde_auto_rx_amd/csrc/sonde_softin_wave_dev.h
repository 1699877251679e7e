// sonde_softin_wave_dev.h — what every soft-bit consumer that runs ONE wavefront per channel shares (k_softin_m10 in sonde_softin_dev.hip, sonde_softin_mxx_dev.h,
// sonde_softin_rs92_dev.h, sonde_softin_imet54_dev.h, sonde_softin_meisei_dev.h — and whatever consumer comes next): the primitives sonde_rs_dev.h does not have, the
// call's soft decisions staged in LDS, the header score of find_softbinhead / corr_softhdb (demod_mod.c:1692-1762) in its float-first form, the ring refresh, the
// slot of a completed record, 8N1 characters and the XOR over the wave.  The search LOOPS stay with the consumers: what a hit does to the ring, the polarity and
// the hits behind it differs from decoder to decoder.
//
// Compiled twice, like sonde_rs_dev.h: by hipcc into the k_softin_* kernels and by g++ under tests/emu/wave_emu.h.  Control flow around every cross-lane primitive
// is wave-uniform.
#ifndef SONDE_SOFTIN_WAVE_DEV_H
#define SONDE_SOFTIN_WAVE_DEV_H
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "sonde_rs_dev.h"
#include "../../include/sonde_hip.h"                                    // (SONDE_E_*, the frame records: what every consumer's callers use)
// (no contraction: the reference is plain C on x86-64 — every product and sum rounded on its own)
#pragma clang fp contract(off)

// ---- the primitives sonde_rs_dev.h does not have: a float from a wave-uniform lane, the reciprocal square root of the float score, the counter of a launch
static RSW_DEV float mxxw_bcast_f(float v, int src) { int u; memcpy(&u, &v, 4); u = rsw_bcast(u, src); memcpy(&v, &u, 4); return v; }
#ifndef SONDE_RS_EMU
static RSW_DEV float mxxw_rsq(float v) { return __builtin_amdgcn_rsqf(v); }
static RSW_DEV unsigned mxxw_atomic_inc(unsigned *p) { return atomicAdd(p, 1u); }
#else
static inline float mxxw_rsq(float v) { return 1.0f / sqrtf(v); }
static inline unsigned mxxw_atomic_inc(unsigned *p) { return (*p)++; }
#endif

#define M10_STAGE_MAX 12288                     // soft decisions of a call a staged consumer keeps in LDS (48 KB); longer calls read them from global memory

// ---- the call's soft decisions: X(p) = symbol p of this call with --softinv applied, from LDS where the call fits into the stage_cap symbols of s_x
struct SoftinX {
    const float *s_x, *x; float sgn; bool staged;
    RSW_DEV float operator()(const int p) const { return staged ? s_x[p] : sgn * x[p]; }
};
// (the caller's rsw_wave_sync() behind its own LDS loads covers the staged symbols as well)
static RSW_DEV SoftinX softin_wave_stage(float *s_x, const float *x, const float sgn, const int nb, const int stage_cap, const int lane) {
    const SoftinX X{s_x, x, sgn, nb <= stage_cap};
    if (X.staged) for (int i = lane; i < nb; i += 64) s_x[i] = sgn * x[i];
    return X;
}

// ---- the header search of a +-1 header of HL <= 64 symbols over W(k) = element k of ring ++ the call's symbols from where the search began
// score of the window W(k0) .. W(k0 + HL - 1) against the header hbits (symbol i in bit i): float first, the reference's double form where that is not safely below ths
template <int HL, class WF>
static RSW_DEV float softin_wave_score(const WF &W, const int k0, const unsigned long long hbits, const float ths) {
    float fs = 0.f, fn = 0.f;
    for (int i = 0; i < HL; i++) {
        const float v = W(k0 + i);
        fs += ((hbits >> i) & 1ull) ? v : -v;
        fn = fmaf(v, v, fn);
    }
    float mv = fs * mxxw_rsq(fn * (float)HL);
    if (!(fabsf(mv) < ths - 1e-3f)) {                                 // (also NaN: an all-zero window is the reference's 0 / 0)
        double sum = 0.0, normx = 0.0;
        for (int i = 0; i < HL; i++) {
            const float v = W(k0 + i);
            const float y = ((hbits >> i) & 1ull) ? 1.f : -1.f;
            sum += (double)(y * v);
            normx += (double)(v * v);
        }
        sum /= sqrt(normx * (double)HL);
        mv = (float)sum;
    }
    return mv;
}
// the ring becomes W(k0) .. W(k0 + HL - 1): the HL elements up to a hit at position q of the search (k0 = q + 1) or up to the call's last symbol
template <int HL, class WF>
static RSW_DEV void softin_wave_ring(float *hist, const WF &W, const int k0, const int lane) {
    const float v = W(k0 + (lane < HL ? lane : 0));
    rsw_wave_sync();
    if (lane < HL) hist[lane] = v;
    rsw_wave_sync();
}

// the slot of a completed record: one count per record, the same value on every lane (a slot at or beyond the launch's capacity is counted, not written)
static RSW_DEV unsigned softin_wave_slot(unsigned *count, const int lane) {
    unsigned slot = 0;
    if (lane == 0) slot = mxxw_atomic_inc(count);
    return (unsigned)rsw_bcast((int)slot, 0);
}

// nchars 8N1 characters from the symbols S(0), S(1), .. on a lane per character: bit = (s >= 0) ^ inv, data bit k (symbol 1 + k of the character) in bit k
template <class SF>
static RSW_DEV void softin_wave_8n1(const SF &S, const int nchars, const int inv, uint8_t *out, const int lane) {
    for (int j = lane; j < nchars; j += 64) {
        unsigned byte = 0;
        for (int k = 0; k < 8; k++) {
            const int bit = (S(10 * j + 1 + k) >= 0.0f ? 1 : 0) ^ inv;
            byte |= (unsigned)bit << k;
        }
        out[j] = (uint8_t)byte;
    }
}
// XOR of v over the 64 lanes, on every lane
static RSW_DEV uint32_t softin_wave_xor(uint32_t v, const int lane) {
    for (int d = 1; d < 64; d <<= 1) v ^= (uint32_t)rsw_shfl_up((int)v, d, lane);
    return (uint32_t)rsw_bcast((int)v, 63);
}
#endif
