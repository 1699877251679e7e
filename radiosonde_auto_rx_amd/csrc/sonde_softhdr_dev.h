// sonde_softhdr_dev.h — find_softbinhead / corr_softhdb (demod/mod/demod_mod.c:1692-1762) for a 64-symbol header, the part the soft-bit consumers of
// sonde_softin_dev.hip share (RS41, LMS6): the normalised correlation of the last 64 soft bits with the +-1 header, decided the reference's way — float
// products, double sums, in order — on a lane per stream position.  The window of call position q is taken from `hist` (the 64 soft bits seen before
// position cur of the call, oldest first: hdb.sbuf) followed by sgn * x[cur ..].  Compiled by hipcc and, under tests/emu/wave_emu.h, by g++.
#ifndef SONDE_SOFTHDR_DEV_H
#define SONDE_SOFTHDR_DEV_H
#include <math.h>
#include "sonde_rs_dev.h"
// (no contraction: the reference is plain C on x86-64 — every product and sum rounded on its own)
#pragma clang fp contract(off)

// mv of the window that ends at call position q >= cur
static RSW_DEV float softhdr_corr64(const float *hist, const float *x, const float sgn, const int cur, const int q, const unsigned char *hdr) {
    double sum = 0.0, normx = 0.0;
    const int e = 64 + (q - cur);                       // window = elements e-63 .. e
    for (int i = 0; i < 64; i++) {
        const int k = e - 63 + i;
        const float v = k < 64 ? hist[k] : sgn * x[cur + (k - 64)];
        const float y = (hdr[i] & 1) ? 1.f : -1.f;
        sum += (double)(y * v);
        normx += (double)(v * v);
    }
    sum /= sqrt(normx * 64.0);
    return (float)sum;
}
// element `lane` of the ring as call position q leaves it: the 64 elements up to q
static RSW_DEV float softhdr_ring64(const float *hist, const float *x, const float sgn, const int cur, const int q, const int lane) {
    const int e = 64 + (q - cur), k = e - 63 + lane;
    return k < 64 ? hist[k] : sgn * x[cur + (k - 64)];
}
#endif
