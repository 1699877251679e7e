// sonde_gps_dev.h — the RS92 position solve's 4-satellite subset search on ONE wavefront (k_gps_subsets, sonde_gps.hip): the closed-form solution and the GDOP of
// every subset of a frame's satellites, and the arg-min the decoder's sequential loop would reach.  Behaviour restated (not code): sonde_gpsnav.cpp closed_form4,
// dop(4, ..), inverse_diagonal4 and the loop of sonde_rs92_fields.cpp solve() (nav_gps_vel.c:682-874, :880-991; rs92mod.c:1160-1230).
//
// SELECTION ONLY.  Nothing computed here is printed: the host solves the winning subset again with its own functions (sonde_rs92_dec_end).  What has to agree
// is which subset wins, and that is decided by + - x / sqrt on doubles alone: k, A, D, c, f, m1..m3, the discriminant, both roots, the norms, G, GtG, det4, the
// cofactor diagonal, gdop.  Those are IEEE-exact here as on the host when no product is fused into an addition, so
//   * every expression below keeps the operand order of sonde_gpsnav.cpp,
//   * contraction is switched off HERE, by pragma, so that no build flag can make the kernel and the emulator differ, and
//   * the file is never compiled with fast-math.
// Transcendentals stay off the deciding path: the rotation by the earth's turn is the host's (the job carries the rotated positions), and the two decisions of
// closed_form4 that go through ecef2elli (atan2, sin, cos; the device's libm may differ from the host's by ulps) raise a DOUBT flag when they are close:
//   * the height gate  height < -1500 || height > 50000 :  |height + 1500| < 0.01 m or |height - 50000| < 0.01 m,
//   * both roots within 60 km of the surface, the one nearer the point below the satellites' mean wins :  |e1 - e2| < 1e-9 degrees.
// These margins are not tolerances on a result.  They are guard bands many orders of magnitude above a few-ulp libm difference (an ulp of the height's operands is
// 1e-9 m, of an angle in degrees 1e-14): a subset inside a band may be decided differently by the two libms, a subset outside cannot.  A frame with any subset in
// doubt is solved by the host's full search; the bands only decide which frames those are.
//
// Compiled twice, like sonde_rs_dev.h: by hipcc into k_gps_subsets and by g++ under tests/emu/wave_emu.h (tests/test_gps_subsets_emu.py).  Control flow around every
// rsw_* call is wave-uniform.
#ifndef SONDE_GPS_DEV_H
#define SONDE_GPS_DEV_H
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "../../include/sonde_rs92.h"
#include "sonde_rs_dev.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define GPSD_GATE_BAND 0.01        // [m] around -1500 and 50000
#define GPSD_NEAR_BAND 1e-9        // [degrees] between e1 and e2

static RSW_DEV double gpsd_sqrt(double v) { return __builtin_sqrt(v); }
static RSW_DEV double gpsd_fabs(double v) { return __builtin_fabs(v); }

// ecef2elli (sonde_gpsnav.cpp:100): the device's atan2 / sin / cos.  Only the height gate and the both-near choice read what it gives
static RSW_DEV void gpsd_ecef2elli(double X, double Y, double Z, double *lat, double *lon, double *alt) {
    constexpr double kPi = 3.1415926535897932384626433832795;
    constexpr double kEarthA = 6378137.0, kEarthB = 6356752.31424518;
    constexpr double kA2B2 = kEarthA * kEarthA - kEarthB * kEarthB;
    const double ea2 = kA2B2 / (kEarthA * kEarthA), eb2 = kA2B2 / (kEarthB * kEarthB);
    const double lam = atan2(Y, X);
    const double p = gpsd_sqrt(X * X + Y * Y);
    const double t = atan2(Z * kEarthA, p * kEarthB);
    const double st = sin(t), ct = cos(t);
    const double phi = atan2(Z + eb2 * kEarthB * st * st * st, p - ea2 * kEarthA * ct * ct * ct);
    const double R = kEarthA / gpsd_sqrt(1 - ea2 * sin(phi) * sin(phi));
    *alt = p / cos(phi) - R;
    *lat = phi * 180.0 / kPi;
    *lon = lam * 180.0 / kPi;
}

// closed_form4 (sonde_gpsnav.cpp:293) up to its return value, on satellites i[0..3] of the job; pos: the chosen root.  *doubt is set where a libm decision was close
static RSW_DEV int gpsd_closed_form4(const sonde_gps_sat_t *sat, const int i0, const int i1, const int i2, const int i3, double pos[3], int *doubt) {
    const int ix[4] = { i0, i1, i2, i3 };
    double p[4], x[4], y[4], z[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { p[i] = sat[ix[i]].p; x[i] = sat[ix[i]].x; y[i] = sat[ix[i]].y; z[i] = sat[ix[i]].z; }

    double dx[3], dy[3], dz[3], dp[3], k[3], A[3][3], D[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        dx[i] = x[0] - x[i + 1]; dy[i] = y[0] - y[i + 1]; dz[i] = z[0] - z[i + 1];
        dp[i] = p[i + 1] - p[0];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        k[i] = dx[i] * dx[i] + dy[i] * dy[i] + dz[i] * dz[i] - dp[i] * dp[i];
        A[i][0] = 2.0 * dx[i]; A[i][1] = 2.0 * dy[i]; A[i][2] = 2.0 * dz[i];
    }
    double t1 = A[1][1] * A[2][2] - A[2][1] * A[1][2];
    double t2 = A[1][0] * A[2][2] - A[2][0] * A[1][2];
    double t3 = A[1][0] * A[2][1] - A[2][0] * A[1][1];
    const double detA = A[0][0] * t1 - A[0][1] * t2 + A[0][2] * t3;
    D[0][0] = t1;  D[1][0] = -t2;  D[2][0] = t3;
    D[0][1] = -A[0][1] * A[2][2] + A[2][1] * A[0][2];
    D[1][1] =  A[0][0] * A[2][2] - A[2][0] * A[0][2];
    D[2][1] = -A[0][0] * A[2][1] + A[2][0] * A[0][1];
    D[0][2] =  A[0][1] * A[1][2] - A[1][1] * A[0][2];
    D[1][2] = -A[0][0] * A[1][2] + A[1][0] * A[0][2];
    D[2][2] =  A[0][0] * A[1][1] - A[1][0] * A[0][1];

    double c[3], f[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        c[i] = (D[i][0] * dp[0] + D[i][1] * dp[1] + D[i][2] * dp[2]) * 2.0 / detA;
        f[i] = (D[i][0] * k[0] + D[i][1] * k[1] + D[i][2] * k[2]) / detA;
    }
    const double m1 = c[0] * c[0] + c[1] * c[1] + c[2] * c[2] - 1.0;
    const double m2 = -2.0 * (c[0] * f[0] + c[1] * f[1] + c[2] * f[2]);
    const double m3 = f[0] * f[0] + f[1] * f[1] + f[2] * f[2];
    t1 = m2 * m2 - 4.0 * m1 * m3;
    if (t1 < 0) return -1;

    const double d0 = (-m2 - gpsd_sqrt(t1)) * 0.5 / m1, d1 = (-m2 + gpsd_sqrt(t1)) * 0.5 / m1;
    const double s00 = c[0] * d0 - f[0] + x[0], s01 = c[1] * d0 - f[1] + y[0], s02 = c[2] * d0 - f[2] + z[0];
    const double s10 = c[0] * d1 - f[0] + x[0], s11 = c[1] * d1 - f[1] + y[0], s12 = c[2] * d1 - f[2] + z[0];
    t1 = gpsd_fabs(gpsd_sqrt(s00 * s00 + s01 * s01 + s02 * s02) - 6371000.0);
    t2 = gpsd_fabs(gpsd_sqrt(s10 * s10 + s11 * s11 + s12 * s12) - 6371000.0);
    int pick = 0;
    bool both = false;
    if (t2 < t1 && t1 >= 60000) pick = 1;
    else if (t2 < 60000) both = true;
    // ecef2elli of the point below the satellites' mean (q = 0, both near only), of root 0 (q = 1) and of root 1 (q = 2): ONE copy of the transcendental code, the
    // points chosen by selects (an array indexed by q would live in scratch memory)
    double laS = 0, loS = 0, la0 = 0, lo0 = 0, al0 = 0, la1 = 0, lo1 = 0, al1 = 0;
    const int q_lo = both ? 0 : 1 + pick, q_hi = both ? 3 : 2 + pick;
#if !defined(SONDE_RS_EMU)
#pragma clang loop unroll(disable)
#endif
    for (int q = q_lo; q < q_hi; q++) {
        const double ex = q == 0 ? (x[0] + x[1] + x[2] + x[3]) / 4.0 : q == 1 ? s00 : s10;
        const double ey = q == 0 ? (y[0] + y[1] + y[2] + y[3]) / 4.0 : q == 1 ? s01 : s11;
        const double ez = q == 0 ? (z[0] + z[1] + z[2] + z[3]) / 4.0 : q == 1 ? s02 : s12;
        double la, lo, al;
        gpsd_ecef2elli(ex, ey, ez, &la, &lo, &al);
        if (q == 0) { laS = la; loS = lo; }
        else if (q == 1) { la0 = la; lo0 = lo; al0 = al; }
        else { la1 = la; lo1 = lo; al1 = al; }
    }
    if (both) {
        const double e1 = gpsd_sqrt((laS - la0) * (laS - la0) + (loS - lo0) * (loS - lo0));
        const double e2 = gpsd_sqrt((laS - la1) * (laS - la1) + (loS - lo1) * (loS - lo1));
        if (e2 < e1) pick = 1;
        if (gpsd_fabs(e1 - e2) < GPSD_NEAR_BAND) *doubt = 1;
    }
    const double height = pick ? al1 : al0;
    pos[0] = pick ? s10 : s00; pos[1] = pick ? s11 : s01; pos[2] = pick ? s12 : s02;
    if (gpsd_fabs(height + 1500.0) < GPSD_GATE_BAND || gpsd_fabs(height - 50000.0) < GPSD_GATE_BAND) *doubt = 1;
    if (height < -1500.0 || height > 50000.0) return -2;
    return 0;
}

// the 4x4 cofactor code of sonde_gpsnav.cpp:30-58 with its index sets as template parameters: every m[..][..] is a register
template <int a, int b, int c, int d> static RSW_DEV double gpsd_det2(const double (&m)[4][4]) { return m[a][c] * m[b][d] - m[a][d] * m[b][c]; }
template <int r0, int r1, int r2, int c0, int c1, int c2> static RSW_DEV double gpsd_det3(const double (&m)[4][4]) {
    return m[r0][c0] * gpsd_det2<r1, r2, c1, c2>(m) - m[r0][c1] * gpsd_det2<r1, r2, c0, c2>(m) + m[r0][c2] * gpsd_det2<r1, r2, c0, c1>(m);
}
static RSW_DEV double gpsd_det4(const double (&m)[4][4]) {
    return m[0][0] * gpsd_det3<1, 2, 3, 1, 2, 3>(m) - m[0][1] * gpsd_det3<1, 2, 3, 0, 2, 3>(m)
         + m[0][2] * gpsd_det3<1, 2, 3, 0, 1, 3>(m) - m[0][3] * gpsd_det3<1, 2, 3, 0, 1, 2>(m);
}

// dop(4, ..) at the subset's closed-form position and gdop = sqrt(DOP[0] + .. + DOP[3]); -1 where the inverse fails (|det| < 1e-4), as solve() sets it
static RSW_DEV double gpsd_gdop4(const sonde_gps_sat_t *sat, const int i0, const int i1, const int i2, const int i3, const double pos[3]) {
    const int ix[4] = { i0, i1, i2, i3 };
    double G[4][4], GtG[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const double d0 = sat[ix[i]].X - pos[0], d1 = sat[ix[i]].Y - pos[1], d2 = sat[ix[i]].Z - pos[2];
        const double norm = gpsd_sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        G[i][0] = d0 / norm; G[i][1] = d1 / norm; G[i][2] = d2 / norm;
        G[i][3] = 1;
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 4; k++) acc += G[k][i] * G[k][j];
            GtG[i][j] = acc;
        }
    const double det = gpsd_det4(GtG);
    if (gpsd_fabs(det) < 0.0001) return -1;
    const double q0 = gpsd_det3<1, 2, 3, 1, 2, 3>(GtG) / det, q1 = gpsd_det3<0, 2, 3, 0, 2, 3>(GtG) / det;
    const double q2 = gpsd_det3<0, 1, 3, 0, 1, 3>(GtG) / det, q3 = gpsd_det3<0, 1, 2, 0, 1, 2>(GtG) / det;
    return gpsd_sqrt(q0 + q1 + q2 + q3);
}

// subset number `at` (< C(n,4)) of the nested loops ix[0] < ix[1] < ix[2] < ix[3] over 0 .. n-1: the first element is the smallest a with more than `at` subsets
// starting at or below it, and so on; C(m,3), C(m,2), C(m,1) subsets remain behind an element with m satellites above it
static RSW_DEV void gpsd_unrank4(int n, int at, int *i0, int *i1, int *i2, int *i3) {
    int a = 0;
    for (;; a++) { const int m = n - 1 - a, cnt = m * (m - 1) * (m - 2) / 6; if (at < cnt) break; at -= cnt; }
    int b = a + 1;
    for (;; b++) { const int m = n - 1 - b, cnt = m * (m - 1) / 2; if (at < cnt) break; at -= cnt; }
    int c = b + 1;
    for (;; c++) { const int m = n - 1 - c; if (at < m) break; at -= m; }
    *i0 = a; *i1 = b; *i2 = c; *i3 = c + 1 + at;
}

// lowest set bit's position of a non-zero mask
static RSW_DEV int gpsd_first(unsigned long long m) { return 63 - rsw_clzll(m & (0ull - m)); }

// One job on one wave.  job: in LDS (or any memory every lane reads), n already known to be 4 .. 12.  Lane l takes subsets l, l + 64, ..; lane 0 writes *out.
static RSW_DEV void gps_wave_solve(const sonde_gps_job_t *job, const int lane, sonde_gps_pick_t *out) {
    const int n = job->n;
    const int total = n * (n - 1) * (n - 2) * (n - 3) / 24;
    const int rounds = (total + 63) >> 6;                             // <= 8
    int num = 0, doubt = 0, bidx = -1;
    unsigned long long bkey = ~0ull;                                  // bits of the lane's best gdop: of positive doubles, ordered as the doubles are
    for (int r = 0; r < rounds; r++) {
        const int at = lane + 64 * r;
        int ok = 0, db = 0;
        if (at < total) {
            int i0, i1, i2, i3;
            double pos[3];
            gpsd_unrank4(n, at, &i0, &i1, &i2, &i3);
            if (gpsd_closed_form4(job->sat, i0, i1, i2, i3, pos, &db) == 0) {
                ok = 1;
                const double gdop = gpsd_gdop4(job->sat, i0, i1, i2, i3, pos);
                if (gdop > 0 && gdop < 1000.0) {                      // (NaN never passes)
                    unsigned long long key;
                    memcpy(&key, &gdop, 8);
                    if (key < bkey) { bkey = key; bidx = at; }        // strictly: the lane's earlier subset keeps a tie
                }
            }
        }
        num += rsw_popcll(rsw_ballot(ok != 0));
        doubt |= rsw_ballot(db != 0) != 0;
    }
    // arg-min over the lanes: the smallest key bit by bit from the top, then among equal keys the smallest subset index (what `gdop < gdop0` leaves in a
    // sequential pass: the first of the smallest)
    unsigned long long cand = rsw_ballot(bidx >= 0);
    int best = -1;
    unsigned long long gbits = 0;
    if (cand) {
        for (int b = 62; b >= 0; b--) {                               // (bit 63, the sign, is clear in every key)
            const unsigned long long z = rsw_ballot(((cand >> lane) & 1) && !((bkey >> b) & 1));
            if (z) cand = z;
        }
        for (int b = 8; b >= 0; b--) {                                // subset indices are below 512
            const unsigned long long z = rsw_ballot(((cand >> lane) & 1) && !((bidx >> b) & 1));
            if (z) cand = z;
        }
        const int w = gpsd_first(cand);
        best = rsw_bcast(bidx, w);
        const unsigned lo = (unsigned)rsw_bcast((int)(unsigned)(bkey & 0xffffffffu), w), hi = (unsigned)rsw_bcast((int)(unsigned)(bkey >> 32), w);
        gbits = ((unsigned long long)hi << 32) | lo;
    }
    if (lane == 0) {
        double g;
        memcpy(&g, &gbits, 8);
        out->num = num; out->best = best; out->doubt = doubt; out->n = n; out->gdop = g;
    }
}
#endif
