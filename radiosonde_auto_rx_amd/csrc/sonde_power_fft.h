// sonde_power_fft.h — the survey's transform (sonde_power.hip): a complex FFT of 2^L points, L = 8 .. 14, in LDS with EXACT twiddles
// (tabulated by the host in double precision and rounded once: tw[m] = exp(-2 pi i m / N), m < N/2).  Not the scanner's sonde_fft_dev.h,
// whose table is the reference's drifting float recurrence and fixed at 8192 points.
//
// Decimation in frequency: natural order in, bit-reversed order out (X[k] ends at position brev_L(k)); the survey accumulates |X|^2 in
// that order and the host undoes the permutation once per fetch, so no reordering pass runs on the device.  Stages are merged into register
// passes of radix 8 (groups of 8 elements at stride 2^p_lo), the L % 3 left-over stages form a first pass of radix 2 or 4; the first pass
// takes its elements from the sample source instead of LDS, the last one hands them to the accumulator instead of storing them.
//
// The pass bodies are plain C++ over (tid, nthreads): tests/emu/power_fft_emu.cpp runs the same text on the CPU, thread after thread and
// pass after pass (a workgroup barrier separates the passes and nothing else couples the threads).
#ifndef SONDE_POWER_FFT_H
#define SONDE_POWER_FFT_H

#ifdef __HIPCC__
#define PW_FN __device__ __forceinline__
#define PW_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
typedef float2 pw_c;
#else
#define PW_FN inline
#define PW_SCHED_FENCE() ((void)0)
struct pw_c { float x, y; };
#endif

// LDS index of element i: i + (i >> 4) + (i >> 8), as XI() of the scanner's transform — the element strides 1, 8, 64, 512, 4096 of the
// register passes all spread over the banks
#define PW_XI(i) ((i) + ((i) >> 4) + ((i) >> 8))

template <int L> struct PowerShape {
    static constexpr int N = 1 << L;
    static constexpr int XN = N + N / 16 + N / 256;                             // padded elements: 17472 (139776 bytes) at 16384 points
    // one radix-8 group per thread and pass up to 4096 points, then 512 threads with 2 and 4 groups each: at 1024 threads (128 registers)
    // the 16 accumulators of 16384 points beside a group's elements and twiddles did not fit without scratch
    static constexpr int THREADS = N / 8 >= 512 ? 512 : (N / 8 < 64 ? 64 : N / 8);
    static constexpr int R0 = L % 3;                                            // radix-2^R0 first pass (0: the first pass is radix 8 too)
    static constexpr int GROUPS = N / 8;                                        // radix-8 groups per pass
    static constexpr int KMAX = (GROUPS + THREADS - 1) / THREADS;               // groups per thread in a radix-8 pass
    static constexpr int ACC = 8 * KMAX;                                        // accumulator registers per thread
};

PW_FN pw_c pw_cmul(pw_c a, pw_c b) { pw_c r; r.x = a.x * b.x - a.y * b.y; r.y = a.x * b.y + a.y * b.x; return r; }

// R merged stages s0 .. s0+R-1 on the 2^R elements base + (e << p_lo), p_lo = L - s0 - R.  Stage s pairs the elements that differ in bit
// L-1-s: (a, b) -> (a + b, (a - b) W_N^((i mod h) 2^s)), h = 2^(L-1-s), i the index of a.
template <int L, int R, int S0>
PW_FN void pw_butterflies(pw_c *v, const pw_c *tw, const int base) {
    constexpr int E = 1 << R, s0 = S0;
    constexpr int p_lo = L - s0 - R;
#pragma unroll
    for (int j = 0; j < R; j++) {
        const int s = s0 + j, bit = 1 << (R - 1 - j), hbits = p_lo + (R - 1 - j);
#pragma unroll
        for (int e = 0; e < E; e++) {
            if (e & bit) continue;
            const pw_c a = v[e], b = v[e | bit];
            pw_c d; d.x = a.x - b.x; d.y = a.y - b.y;
            v[e].x = a.x + b.x; v[e].y = a.y + b.y;
            if (hbits == 0) { v[e | bit] = d; continue; }                       // last stage: W^0
            const int idx = base + (e << p_lo);
            v[e | bit] = pw_cmul(d, tw[(idx & ((1 << hbits) - 1)) << s]);
        }
        PW_SCHED_FENCE();                                                       // one stage's twiddles in registers at a time
    }
}

// first pass: SRC(i) -> sample i of the segment, already converted and windowed
template <int L, int R, class SRC>
PW_FN void pw_pass_first(pw_c *x, const pw_c *tw, const SRC &src, const int tid) {
    constexpr int E = 1 << R, NG = (1 << L) >> R, p_lo = L - R;
#pragma unroll 1
    for (int g = tid; g < NG; g += PowerShape<L>::THREADS) {
        pw_c v[E];
#pragma unroll
        for (int e = 0; e < E; e++) v[e] = src(g + (e << p_lo));
        pw_butterflies<L, R, 0>(v, tw, g);
#pragma unroll
        for (int e = 0; e < E; e++) x[PW_XI(g + (e << p_lo))] = v[e];
    }
}

// a radix-8 pass LDS -> LDS starting at stage s0
template <int L, int S0>
PW_FN void pw_pass_mid(pw_c *x, const pw_c *tw, const int tid) {
    constexpr int p_lo = L - S0 - 3;
#pragma unroll 1
    for (int g = tid; g < PowerShape<L>::GROUPS; g += PowerShape<L>::THREADS) {
        const int low = g & ((1 << p_lo) - 1), high = g >> p_lo;
        const int base = (high << (p_lo + 3)) | low;
        pw_c v[8];
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] = x[PW_XI(base + (e << p_lo))];
        pw_butterflies<L, 3, S0>(v, tw, base);
#pragma unroll
        for (int e = 0; e < 8; e++) x[PW_XI(base + (e << p_lo))] = v[e];
    }
}

// the radix-8 passes between the first and the last, each followed by SYNC() (the workgroup barrier)
template <int L, int S0, class SYNC>
PW_FN void pw_passes_mid(pw_c *x, const pw_c *tw, const int tid, const SYNC &sync) {
    if constexpr (S0 < L - 3) {
        pw_pass_mid<L, S0>(x, tw, tid);
        sync();
        pw_passes_mid<L, S0 + 3>(x, tw, tid, sync);
    }
}

// the last pass (stages L-3 .. L-1, elements 8 g .. 8 g + 7): acc[8 k + e] += |X|^2 of position 8 (tid + k THREADS) + e
template <int L>
PW_FN void pw_pass_last(const pw_c *x, const pw_c *tw, float *acc, const int tid) {
#pragma unroll
    for (int k = 0; k < PowerShape<L>::KMAX; k++) {
        const int g = tid + k * PowerShape<L>::THREADS;
        if (g < PowerShape<L>::GROUPS) {
            pw_c v[8];
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] = x[PW_XI(8 * g + e)];
            pw_butterflies<L, 3, L - 3>(v, tw, 8 * g);
#pragma unroll
            for (int e = 0; e < 8; e++) acc[8 * k + e] += v[e].x * v[e].x + v[e].y * v[e].y;
        }
        PW_SCHED_FENCE();                                                       // one group's 8 elements in registers at a time
    }
}

#endif
