// The survey's transform network (radiosonde_auto_rx_amd/csrc/sonde_power_fft.h) executed on the CPU: the same pass bodies the kernel
// k_power_seg<L> compiles, run thread after thread and pass after pass (a workgroup barrier separates the passes on the device and nothing
// else couples the threads).  out[p] = |X|^2 at network position p (bit-reversed bin order), summed over the segments.
#include "../../radiosonde_auto_rx_amd/csrc/sonde_power_fft.h"
#include <cmath>
#include <vector>

namespace {

template <int L, int S0> void mids(pw_c *x, const pw_c *tw) {
    if constexpr (S0 < L - 3) {
        for (int tid = 0; tid < PowerShape<L>::THREADS; tid++) pw_pass_mid<L, S0>(x, tw, tid);
        mids<L, S0 + 3>(x, tw);
    }
}

template <int L> int run(const float *in, int nseg, float *out) {
    using S = PowerShape<L>;
    std::vector<pw_c> x(S::XN), tw(S::N / 2);
    const double PI = 3.14159265358979323846;
    for (int m = 0; m < S::N / 2; m++) { tw[m].x = (float)std::cos(2.0 * PI * m / S::N); tw[m].y = (float)-std::sin(2.0 * PI * m / S::N); }
    std::vector<float> acc((size_t)S::THREADS * S::ACC, 0.f);
    for (int seg = 0; seg < nseg; seg++) {
        const float *p = in + (size_t)seg * 2 * S::N;
        const auto src = [p](int i) { pw_c v; v.x = p[2 * i]; v.y = p[2 * i + 1]; return v; };
        constexpr int R = S::R0 ? S::R0 : 3;
        for (int tid = 0; tid < S::THREADS; tid++) pw_pass_first<L, R>(x.data(), tw.data(), src, tid);
        mids<L, R>(x.data(), tw.data());
        for (int tid = 0; tid < S::THREADS; tid++) pw_pass_last<L>(x.data(), tw.data(), &acc[(size_t)tid * S::ACC], tid);
    }
    for (int tid = 0; tid < S::THREADS; tid++)
        for (int k = 0; k < S::KMAX; k++) {
            const int g = tid + k * S::THREADS;
            if (g < S::GROUPS) for (int e = 0; e < 8; e++) out[8 * g + e] = acc[(size_t)tid * S::ACC + 8 * k + e];
        }
    return S::THREADS;
}

}  // namespace

// in: nseg segments of 2^log2n (re, im) pairs; returns the workgroup size of that instantiation, -1 for a size the kernel does not have
extern "C" int emu_power_segments(int log2n, const float *in, int nseg, float *out) {
    switch (log2n) {
    case 8: return run<8>(in, nseg, out);   case 9: return run<9>(in, nseg, out);   case 10: return run<10>(in, nseg, out);
    case 11: return run<11>(in, nseg, out); case 12: return run<12>(in, nseg, out); case 13: return run<13>(in, nseg, out);
    case 14: return run<14>(in, nseg, out);
    default: return -1;
    }
}
