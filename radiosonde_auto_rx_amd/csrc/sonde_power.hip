// sonde_power.hip — spectrum survey: averaged periodogram of wideband IQ streams (the rtl_power step of auto_rx, autorx/sdr_wrappers.py:571-766).
//
// k_power_seg<L>: one workgroup transforms whole segments of 2^L samples (sonde_power_fft.h: exact twiddles, natural in / bit-reversed out)
//   and keeps the sum of |X|^2 over ITS segments of the call in registers (f32); at the end it writes that sum as one row of `partial`.
//   The grid is [workgroups per stream][streams]; workgroup w takes segments w, w + workgroups, ...  A segment's samples come from the
//   carried tail of earlier calls first and from the call's input behind it, converted as the family does (cs16 / 32768, (cu8 - 128) / 128,
//   cf32 as it is) and weighted by the window.
// k_power_fold: adds the rows of `partial` in row order, in double, to the persistent accumulator.  No floating-point atomics anywhere: the
//   same call pattern gives the same bits.
// k_power_tail: moves the samples behind the last whole segment into the tail buffer (after the transform has read it).
#include "sonde_power_dev.h"
#include "sonde_power_fft.h"
#include "../../include/sonde_hip.h"
#include <cstdio>

namespace {

struct PowerSrc {
    const PowerArgs &a;
    const size_t in0, tail0;        // first sample of this stream in `in` / `tail`
    const long long q0;             // position of the segment's first sample in (tail ++ in)
    __device__ __forceinline__ float2 operator()(const int i) const {
        const long long q = q0 + i;
        const bool t = q < a.tail_len;
        const void *base = t ? a.tail : a.in;
        const size_t k = t ? tail0 + (size_t)q : in0 + (size_t)(q - a.tail_len);
        float2 v;
        if (a.bits == 16) { const short2 s = ((const short2 *)base)[k]; v = make_float2((float)s.x * 3.0517578125e-05f, (float)s.y * 3.0517578125e-05f); }
        else if (a.bits == 8) { const uchar2 u = ((const uchar2 *)base)[k]; v = make_float2((float)((int)u.x - 128) * 0.0078125f, (float)((int)u.y - 128) * 0.0078125f); }
        else v = ((const float2 *)base)[k];
        if (a.win) { const float w = a.win[i]; v.x *= w; v.y *= w; }
        return v;
    }
};

template <int L>
__global__ __launch_bounds__(PowerShape<L>::THREADS) void k_power_seg(const PowerArgs a) {
    using S = PowerShape<L>;
    __shared__ float2 x[S::XN];
    const int tid = threadIdx.x, c = blockIdx.y;
    float acc[S::ACC];
#pragma unroll
    for (int i = 0; i < S::ACC; i++) acc[i] = 0.f;
    const auto sync = [] { __syncthreads(); };
    for (int seg = blockIdx.x; seg < a.nseg; seg += gridDim.x) {
        const PowerSrc src{a, (size_t)c * (size_t)a.stride, (size_t)c * S::N, (long long)seg * S::N};
        constexpr int R = S::R0 ? S::R0 : 3;
        pw_pass_first<L, R>(x, a.tw, src, tid);
        __syncthreads();
        pw_passes_mid<L, R>(x, a.tw, tid, sync);
        pw_pass_last<L>(x, a.tw, acc, tid);
        __syncthreads();                                       // the next segment's first pass overwrites what the last pass reads
    }
    float *row = a.partial + ((size_t)c * gridDim.x + blockIdx.x) * S::N;
#pragma unroll
    for (int k = 0; k < S::KMAX; k++) {
        const int g = tid + k * S::THREADS;
        if (g < S::GROUPS) {
            ((float4 *)(row + 8 * g))[0] = make_float4(acc[8 * k], acc[8 * k + 1], acc[8 * k + 2], acc[8 * k + 3]);
            ((float4 *)(row + 8 * g))[1] = make_float4(acc[8 * k + 4], acc[8 * k + 5], acc[8 * k + 6], acc[8 * k + 7]);
        }
    }
}

__global__ __launch_bounds__(256) void k_power_fold(const float *partial, double *acc, const int rows, const int n) {
    const int p = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (p >= n) return;
    const float *col = partial + (size_t)c * rows * n + p;
    double sum = 0.0;
    for (int w = 0; w < rows; w++) sum += (double)col[(size_t)w * n];
    acc[(size_t)c * n + p] += sum;
}

// T: one complex sample of the input format
template <class T>
__global__ __launch_bounds__(256) void k_power_tail(const T *in, T *tail, const long long stride, const int n, const int src_off, const int dst_off, const int count) {
    const int j = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (j < count) tail[(size_t)c * n + dst_off + j] = in[(size_t)c * (size_t)stride + src_off + j];
}

template <int L> int launch_seg(const PowerArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_power_seg<L>, dim3(a.workgroups, a.n_streams), dim3(PowerShape<L>::THREADS), 0, s, a);
    return 0;
}

template <int L> int kernel_info(PowerKernelInfo *out) {
    out->threads = PowerShape<L>::THREADS;
    out->lds_bytes = PowerShape<L>::XN * (int)sizeof(float2);
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_power_seg<L>, PowerShape<L>::THREADS, 0) != hipSuccess || per_cu < 1) { (void)hipGetLastError(); return SONDE_E_NOGPU; }
    out->max_per_cu = per_cu;
    return 0;
}

}  // namespace

#define PW_DISPATCH(log2n, CALL) \
    switch (log2n) { \
    case 8: return CALL(8); case 9: return CALL(9); case 10: return CALL(10); case 11: return CALL(11); \
    case 12: return CALL(12); case 13: return CALL(13); case 14: return CALL(14); \
    default: return SONDE_E_ARG; }

extern "C" int sonde_power_kernel_info(int log2n, PowerKernelInfo *out) {
#define PW_INFO(L) kernel_info<L>(out)
    PW_DISPATCH(log2n, PW_INFO)
}

static int launch_seg_any(const PowerArgs &a, hipStream_t s) {
#define PW_SEG(L) launch_seg<L>(a, s)
    PW_DISPATCH(a.log2n, PW_SEG)
}

extern "C" int sonde_launch_power(const PowerArgs *a, void *tail_rw, int src_off, int dst_off, int count, hipStream_t s) {
    const int n = 1 << a->log2n;
    if (a->nseg > 0) {
        if (a->workgroups < 1 || a->workgroups > a->nseg) return SONDE_E_ARG;
        const int rc = launch_seg_any(*a, s);
        if (rc) return rc;
        hipLaunchKernelGGL(k_power_fold, dim3((n + 255) / 256, a->n_streams), dim3(256), 0, s, a->partial, a->acc, a->workgroups, n);
    }
    if (count > 0) {
        if (dst_off < 0 || src_off < 0 || dst_off + count > n) return SONDE_E_ARG;
        const dim3 grid((count + 255) / 256, a->n_streams);
        if (a->bits == 16) hipLaunchKernelGGL(k_power_tail<short2>, grid, dim3(256), 0, s, (const short2 *)a->in, (short2 *)tail_rw, a->stride, n, src_off, dst_off, count);
        else if (a->bits == 8) hipLaunchKernelGGL(k_power_tail<uchar2>, grid, dim3(256), 0, s, (const uchar2 *)a->in, (uchar2 *)tail_rw, a->stride, n, src_off, dst_off, count);
        else hipLaunchKernelGGL(k_power_tail<float2>, grid, dim3(256), 0, s, (const float2 *)a->in, (float2 *)tail_rw, a->stride, n, src_off, dst_off, count);
    }
    return hipGetLastError() == hipSuccess ? 0 : SONDE_E_NOGPU;
}
