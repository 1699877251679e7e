// sonde_power_dev.h — launch interface between the survey's host engine (sonde_power.cpp) and its kernels (sonde_power.hip).
#ifndef SONDE_POWER_DEV_H
#define SONDE_POWER_DEV_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PW_LOG2_MIN 8
#define PW_LOG2_MAX 14

struct PowerArgs {
    const void  *in;            // new samples of the call: stream c at sample c * stride
    const void  *tail;          // [n_streams][nfft] samples in the input format: what earlier calls left over (tail_len of them)
    const float2 *tw;           // [nfft / 2] exp(-2 pi i m / nfft)
    const float *win;           // [nfft] window weights, nullptr = rectangular
    float       *partial;       // [n_streams][workgroups][nfft] sums of |X|^2 over a workgroup's segments, in bit-reversed bin order
    double      *acc;           // [n_streams][nfft] the persistent accumulator, same order
    long long    stride;        // samples between streams in `in`
    int          tail_len;      // samples per stream in `tail`
    int          nseg;          // whole segments per stream in (tail ++ in)
    int          n_streams;
    int          bits;          // 8 (cu8), 16 (cs16), 32 (cf32)
    int          log2n;
    int          workgroups;    // per stream: workgroup w transforms segments w, w + workgroups, ...
};

struct PowerKernelInfo { int threads, lds_bytes, max_per_cu; };

// occupancy of the transform kernel for 2^log2n points as the runtime reports it (workgroups per CU), its workgroup size and LDS
extern "C" int sonde_power_kernel_info(int log2n, PowerKernelInfo *out);
// transform + accumulate + fold of one call; then the samples behind the last whole segment go to `tail`: count samples per stream from
// in[src_off] to tail[dst_off]
extern "C" int sonde_launch_power(const PowerArgs *a, void *tail_rw, int src_off, int dst_off, int count, hipStream_t s);

#endif
