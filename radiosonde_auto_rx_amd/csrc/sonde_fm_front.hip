// sonde_fm_front.hip — k_fm_front: the front end of the FM slicers for the input a channelizer produces, float32 IQ at a rate at which iq_dec does not
// decimate (sonde_fm_front_dev.h: IQ-dc removal, table mixer, discriminator and FM low-pass of `iq_dec --FM --lpFM --iq fq - <sr> 32`).  One workgroup of
// one wavefront per channel, each channel on a sample clock of its own; a released channel's workgroup returns before it reads anything.  The tap count is
// an argument (iq_dec's 4 sr / 2000 made odd), so an engine at another IF rate instantiates the same kernel.
//
// Floating-point contraction is off in this file: the reference is plain C on x86-64 (every product and sum rounded on its own).
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#define SONDE_FM_FRONT_BODY
#include "sonde_fm_front_dev.h"

namespace {

__global__ __launch_bounds__(64) void k_fm_front(const FmFrontArgs a) {
    const int c = blockIdx.x;
    if (!a.active[c]) return;                                          // a released channel: nothing read, nothing written
    __shared__ FmFrontLds lds;
    fm_front_channel(a.chan + c, a.in + (size_t)c * (size_t)a.ch_stride, a.n, a.fm + (size_t)c * a.ring, a.first, (uint32_t)a.ring - 1,
                     a.raw + (size_t)c * a.rring, a.rring, a.ws2, a.taps, &lds, (int)threadIdx.x);
}

}  // namespace

extern "C" int sonde_launch_fm_front(const FmFrontArgs *a, hipStream_t s) {
    if (a->n_ch < 1 || a->n < 1) return 0;
    if (a->taps < 1 || a->taps > FMF_TAPS_MAX || a->rring > FMF_RING_MAX || a->rring < a->taps + 128 || (a->rring & (a->rring - 1)) ||
        a->ring < a->n || (a->ring & (a->ring - 1)) || a->ch_stride < a->n) return -1;
    hipLaunchKernelGGL(k_fm_front, dim3(a->n_ch), dim3(64), 0, s, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
