// sonde_wxr.hip — k_wxr_slice: the slicer of sonde_slice_dev.h as the reference's weathex/weathex301d.c has it (read_bits_fsk :171,
// read_rawbit :200 with bitgrenze from sample_count 0 of the bit start, the frame loop of main :649-707): float samples, a run of 0 bits
// puts an 'x' into the header ring (:660), frame_bits is filled from bit 0 with the header first, and -b bits stay out of the ring.
#include "sonde_wxr_dev.h"

namespace {

using namespace sonde_slice;

struct WxrSlice {
    typedef float sample_t;
    typedef WxrArgs Args;
    static constexpr int BITS = WXR_BITS, STRIDE = WXR_STRIDE, EDGE = 0;
    static constexpr bool ZERO_RUN_X = true, HDR_PRESET = false, RAW_INTO_RING = false, FINISH = false;

    static __device__ __forceinline__ int sample_bytes(int kind) { return kind == WXR_IN_S16 ? 2 : kind == WXR_IN_U8 ? 1 : 4; }
    // f32read_signed_sample (:139-167): 8-bit unsigned and 16-bit signed PCM scaled to +-1, float as it is
    static __device__ __forceinline__ float load_sample(const Args &a, const char *row, int i) {
        const uint32_t k = (a.first + (uint32_t)i) & a.mask;
        if (a.kind == WXR_IN_S16) return (float)((const int16_t *)row)[k] / 32768.0f;
        if (a.kind == WXR_IN_U8) return (float)((int)((const uint8_t *)row)[k] - 128) / 128.0f;
        return ((const float *)row)[k];
    }
    static __device__ __forceinline__ u64 header(const Args &a) { return a.hdr; }
    // a frame leaves the kernel only when it is full; sonde_wxr_finish reads a cut one from the state on the host
    static __device__ void complete(const Args &a, int c, const uint8_t *fb, int, u64 t_hdr, int, int lane) {
        __syncthreads();
        int idx = 0;
        if (lane == 0) idx = atomicAdd(a.q_count, 1);
        idx = uni(__shfl(idx, 0));
        if (idx < a.q_cap) {                                   // a full queue drops the frame; the host sees the count and reports it
            WxrFrame *f = a.q + idx;
            if (lane == 0) { f->channel = c; f->nbits = WXR_BITS; f->sample = t_hdr; }
            for (int j = lane; j < WXR_BITS; j += 64) f->bits[j] = fb[j];
        }
        __syncthreads();
    }
};

__global__ __launch_bounds__(64) void k_wxr_slice(WxrArgs a) { slice<WxrSlice>(a); }

}  // namespace

extern "C" int sonde_launch_wxr(const WxrArgs *a, hipStream_t s) {
    if (a->n_ch < 1 || a->n < 1) return 0;
    hipLaunchKernelGGL(k_wxr_slice, dim3(a->n_ch), dim3(64), 0, s, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
