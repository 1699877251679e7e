// sonde_drop.hip — k_drop_slice: the slicer of sonde_slice_dev.h as the reference's dropsonde/rd94rd41drop.c has it (read_bits_fsk :207,
// read_rawbit :242 with bitgrenze = sc0 - 1 + i * spb, the frame loop of main :1399-1446), and the completion of a finished frame on the
// device (drop_complete_frame: Manchester pairs -> bytes -> both check masks).  Integer samples, a run of 0 bits leaves no trace
// (`continue` in main), frame_rawbits keeps the header in front (:1353) and is filled from bit 40, -b bits enter the ring, and at the
// end of the input a -b frame whose header is open is completed with '0' bits (print_bitframe :1253).
#include "sonde_drop_dev.h"

namespace {

using namespace sonde_slice;

struct DropSlice {
    typedef int sample_t;
    typedef DropArgs Args;
    static constexpr int BITS = DROP_RAWBITS, STRIDE = DROP_RAWBITS, EDGE = 1;
    static constexpr bool ZERO_RUN_X = false, HDR_PRESET = true, RAW_INTO_RING = true, FINISH = true;

    static __device__ __forceinline__ int sample_bytes(int kind) { return kind == DROP_IN_S16 ? 2 : kind == DROP_IN_U8 ? 1 : 4; }
    // read_signed_sample (:179-202): 16-bit signed, 8-bit unsigned minus 128; the ring through fwrite_fm_blk's 16-bit conversion of iq_dec
    // (x *= 128; x *= 256; (short)x — truncation, wrapping as the x86 conversion does)
    static __device__ __forceinline__ int load_sample(const Args &a, const char *row, int i) {
        const uint32_t k = (a.first + (uint32_t)i) & a.mask;
        if (a.kind == DROP_IN_S16) return (int)((const int16_t *)row)[k];
        if (a.kind == DROP_IN_U8) return (int)((const uint8_t *)row)[k] - 128;
        float v = ((const float *)row)[k] * 128.0f;
        v *= 256.0f;
        return (int)(int16_t)(int)v;
    }
    static __device__ __forceinline__ u64 header(const Args &) { return DROP_HDR40; }
    static __device__ __forceinline__ void complete(const Args &a, int c, const uint8_t *fb, int nraw, u64 t_hdr, int complete, int lane) {
        __shared__ uint8_t by[128];
        drop_complete_frame(fb, nraw, by, a.q, a.q_count, a.q_cap, c, t_hdr, complete, lane);
    }
};

__global__ __launch_bounds__(64) void k_drop_slice(DropArgs a) { slice<DropSlice>(a); }

}  // namespace

extern "C" int sonde_launch_drop(const DropArgs *a, hipStream_t s) {
    if (a->n_ch < 1 || (a->n < 1 && !a->finish)) return 0;
    hipLaunchKernelGGL(k_drop_slice, dim3(a->n_ch), dim3(64), 0, s, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
