// sonde_drop.hip — k_drop_slice: the slicer of sonde_slice_dev.h as the reference's dropsonde/rd94rd41drop.c has it (read_bits_fsk :207,
// read_rawbit :242 with bitgrenze = sc0 - 1 + i * spb, the frame loop of main :1399-1446), and the completion of a finished frame on the
// device (drop_complete_frame: Manchester pairs -> bytes -> both check masks).  Integer samples, a run of 0 bits leaves no trace
// (`continue` in main), frame_rawbits keeps the header in front (:1353) and is filled from bit 40, -b bits enter the ring, and at the
// end of the input a -b frame whose header is open is completed with '0' bits (print_bitframe :1253).
// Engines created with bits = 32 hand their channels out at run time: k_drop_slice_rt (the active mask, one channel finished on its own) and
// k_drop_restart; every other engine launches k_drop_slice as it always was.
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
// engines whose channels are handed out at run time (created with bits = 32): the active mask, workgroup b on channel a.ch0 + b
__global__ __launch_bounds__(64) void k_drop_slice_rt(DropArgs a) { slice<DropSlice, true>(a); }

// Channel restart: channel c becomes what create builds — the front end's record (built on the host by the function create uses), a zeroed FM row and
// unfiltered history, the slicer's record (par = 1, bit_count = 40), the frame bits with the preset header in front — and is marked active.  Grid-stride over
// the longest of the rows; every index is checked against its own row length, so nothing outside channel c is written.
__global__ __launch_bounds__(256) void k_drop_restart(const DropArgs a, const FmFrontArgs f, const int c, const FmFrontChan fresh) {
    if (c < 0 || c >= a.n_ch || c >= f.n_ch) return;
    const size_t step = (size_t)gridDim.x * blockDim.x;
    const size_t ring = (size_t)f.ring, rring = (size_t)f.rring;
    float *fm = f.fm + (size_t)c * ring, *raw = f.raw + (size_t)c * rring;
    uint8_t *frame = a.frames + (size_t)c * DROP_RAWBITS;
    size_t top = ring > rring ? ring : rring;
    if ((size_t)DROP_RAWBITS > top) top = DROP_RAWBITS;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < top; i += step) {
        if (i < ring) fm[i] = 0.f;
        if (i < rring) raw[i] = 0.f;
        if (i < (size_t)DROP_RAWBITS) frame[i] = i < DROP_HEADLEN ? (uint8_t)((DROP_HDR40 >> (DROP_HEADLEN - 1 - i)) & 1) : (uint8_t)0;   // frame_rawbits (:1353)
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        DropChan s;
        s.total = 0; s.t_hdr = 0; s.hist = 0; s.valid = 0; s.n_run = 0; s.scount = 0; s.sum = 0;
        s.par = 1; s.found = 0; s.bit_count = DROP_HEADLEN; s.raw = 0; s.raw_i = 0;
        f.chan[c] = fresh; a.chan[c] = s; a.active[c] = 1;
    }
}

}  // namespace

extern "C" int sonde_launch_drop(const DropArgs *a, hipStream_t s) {
    if (a->n_ch < 1 || (a->n < 1 && !a->finish)) return 0;
    if (a->active) hipLaunchKernelGGL(k_drop_slice_rt, dim3(a->n_ch), dim3(64), 0, s, *a);
    else hipLaunchKernelGGL(k_drop_slice, dim3(a->n_ch), dim3(64), 0, s, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int sonde_launch_drop_restart(const DropArgs *a, const FmFrontArgs *f, int c, const FmFrontChan *fresh, hipStream_t s) {
    hipLaunchKernelGGL(k_drop_restart, dim3(8), dim3(256), 0, s, *a, *f, c, *fresh);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
