// sonde_wxr_dev.h — what the host engine (sonde_wxr.cpp) and the kernel k_wxr_slice (sonde_wxr.hip) share.
#ifndef SONDE_WXR_DEV_H
#define SONDE_WXR_DEV_H
#include <hip/hip_runtime.h>
#include <cstdint>

#define WXR_BITS 552                // BITFRAMELEN
#define WXR_HEADLEN 40
#define WXR_STRIDE 576              // frame_bits of a channel in device memory
#define WXR_UNSET 2
#define WXR_IN_RING 0               // FM samples in a power-of-two ring by absolute sample (the iq_dec front end's fm tap)
#define WXR_IN_F32 1                // FM samples of the call, channel-major: float / int16 / uint8
#define WXR_IN_S16 2
#define WXR_IN_U8 3

// per-channel state between calls: the globals and main() locals of weathex301d.c that outlive a sample
struct WxrChan {
    unsigned long long total;          // sample_count
    unsigned long long t_hdr;          // sample_count when the open header matched
    unsigned long long hist, valid;    // buf[40]: bit values, and which positions hold a bit at all ('x' and the initial bytes do not)
    uint32_t n_run;                    // read_bits_fsk's n of the run in progress
    uint32_t scount;                   // read_rawbit: samples since bitstart
    float sum;                         // read_rawbit: sum of the bit in progress
    int32_t par, found, bit_count, raw, raw_i;   // raw: inside the -b loop; raw_i: bits it has finished since bitstart
};

struct WxrFrame {
    int32_t channel, nbits;
    uint64_t sample;
    uint8_t bits[WXR_BITS];
};

struct WxrArgs {
    WxrChan *chan;
    uint8_t *frames;                   // [n_ch][WXR_STRIDE]
    WxrFrame *q;
    int *q_count;
    const void *in;
    unsigned long long hdr;            // the 40 header bits, first bit highest
    long long ch_stride;               // samples between two channels of `in`
    uint32_t first, mask;              // sample i of the call is in[(first + i) & mask]
    int q_cap, n_ch, n, kind, inv, opt_b;
    float spb;
};

extern "C" int sonde_launch_wxr(const WxrArgs *a, hipStream_t s);
#endif
