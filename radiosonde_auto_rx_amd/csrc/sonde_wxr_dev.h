// sonde_wxr_dev.h — what the host engine (sonde_wxr.cpp) and the kernel k_wxr_slice (sonde_wxr.hip) share.
#ifndef SONDE_WXR_DEV_H
#define SONDE_WXR_DEV_H
#include "sonde_slice_dev.h"

#define WXR_BITS 552                // BITFRAMELEN
#define WXR_HEADLEN SLICE_HEADLEN
#define WXR_STRIDE 576              // frame_bits of a channel in device memory
#define WXR_UNSET 2
#define WXR_IN_RING 0               // FM samples in a power-of-two ring by absolute sample (the iq_dec front end's fm tap)
#define WXR_IN_F32 1                // FM samples of the call, channel-major: float / int16 / uint8
#define WXR_IN_S16 2
#define WXR_IN_U8 3

typedef SliceChan<float> WxrChan;

struct WxrFrame {
    int32_t channel, nbits;
    uint64_t sample;
    uint8_t bits[WXR_BITS];
};

typedef SliceArgs<float, WxrFrame> WxrArgs;

extern "C" int sonde_launch_wxr(const WxrArgs *a, hipStream_t s);
#endif
