// sonde_drop_dev.h — what the host engine (sonde_drop.cpp), the slicer kernel k_drop_slice (sonde_drop.hip) and the soft-bit consumer
// k_softin_drop (sonde_softin_dev.hip) share: the per-channel state records, the frame record, and the completion of a frame on the device.
#ifndef SONDE_DROP_DEV_H
#define SONDE_DROP_DEV_H
#include "sonde_slice_dev.h"
#include "sonde_fm_front_dev.h"

#define DROP_RAWBITS 2400           // RAWBITFRAME_LEN
#define DROP_FRAME_LEN 120
#define DROP_HEADLEN SLICE_HEADLEN
#define DROP_HDR40 0xA9555995A9ULL  // FC 1D as Manchester-coded 8N1 (header[HEADOFS..] of rd94rd41drop.c), first raw bit highest
#define DROP_IN_RING 0              // FM samples in a power-of-two float ring by absolute sample (the iq_dec front end's fm tap), read
                                    // through iq_dec's 16-bit output conversion
#define DROP_IN_S16 1               // FM samples of the call, channel-major: int16 / uint8
#define DROP_IN_U8 2

typedef SliceChan<int32_t> DropChan;

struct DropFrame {
    int32_t channel, nraw, complete, err94, err41, pad;
    uint64_t sample;
    uint8_t bytes[DROP_FRAME_LEN];
};

typedef SliceArgs<int32_t, DropFrame> DropArgs;

// (a->active set: the run-time-channel form k_drop_slice_rt, workgroup b on channel a->ch0 + b)
extern "C" int sonde_launch_drop(const DropArgs *a, hipStream_t s);
// k_drop_restart: channel c of an engine with a front end of its own (sonde_fm_front_dev.h) becomes what create builds, and active
extern "C" int sonde_launch_drop_restart(const DropArgs *a, const FmFrontArgs *f, int c, const FmFrontChan *fresh, hipStream_t s);

#ifdef __HIPCC__
// start and length of the checked bytes; the check word follows them, high byte first.  0..4: chksum16 (RD94), 5..11: CRC-16 (RD41)
static __constant__ uint8_t DROP_BLK[12][2] = { { 2, 3 }, { 7, 17 }, { 26, 47 }, { 75, 18 }, { 95, 21 },
                                         { 2, 3 }, { 7, 16 }, { 25, 17 }, { 44, 12 }, { 58, 13 }, { 73, 27 }, { 102, 14 } };

// print_bitframe up to the check masks, by one wavefront: raw bits fb[0..nraw) (0 / 1; behind nraw '0') -> Manchester pairs -> 8N1 data
// bits -> 120 bytes (a lane per byte), then a lane per block: five chksum16 and seven CRC-16 (poly 0x1021, start 0) against their check
// words.  by[] is 128 bytes of LDS.  The record goes to q[idx]; idx is reserved here.
__device__ __forceinline__ void drop_complete_frame(const uint8_t *fb, int nraw, uint8_t *by, DropFrame *q, int *q_count, int q_cap, int c,
                                                    unsigned long long t_hdr, int complete, int lane) {
    __syncthreads();
    for (int j = lane; j < DROP_FRAME_LEN; j += 64) {
        int v = 0;
        for (int i = 1; i < 9; i++) {
            const int p = 2 * (10 * j + i);
            const int b0 = p < nraw ? fb[p] : 0, b1 = p + 1 < nraw ? fb[p + 1] : 0;
            if (b0 == 0 && b1 == 1) v |= 1 << (i - 1);
        }
        by[j] = (uint8_t)v;
    }
    __syncthreads();
    bool bad = false;
    if (lane < 12) {
        const int p0 = DROP_BLK[lane][0], len = DROP_BLK[lane][1];
        unsigned chk;
        if (lane < 5) {
            unsigned s1 = 0, s2 = 0;
            for (int i = 0; i < len; i++) { s1 = (s1 + by[p0 + i]) & 0xFF; s2 = (s2 + s1) & 0xFF; }
            chk = s2 | (s1 << 8);
        } else {
            unsigned rem = 0;
            for (int i = 0; i < len; i++) {
                rem ^= (unsigned)by[p0 + i] << 8;
                for (int j = 0; j < 8; j++) rem = ((rem & 0x8000) ? (rem << 1) ^ 0x1021 : rem << 1) & 0xFFFF;
            }
            chk = rem;
        }
        bad = chk != (((unsigned)by[p0 + len] << 8) | by[p0 + len + 1]);
    }
    const unsigned long long m = __ballot(bad);
    const int err94 = (int)(m & 0x1F), err41 = (int)((m >> 5) & 0x7F);
    int idx = 0;
    if (lane == 0) idx = atomicAdd(q_count, 1);
    idx = __builtin_amdgcn_readfirstlane(__shfl(idx, 0));
    if (idx < q_cap) {                                     // a full queue drops the frame; the host sees the count and reports it
        DropFrame *f = q + idx;
        if (lane == 0) { f->channel = c; f->nraw = nraw; f->complete = complete; f->err94 = err94; f->err41 = err41; f->pad = 0; f->sample = t_hdr; }
        for (int j = lane; j < DROP_FRAME_LEN; j += 64) f->bytes[j] = by[j];
    }
    __syncthreads();
}
#endif
#endif
