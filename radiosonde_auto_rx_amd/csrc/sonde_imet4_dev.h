// sonde_imet4_dev.h — what the host engine (sonde_imet4.cpp) and k_imet4_afsk (sonde_imet4.hip) share.
#ifndef SONDE_IMET4_DEV_H
#define SONDE_IMET4_DEV_H
#include <hip/hip_runtime.h>
#include <cstdint>

#define IMET4_FRAME_BITS 1000
#define IMET4_FRAME_STRIDE 1024
#define IMET4_HEADER_PAT 0x3FFFFD01u   // "1111111111111111111" "10" "10000000" "1", newest character in bit 0

// per-channel state between calls (the reference's dsp_t / IQdc / slicer locals that outlive a sample)
struct Imet4Chan {
    double Df, dc, sumx, sumy, f0;
    double F1r, F1i, F2r, F2i, pos_bit;
    unsigned long long sample_hi, base;     // base: base-rate samples taken by the decimator
    float xsum, avgx, avgy, prevr, previ;
    uint32_t sample, pre_pos, cnt, maxcnt, maxlim, hreg;
    int32_t lut_len, locked, bit0, pos, hf, bitpos, hcount, bb0, bb1, bb2;
};

struct Imet4Frame {
    int32_t channel, nbits;
    uint64_t sample;
    uint8_t bits[IMET4_FRAME_BITS];
};

struct Imet4Args {
    Imet4Chan *chan;
    float2 *zring;
    float *fmring, *xring, *bufs;
    uint8_t *frames;                   // per channel: the bit frame in progress (IMET4_FRAME_STRIDE bytes)
    const float *ws_iq0, *ws_iq1, *ws_fm, *ws_dec;   // duplicated tap tables (2 T entries)
    float2 *bring, *ifbuf;             // decM > 1: base-rate ring (bring_len per channel), IF samples (if_stride per channel)
    const void *in;
    Imet4Frame *q;
    int *q_count;
    int q_cap, n_ch, n, iq, bits, dc, lp_iq, lp_fm, taps_iq, taps_fm, sr, M;   // n: IF samples per channel of the call; bits: 8, 16, 32 (float32)
    int ring, pre, decM, taps_dec, bring_len, if_stride;   // ring: history ring length (power of 2); pre: IF input from k_imet4_decim
    double bitlen, w1, w2;
    float head_sps;
    // behind the fields above, whose offsets the 8- / 16-bit instantiation's code depends on
    long long ch_stride;               // input samples (complex ones for IQ) between the starts of two channels' rows
    int *active;                       // per channel: 0 = released (its workgroups return at once and touch nothing)
    int rt;                            // per call, by the host: launch the instantiation with the mask, the row stride and the float loads
};

extern "C" int sonde_launch_imet4(const Imet4Args *a, hipStream_t s);
// channel c becomes what sonde_imet4_create builds for a channel whose record is `fresh`: rings, AFC buffer, IF row and frame bits as at
// create, active[c] = 1.  One small kernel on s, in order with the process calls around it.
extern "C" int sonde_launch_imet4_restart(const Imet4Args *a, int c, const Imet4Chan *fresh, hipStream_t s);
#endif
