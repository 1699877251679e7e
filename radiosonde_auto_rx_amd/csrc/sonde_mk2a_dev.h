// sonde_mk2a_dev.h — what the host engine (sonde_mk2a.cpp) and the kernels k_mk2a_mix / k_mk2a (sonde_mk2a.hip) share.
#ifndef SONDE_MK2A_DEV_H
#define SONDE_MK2A_DEV_H
#include <hip/hip_runtime.h>
#include <cstdint>

#define MK2A_THREADS 512
#define MK2A_M 8192                 // bufs / fm_buffer ring and N_DFT (mk2a1680mod.c:1337-1341); other sizes are refused at create
#define MK2A_MAX_BITS 1760          // BITFRAME_LEN
#define MK2A_FRAME_STRIDE 1792
#define MK2A_FRMSTART 20
#define MK2A_HDRLEN 50
#define MK2A_TILE 2048              // IF samples the front end produces per pass of its phases
#define MK2A_LP_IQ 1
#define MK2A_LP_FM 2
#define MK2A_LP_IQFM 4

// per-channel state between calls (the reference's dsp_t / IQdc / main() locals that outlive a sample)
struct Mk2aChan {
    double Df, dDf, dc, sumx, sumy, f0;
    unsigned long long base;           // base-rate samples taken by k_mk2a_mix
    unsigned long long U;              // IF samples through the front end (_sample)
    unsigned long long N;              // output samples written (sample_in)
    unsigned long long n_start;        // sample_in when the running find_header last set k = 0
    unsigned long long n_hdr;          // sample_in at the header of the frame in progress
    float avgx, avgy, mv;
    uint32_t cnt, maxcnt, maxlim, mv_pos;
    int32_t lut_len, locked, mode, inv, buffered0, bitpos;
};

struct Mk2aFrame {
    int32_t channel, nbits, inv;
    float mv;
    double Df;
    uint32_t mv_pos, pad;
    uint64_t sample;
    uint8_t bits[MK2A_MAX_BITS];
};

struct Mk2aTone { int n; int pad; double e1r, e1i, e2r, e2i; };

struct Mk2aArgs {
    Mk2aChan *chan;
    const void *in;
    float2 *bring, *ifbuf;             // base-rate ring (decM > 1), IF samples of the call (if_stride per channel)
    float2 *zrot, *zlp;                // IF-rate rings by absolute sample: behind the AFC rotation, behind the IF low-pass (rot_iqbuf)
    float *fmr, *sraw;                 // discriminator output, tone-correlator output (--IQ)
    float *bufs, *fmbuf;               // dsp->bufs, dsp->fm_buffer (MK2A_M each)
    float2 *Xg;                        // [n_ch][MK2A_M] the window's spectrum while its correlation is transformed back
    const float2 *Fm, *tws;            // Fm: [2][MK2A_M] spectrum of the time-reversed header, natural and bit-reversed order
    const float *ws_iq0, *ws_iq1, *ws_fm, *ws_iqfm, *ws_dec;   // duplicated tap tables
    const Mk2aTone *tone;
    uint8_t *frames;
    Mk2aFrame *q;
    int *q_count;
    int q_cap, n_ch, n_base, n_if, bits, bring_len, if_stride, ring;
    int decM, taps_dec, taps_iq, taps_fm, taps_iqfm, n_tone;
    int opt_iq, lp, dc, decFM, sr, K, L, delay, bitofs, mp_ofs, slice_cap;
    float sps, thres, bl, tone_sps;
};

extern "C" int sonde_launch_mk2a(const Mk2aArgs *a, hipStream_t s);
#endif
