/*
 * sonde_imet4.h — iMet-4 / iMet-1-RS (Bell 202 AFSK, 1200 Bd 8N1 on FM) of libsonde_hip.so: the reference's imet/imet4iq.c.
 *
 * Two parts:
 *  - the engine (GPU): per channel the reference's front end (IQ: IQ-dc removal, LUT mixer, --dc rotation, IF low-pass with the
 *    acquisition / nominal tap sets, FM discriminator, FM low-pass; FM audio: the sample, --dc subtraction), the once-per-second AFC,
 *    the two-tone sliding DFT and the run-length / majority slicer (imet4iq.c:445-578, 1532-1640).  It hands out complete 1000-bit
 *    frames; many channels per call.
 *  - the printer (host only, no GPU): bits -> 8N1 bytes -> GPS / eGPS / PTU / ePTU / XDATA packets -> text, -r, --rawbits, JSON
 *    (imet4iq.c:873-1315), byte-identical to the reference's stdout.
 *
 * Input above the IF rate the reference picks (48 / 32 / 96 / 64 kHz) goes through its decimating front end (decM > 1: IQ-dc removal and
 * the mixer table at the input rate, the decimator low-pass, k_imet4_decim) first.  Samples are 8-bit unsigned, 16-bit signed or float32, as the
 * reference reads them.  Not built (SONDE_E_ARG): --decFM, --noLUT, rates whose filters do not fit the history rings (far above any sonde
 * channel).
 *
 * An engine's channels can be handed out at run time (a receiver behind a channelizer): sonde_imet4_release_channel takes a channel out of
 * the launches, sonde_imet4_restart_channel makes it a fresh channel at a new --iq fq, sonde_imet4_process_device_strided reads rows of a
 * staging array whose stride is not the call's length.
 */
#ifndef SONDE_IMET4_H
#define SONDE_IMET4_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SONDE_IMET4_FRAME_BITS 1000      /* LEN_BITFRAME - 200: the frame is printed at this bit count, imet4iq.c:1586 */

typedef struct {
    int32_t sample_rate;     /* input rate (Hz)                                                                             */
    int32_t bits;            /* per sample component: 8 (unsigned), 16 (signed) or 32 (float32, little-endian, taken as it is)   */
    int32_t iq;              /* 1: complex IQ (--iq fq), 0: FM audio (mono)                                                 */
    int32_t lp_iq;           /* --lpIQ / --lpbw: IF low-pass                                                                */
    int32_t lpbw_hz;         /* IF low-pass bandwidth; <= 0: the reference's default (16 kHz, 80 kHz with imet1)            */
    int32_t lp_fm;           /* --lpFM: 6 kHz FM low-pass                                                                   */
    int32_t dc;              /* --dc: AFC                                                                                   */
    int32_t min;             /* --min: 32 kHz designated IF rate                                                            */
    int32_t imet1;           /* --imet1: 96 kHz designated IF rate, 80 kHz IF low-pass                                      */
    int32_t reserved[7];
} sonde_imet4_cfg_t;

typedef struct {
    int32_t  channel;
    int32_t  nbits;                            /* SONDE_IMET4_FRAME_BITS                                                    */
    uint64_t sample;                           /* IF-rate sample index of the frame's last bit decision                     */
    uint8_t  bits[SONDE_IMET4_FRAME_BITS];     /* 0 / 1; the first ten are the SOH character of the header                  */
} sonde_imet4_frame_t;

typedef struct sonde_imet4 sonde_imet4_t;

/* fq[c] = --iq fq of channel c (ignored for FM audio); max_chunk = most input samples per channel in one process call (rounded down to a
 * multiple of the decimation).
 * Writes the IF rate and decimation the reference reports ("IF:", "dec:") to *if_rate / *dec_m when not NULL. */
int  sonde_imet4_create(const sonde_imet4_cfg_t *cfg, int32_t n_channels, const double *fq, int32_t max_chunk,
                        sonde_imet4_t **out, int32_t *if_rate, int32_t *dec_m);
void sonde_imet4_destroy(sonde_imet4_t *e);
/* n input samples per channel (a multiple of the decimation, SONDE_E_RANGE otherwise), channel-major: channel c's samples (IQ interleaved
 * for iq = 1) start at c * n * (iq ? 2 : 1).  SONDE_E_OVERFLOW: the frame queue of this call overflowed (frames lost; reported once). */
int  sonde_imet4_process_host(sonde_imet4_t *e, const void *samples, int32_t n);
int  sonde_imet4_process_device(sonde_imet4_t *e, const void *dev_samples, int32_t n);
/* the same with channel c's samples starting at c * ch_stride samples (complex samples for iq = 1) instead of c * n: rows of a staging
 * array of which the first n entries are valid.  ch_stride >= n, SONDE_E_ARG otherwise; n as for process_device.  float32 IQ input of
 * either entry is 8-byte aligned.  A refused call leaves all state alone. */
int  sonde_imet4_process_device_strided(sonde_imet4_t *e, const void *dev_samples, int64_t ch_stride, int32_t n);
/* completed frames in channel / time order; returns their number (<= max) or a SONDE_E_* code.  Frames not fetched stay queued.
 * There is no finish / flush: a frame still in progress at the end of the input is never printed by the reference (imet4iq.c:1638), so
 * nothing is handed out for it. */
int  sonde_imet4_fetch_frames(sonde_imet4_t *e, sonde_imet4_frame_t *out, int32_t max);

/* ------------------------------------------------------------------ channels at run time
 * After create every channel is active.  A released channel costs a launch nothing: its workgroups return before they read their input
 * (which may be uninitialised memory) and write nothing — no state, no history, no frame.  Both calls are queued on the engine's stream
 * between two process calls and do not wait for the device; SONDE_E_ARG for a channel out of range, and then nothing has changed.
 *
 * restart: from the next process call on the channel is what sonde_imet4_create builds for a channel at --iq fq (fq is ignored for FM
 * audio): state, filter history and the frame in progress are as at create, frame.sample counts from the restart, and the channel is
 * active.  No other channel is touched.
 * release: the channel is inactive from the next process call on.  Frames already completed stay queued for sonde_imet4_fetch_frames.  The
 * frame in progress is dropped: the reference never prints a frame that the end of its input cuts short (imet4iq.c:1638). */
int  sonde_imet4_restart_channel(sonde_imet4_t *e, int32_t channel, double fq);
int  sonde_imet4_release_channel(sonde_imet4_t *e, int32_t channel);
/* 1: active, 0: released */
int  sonde_imet4_channel_active(const sonde_imet4_t *e, int32_t channel);

/* ------------------------------------------------------------------ testing taps (host code; not part of the decoding interface)
 * Read-only views of what the kernels left in device memory, for tests that compare every sample with a reference.  Each call waits for the
 * engine's stream and copies from the device; nothing the kernels compute depends on them. */
#define SONDE_IMET4_TAP_IF      0   /* cf32: IF samples of the last process call (behind IQ-dc removal, mixer and decimator); decimation > 1 */
#define SONDE_IMET4_TAP_ZRING   1   /* cf32: the sample the IF low-pass takes in (behind the AFC rotation); with the IF low-pass only         */
#define SONDE_IMET4_TAP_FMRING  2   /* f32:  the sample the FM low-pass takes in (discriminator output or FM audio); with lp_fm only          */
#define SONDE_IMET4_TAP_XRING   3   /* f32:  the front-end sample the sliding two-tone DFT takes (the reference's f32_sample output)          */

typedef struct {                         /* one channel's state between calls, as the kernels keep it                                        */
    double   df, dc, sum_x, sum_y, f0;   /* AFC offset (Hz), its last mean; IQ-dc block sums; mixer frequency (cycles per input sample)      */
    double   f1_re, f1_im, f2_re, f2_im; /* the sliding DFT sums of the 2200 Hz and 1200 Hz tones                                            */
    double   pos_bit;                    /* slicer: position of the last bit decision                                                        */
    uint64_t sample_hi, base;            /* upper part of the IF sample count; input samples taken by the decimator                         */
    float    xsum, avg_x, avg_y, prev_re, prev_im;   /* AFC running sum; IQ-dc average in effect; the last IF sample (discriminator)         */
    uint32_t sample, pre_pos, cnt, maxcnt, maxlim, hreg;   /* IF samples done (low 32 bits); AFC phase; IQ-dc block position / length / limit */
    int32_t  lut_len, locked, bit0, pos, hf, bitpos, hcount, bb0, bb1, bb2;   /* mixer table length; tap set; slicer                         */
} sonde_imet4_state_t;

/* copy `count` samples of one channel's tap starting at absolute IF sample index `first`; they must still be inside the history ring, which
 * keeps the last (ring - 64) samples (SONDE_IMET4_TAP_IF: inside the last call), SONDE_E_RANGE otherwise; SONDE_E_ARG for a tap the
 * configuration does not have.  out: count floats (x2 for the cf32 taps).  Returns count. */
int  sonde_imet4_read_tap(sonde_imet4_t *e, int32_t channel, int32_t tap, int64_t first, int32_t count, float *out);
int  sonde_imet4_read_state(sonde_imet4_t *e, int32_t channel, sonde_imet4_state_t *out);
/* length of the history rings behind taps 1-3 (a power of two) */
int  sonde_imet4_tap_ring(sonde_imet4_t *e);

/* ------------------------------------------------------------------ printer (host code) */
typedef struct sonde_imet4_printer sonde_imet4_printer_t;

typedef struct {
    int32_t raw;             /* -r                                                                                          */
    int32_t rawbits;         /* --rawbits                                                                                   */
    int32_t json;            /* --json                                                                                      */
    int32_t jsn_freq_khz;    /* "freq" of the JSON when > 0                                                                 */
    char    version[32];     /* "version" of the JSON; "" = omit                                                            */
    int32_t reserved[4];
} sonde_imet4_opts_t;

int  sonde_imet4_printer_create(const sonde_imet4_opts_t *opts, sonde_imet4_printer_t **out);
void sonde_imet4_printer_destroy(sonde_imet4_printer_t *p);
/* one frame of nbits bits (print_frame(dsp, nbits / 10)): writes what the reference prints NUL-terminated into out; returns its length
 * or a negative SONDE_E_* code */
int  sonde_imet4_print_frame(sonde_imet4_printer_t *p, const uint8_t *bits, int32_t nbits, char *out, size_t outlen);
/* CRC-16 of the packets (CCITT polynomial, initial value 0x1D0F) */
int  sonde_imet4_crc16(const uint8_t *bytes, int32_t len);

#ifdef __cplusplus
}
#endif
#endif
