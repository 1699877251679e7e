/*
 * sonde_wxr.h — Weathex WxR-301D (2-FSK, 64 kHz wide; 4800 Bd, or 5000 Bd with PN9 whitening) of libsonde_hip.so: the reference's
 * weathex/weathex301d.c, and in IQ form the `iq_dec --FM --IFbw k --lpFM --iq fq` that auto_rx runs in front of it.
 *
 * Three parts:
 *  - the engine (GPU): per channel the FM stream — in IQ form made on the device by the iq_dec front end (IQ-dc removal, table mixer,
 *    decimator, discriminator, FM low-pass; demod/mod/iq_dec.c:550-760), in FM form supplied by the caller — and the reference's bit
 *    slicer on it: runs between sign changes, the 40-bit header ring, and with -b the integrate-and-dump bits behind a header
 *    (weathex301d.c:171-226, 649-707).  It hands out the 552 bit values of finished frames; many channels per call.
 *  - the printer (host only, no GPU): bits -> bytes -> PN9 -> check -> text, -r, -R, JSON (print_frame, :359-527), byte-identical to
 *    the reference's stdout, with the pairing of frame ids 1 and 2 that persists between frames.
 *  - the soft-bit framer: the --softin loop of main (:607-648).  For one stream it is host code (sonde_wxr_softin_push, what host/weathex301d --softin
 *    runs); for a batch of channels behind the GPU modem it runs on the device (sonde_softin_dev_create_wxr, include/sonde_fsk.h), which also does bytes, PN9 and
 *    the check, and sonde_wxr_print_decoded prints from its records.
 *
 * Not built (SONDE_E_ARG): float32 IQ input, rates with fewer than 2 or more than 4096 samples per bit.
 */
#ifndef SONDE_WXR_H
#define SONDE_WXR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SONDE_WXR_BITS 552               /* BITFRAMELEN = 8 * 69 */
#define SONDE_WXR_BIT_UNSET 2            /* a bit the slicer has never written (the reference's frame_bits starts as NUL bytes) */

#define SONDE_WXR_IN_IQ 0                /* baseband IQ, 8 (unsigned) or 16 (signed) bits per component                             */
#define SONDE_WXR_IN_FM 1                /* FM samples: one real sample per frame, 8 (unsigned) / 16 (signed) / 32 (float) bits      */

typedef struct {
    int32_t sample_rate;     /* input rate (Hz)                                                                              */
    int32_t input;           /* SONDE_WXR_IN_IQ / SONDE_WXR_IN_FM                                                            */
    int32_t bits;            /* per sample (component)                                                                       */
    int32_t pn9;             /* --pn9: 5000 Bd, header AA AA AA C1 94                                                        */
    int32_t invert;          /* -i                                                                                           */
    int32_t opt_b;           /* -b: integrate-and-dump behind the header                                                     */
    int32_t if_bw_khz;       /* IQ form: iq_dec --IFbw (>= 32; <= 0: 48)                                                     */
    float   baud;            /* <= 0: 4800 / 5000                                                                            */
    int32_t reserved[8];
} sonde_wxr_cfg_t;

typedef struct {
    int32_t if_rate, dec_m;              /* "IF:", "dec:" of iq_dec's stderr (FM form: the sample rate, 1)                    */
    int32_t taps_dec, taps_fm;           /* decimator and FM low-pass taps (0 in FM form)                                     */
    float   sps;                         /* "samples/bit:" of weathex301d's stderr                                            */
    int32_t reserved[7];
} sonde_wxr_info_t;

typedef struct {
    int32_t  channel;
    int32_t  nbits;                      /* 552, or what the stream reached when finish handed the frame out                  */
    int32_t  complete;                   /* 0: header open at the end of the input (the reference prints it only with -b)     */
    int32_t  reserved;
    uint64_t sample;                     /* samples read when the header matched (-t prints sample / rate)                    */
    uint8_t  bits[SONDE_WXR_BITS];       /* 0 / 1 / SONDE_WXR_BIT_UNSET; behind nbits what the previous frame left there      */
} sonde_wxr_frame_t;

typedef struct sonde_wxr sonde_wxr_t;

/* fq[c] = --iq fq of channel c (IQ form; NULL in FM form); max_chunk = most input samples per channel in one process call (rounded
 * down to a multiple of the decimation). */
int  sonde_wxr_create(const sonde_wxr_cfg_t *cfg, int32_t n_channels, const double *fq, int32_t max_chunk, sonde_wxr_t **out);
void sonde_wxr_destroy(sonde_wxr_t *e);
int  sonde_wxr_info(const sonde_wxr_t *e, sonde_wxr_info_t *info);
/* the same numbers from the configuration alone (host code, no GPU) */
int  sonde_wxr_design(const sonde_wxr_cfg_t *cfg, sonde_wxr_info_t *info);
/* n input samples per channel (IQ form: a multiple of the decimation, SONDE_E_RANGE otherwise), channel-major: channel c's samples start
 * at sample c * n.  SONDE_E_OVERFLOW: the frame queue of this call overflowed (frames lost; reported once). */
int  sonde_wxr_process_host(sonde_wxr_t *e, const void *samples, int32_t n);
int  sonde_wxr_process_device(sonde_wxr_t *e, const void *dev_samples, int32_t n);
/* end of the input: a frame whose header is open is handed out with complete = 0 (main after EOF, :692-704) */
int  sonde_wxr_finish(sonde_wxr_t *e);
/* frames in channel / time order; returns their number (<= max) or a SONDE_E_* code.  Frames not fetched stay queued. */
int  sonde_wxr_fetch_frames(sonde_wxr_t *e, sonde_wxr_frame_t *out, int32_t max);

/* ------------------------------------------------------------------ printer (host code) */
typedef struct sonde_wxr_printer sonde_wxr_printer_t;

typedef struct {
    int32_t raw;             /* -r: 1, -R: 2                                                                                 */
    int32_t vbs;             /* -v                                                                                           */
    int32_t json;            /* --json                                                                                       */
    int32_t pn9;             /* --pn9                                                                                        */
    int32_t jsn_freq_khz;    /* "freq" of the JSON when > 0                                                                  */
    char    version[32];     /* "version" of the JSON; "" = omit                                                             */
    int32_t ts;              /* -t, sonde_wxr_print_decoded only: "<%8.3f> " of hdr_bit / 4800 (--pn9: 5000) in front of the frame's text  */
    int32_t reserved[3];
} sonde_wxr_opts_t;

int  sonde_wxr_printer_create(const sonde_wxr_opts_t *opts, sonde_wxr_printer_t **out);
void sonde_wxr_printer_destroy(sonde_wxr_printer_t *p);
/* print_frame (weathex301d.c:359-527) on the 552 bit values of a frame: writes what the reference prints into out (NUL-terminated; -R of
 * an unset bit puts a NUL inside, so take the length from the return value); returns the length or a negative SONDE_E_* code */
int  sonde_wxr_print_frame(sonde_wxr_printer_t *p, const uint8_t *bits, char *out, size_t outlen);
/* print_frame on a record of the device soft-bit consumer (sonde_softin_dev_fetch_wxr, include/sonde_fsk.h): the same text, -r, -R, -v, JSON and pairing of frame
 * ids 1 and 2, with the -t prefix of the --softin loop in front (opts.ts), from the record's bytes (x; -R: raw), check values, verdict, frame id, serial and
 * counter as the device left them — nothing is recomputed.  Returns the length or a negative SONDE_E_* code */
typedef struct sonde_wxr_softin_rec sonde_wxr_softin_rec_t;      /* the struct is defined in include/sonde_fsk.h */
int  sonde_wxr_print_decoded(sonde_wxr_printer_t *p, const sonde_wxr_softin_rec_t *rec, char *out, size_t outlen);
/* (xor8 << 8) | sum8 (xor8sum, :318-330) */
int  sonde_wxr_xor8sum(const uint8_t *bytes, int32_t len);

/* ------------------------------------------------------------------ soft-bit framer for one stream (host code; many channels: sonde_softin_dev_create_wxr) */
typedef struct sonde_wxr_softin sonde_wxr_softin_t;

int  sonde_wxr_softin_create(int32_t pn9, int32_t invert, sonde_wxr_softin_t **out);
void sonde_wxr_softin_destroy(sonde_wxr_softin_t *s);
/* n float32 soft bits (one per bit); completed frames into out (at most max; the rest stay queued for the next call, which may pass
 * n = 0).  frame.sample = bits read when the header matched.  Returns the number of frames written. */
int  sonde_wxr_softin_push(sonde_wxr_softin_t *s, const float *soft, int32_t n, sonde_wxr_frame_t *out, int32_t max);
/* end of the input: 1 and the open header's frame (complete = 0) in out if a header is open, else 0 */
int  sonde_wxr_softin_finish(sonde_wxr_softin_t *s, sonde_wxr_frame_t *out);

#ifdef __cplusplus
}
#endif
#endif
