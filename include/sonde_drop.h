/*
 * sonde_drop.h — Vaisala RD94 / RD41 dropsondes (Manchester-coded 8N1 at 4800 raw bits/s, 120-byte frames, two a second) of
 * libsonde_hip.so: the reference's dropsonde/rd94rd41drop.c, and in IQ form the `iq_dec --FM --lpFM --wav --bo 16 --iq fq` in front of it.
 *
 * Three parts:
 *  - the engine (GPU): per channel the FM stream as 16-bit (or 8-bit) integers — in IQ form made on the device by the iq_dec front end
 *    and read through iq_dec's own 16-bit conversion, in FM form supplied by the caller — the reference's bit slicer on it (runs between
 *    sign changes, the 40-bit header ring, with -b integer integrate-and-dump behind a header; rd94rd41drop.c:207-271, 1399-1446), and the
 *    completion of a frame on the device: Manchester pairs -> 1200 bits -> 120 bytes, five chksum16 and seven CRC-16 checks.
 *  - the printer (host only, no GPU): print_frame (:1013-1251) with its type choice, text, -r, -R, -v, -vv and JSON, byte-identical to
 *    the reference's stdout, with the fields that persist from frame to frame.
 *  - the soft-bit framer (host only): the --softin / --softinv loop of main (:1357-1386), and the --rawhex line reader (:1450-1462).
 *
 * Channels at run time: an engine created with bits = 32 (float32 IQ at a rate at which iq_dec does not decimate, what a channelizer produces) has a front
 * end of its own on the device (k_fm_front: iq_dec.c f32read_cblock :337-382, the table mixer :674-711 / :571-573, the discriminator :593-596, re_lowpass
 * :599-604, every channel on a sample clock that starts at its restart) and hands its channels out while it runs: restart, release and finish of one channel.
 *
 * Not built (SONDE_E_ARG): float32 FM samples, float32 IQ at rates at which iq_dec decimates (96 000 Hz, 100 000 Hz, ...), rates with fewer than 2 or more
 * than 4096 samples per raw bit, the reference's unused option_res.
 */
#ifndef SONDE_DROP_H
#define SONDE_DROP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SONDE_DROP_FRAME_LEN 120         /* FRAME_LEN                                                                          */
#define SONDE_DROP_RAWBITS 2400          /* RAWBITFRAME_LEN = 120 bytes * 10 bits (8N1) * 2 (Manchester)                        */

#define SONDE_DROP_IN_IQ 0               /* baseband IQ, 8 (unsigned) or 16 (signed) bits per component, or float32             */
#define SONDE_DROP_IN_FM 1               /* FM samples: one real sample per frame, 8 (unsigned) or 16 (signed) bits             */

typedef struct {
    int32_t sample_rate;     /* input rate (Hz)                                                                              */
    int32_t input;           /* SONDE_DROP_IN_IQ / SONDE_DROP_IN_FM                                                          */
    int32_t bits;            /* per sample (component): 8 or 16; 32: float32 IQ taken as it is (iq_dec.c:361-364), IQ form at
                                dec_m = 1 only                                                                               */
    int32_t invert;          /* -i                                                                                           */
    int32_t opt_b;           /* -b: integrate-and-dump behind the header                                                     */
    float   baud;            /* --br (kept when within 4700..4900, else 4800); <= 0: 4800                                    */
    int32_t reserved[8];
} sonde_drop_cfg_t;

typedef struct {
    int32_t if_rate, dec_m;              /* "IF:", "dec:" of iq_dec's stderr (FM form: the sample rate, 1)                    */
    int32_t taps_dec, taps_fm;           /* decimator and FM low-pass taps (0 in FM form)                                     */
    float   sps;                         /* "samples/bit:" of rd94rd41drop's stderr, "corr:" with --br                        */
    int32_t reserved[7];
} sonde_drop_info_t;

typedef struct {
    int32_t  channel;
    int32_t  nraw;                       /* raw bits present: 2400, or what the stream reached when finish handed the frame out; the
                                            rest counts as '0' (print_bitframe, :1253)                                         */
    int32_t  complete;                   /* 0: header open at the end of the input (the reference prints it only with -b)     */
    int32_t  err94;                      /* geterr_rd94: bit i set = chksum16 block i fails (5 blocks)                        */
    int32_t  err41;                      /* geterr_rd41: bit i set = CRC-16 block i fails (7 blocks)                          */
    int32_t  reserved;
    uint64_t sample;                     /* samples (soft bits) read when the header matched                                  */
    uint8_t  bytes[SONDE_DROP_FRAME_LEN];
} sonde_drop_frame_t;

typedef struct sonde_drop sonde_drop_t;

/* fq[c] = --iq fq of channel c (IQ form; NULL in FM form); max_chunk = most input samples per channel in one process call (rounded
 * down to a multiple of the decimation). */
int  sonde_drop_create(const sonde_drop_cfg_t *cfg, int32_t n_channels, const double *fq, int32_t max_chunk, sonde_drop_t **out);
void sonde_drop_destroy(sonde_drop_t *e);
int  sonde_drop_info(const sonde_drop_t *e, sonde_drop_info_t *info);
/* the same numbers from the configuration alone (host code, no GPU) */
int  sonde_drop_design(const sonde_drop_cfg_t *cfg, sonde_drop_info_t *info);
/* n input samples per channel (IQ form: a multiple of the decimation, SONDE_E_RANGE otherwise), channel-major: channel c's samples start
 * at sample c * n.  SONDE_E_OVERFLOW: the frame queue of this call overflowed (frames lost; reported once). */
int  sonde_drop_process_host(sonde_drop_t *e, const void *samples, int32_t n);
int  sonde_drop_process_device(sonde_drop_t *e, const void *dev_samples, int32_t n);
/* end of the input: with -b a frame whose header is open is completed with '0' bits on the device and handed out with complete = 0
 * (main :1430-1445); without -b the reference prints nothing for it and nothing is handed out */
int  sonde_drop_finish(sonde_drop_t *e);
/* frames in channel / time order; returns their number (<= max) or a SONDE_E_* code.  Frames not fetched stay queued. */
int  sonde_drop_fetch_frames(sonde_drop_t *e, sonde_drop_frame_t *out, int32_t max);

/* ---- channels at run time: engines created with bits = 32 only (SONDE_E_ARG on every other engine, for a channel out of range, and for
 * fq outside -0.5 .. 0.5).  restart / release only enqueue on the engine's stream, in order with the process calls. */
/* process_device on rows ch_stride (>= n) samples apart: channel c's samples start at sample c * ch_stride.  The row of a released channel is not read. */
int  sonde_drop_process_device_strided(sonde_drop_t *e, const void *dev_samples, int64_t ch_stride, int32_t n);
/* from the next call on the channel is what create builds, at --iq fq, and active: the pipeline `iq_dec ... --iq fq - <rate> 32 | rd94rd41drop` started on
 * the channel's next sample.  Its sample clock starts here: the IQ-dc schedule of iq_dec.c:752-758, the mixer table's index (:533), z0 (:552), the FM
 * low-pass buffer (:747) and rd94rd41drop's sample_count, so sonde_drop_frame_t.sample counts from the restart. */
int  sonde_drop_restart_channel(sonde_drop_t *e, int32_t channel, double fq);
/* the channel takes no part in the calls that follow: nothing of it is read or written; a frame in progress is dropped */
int  sonde_drop_release_channel(sonde_drop_t *e, int32_t channel);
/* 1 / 0 */
int  sonde_drop_channel_active(const sonde_drop_t *e, int32_t channel);
/* the end of the input for one channel (main :1430-1445): with -b a frame whose header is open is completed with '0' bits and queued with complete = 0;
 * then the channel is released.  Nothing happens to a released channel. */
int  sonde_drop_finish_channel(sonde_drop_t *e, int32_t channel);
/* testing tap: count samples of the channel's FM stream from its sample `first` (counted from its restart; still inside the ring of at least max_chunk
 * samples, SONDE_E_RANGE otherwise) through iq_dec's 16-bit conversion (fwrite_fm_blk with --bo 16): what `iq_dec --FM --lpFM --wav --bo 16` writes.
 * Returns count.  A released channel has no stream: SONDE_E_ARG. */
int  sonde_drop_read_fm(sonde_drop_t *e, int32_t channel, int64_t first, int32_t count, int16_t *out);

/* ------------------------------------------------------------------ printer (host code) */
typedef struct sonde_drop_printer sonde_drop_printer_t;

typedef struct {
    int32_t raw;             /* -r: 1, -R: 2                                                                                 */
    int32_t vbs;             /* -v: 1, -vv: 2                                                                                */
    int32_t json;            /* --json                                                                                       */
    int32_t type;            /* --rd41: 41, --rd94: 94, 0: chosen per frame                                                  */
    int32_t jsn_freq_khz;    /* "freq" of the JSON when > 0                                                                  */
    char    version[32];     /* "version" of the JSON; "" = omit                                                             */
    int32_t reserved[4];
} sonde_drop_opts_t;

int  sonde_drop_printer_create(const sonde_drop_opts_t *opts, sonde_drop_printer_t **out);
void sonde_drop_printer_destroy(sonde_drop_printer_t *p);
/* print_frame (:1013-1251) on the 120 bytes of a frame: writes what the reference prints into out (NUL-terminated); returns the length
 * or a negative SONDE_E_* code */
int  sonde_drop_print_frame(sonde_drop_printer_t *p, const uint8_t *bytes, char *out, size_t outlen);
/* the type print_frame gave the last frame (41 / 94), and whether it printed that frame's JSON */
int  sonde_drop_printer_last(const sonde_drop_printer_t *p, int32_t *type, int32_t *json_printed);
uint32_t sonde_drop_chksum16(const uint8_t *bytes, int32_t len);
uint32_t sonde_drop_crc16(const uint8_t *bytes, int32_t len);
/* geterr_rd94 / geterr_rd41 on the 120 bytes of a frame */
int  sonde_drop_errs(const uint8_t *bytes, int32_t *err94, int32_t *err41);
/* one --rawhex line -> 120 bytes (:1451-1458); returns 1 when bytes 0-1 are FC 1D (the frame is printed), else 0 */
int  sonde_drop_rawhex(const char *line, uint8_t *bytes);

/* ------------------------------------------------------------------ soft-bit framer (host code) */
typedef struct sonde_drop_softin sonde_drop_softin_t;

/* invert = (--softinv) xor (-i): the two cancel each other */
int  sonde_drop_softin_create(int32_t invert, sonde_drop_softin_t **out);
void sonde_drop_softin_destroy(sonde_drop_softin_t *s);
/* n float32 soft bits (one per raw bit); completed frames into out (at most max; the rest stay queued for the next call, which may pass
 * n = 0).  frame.sample = soft bits read when the header matched.  Returns the number of frames written. */
int  sonde_drop_softin_push(sonde_drop_softin_t *s, const float *soft, int32_t n, sonde_drop_frame_t *out, int32_t max);
/* raw bits 0 / 1 (anything else counts as 'x') -> bytes and both masks of f, as print_bitframe does (host mirror of the device's
 * frame completion); bits behind nraw count as '0' */
int  sonde_drop_frame_from_rawbits(const uint8_t *rawbits, int32_t nraw, sonde_drop_frame_t *f);

#ifdef __cplusplus
}
#endif
#endif
