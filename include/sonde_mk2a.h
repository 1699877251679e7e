/*
 * sonde_mk2a.h — LMS6-1680 / Sippican MkIIa (9616 Bd 8N1 on +/- 50 kHz FSK, L band) of libsonde_hip.so: the reference's mk2a/mk2a1680mod.c.
 *
 * Two parts:
 *  - the engine (GPU): per channel the reference's L-band front end (IQ-dc removal, LUT mixer, decimator; --dc rotation, IF low-pass with
 *    the acquisition / nominal tap sets, FM discriminator, the --IQ tone correlator, FM / IQFM low-pass on every decFM-th sample;
 *    mk2a1680mod.c:785-948, 1141-1442), the header search with its 8192-point transform and the AFC it drives (:331-480, 1505-1560),
 *    headcmp, the bit slicer and findsync (:992-1108, 1727, 2366-2430).  It hands out the hard bits of finished frames with mv, mv_pos,
 *    Df and the polarity in effect; many channels per call.
 *  - the printer (host only, no GPU): bits -> 8N1 bytes -> CRC -> subframes 4D / 54 -> text, -r, -v/-vv/-vvv, JSON (:1742-2071),
 *    byte-identical to the reference's stdout.
 *
 * Not built (SONDE_E_ARG): FM-audio input, --iq0, float32 samples, --noLUT, rates whose header window does not fit the 8192-point transform
 * or whose filters do not fit the history rings.
 */
#ifndef SONDE_MK2A_H
#define SONDE_MK2A_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SONDE_MK2A_MAX_BITS 1760         /* BITFRAME_LEN: a frame ends at CA CA CA CA or here, mk2a1680mod.c:2394 */

typedef struct {
    int32_t sample_rate;     /* input rate (Hz)                                                                              */
    int32_t bits;            /* 8 (unsigned) or 16 (signed) per sample component                                             */
    int32_t opt_iq;          /* 6: --iq fq (discriminator), 5: --IQ fq (tone correlator)                                     */
    int32_t lp_iq;           /* --lpIQ / --lpbw: IF low-pass                                                                 */
    int32_t lpbw_hz;         /* IF low-pass bandwidth; <= 0: the reference's default (180 kHz)                               */
    int32_t lp_fm;           /* --lpFM                                                                                       */
    int32_t dec_fm;          /* --decFM: 4, --decFM2: 2, --decFM1: 1, none: 0                                                */
    int32_t dc;              /* --dc: AFC                                                                                    */
    int32_t min;             /* --min: 4 x 32 kHz designated IF rate                                                         */
    int32_t invert;          /* -i                                                                                           */
    int32_t shift;           /* -d <shift>, -4 .. 4                                                                          */
    float   thres;           /* --ths; <= 0: 0.7                                                                             */
    float   baud;            /* --br (9400 .. 9800); <= 0: 9616                                                              */
    int32_t reserved[7];
} sonde_mk2a_cfg_t;

typedef struct {
    int32_t if_rate, dec_m, dec_fm;      /* "IF:", "dec:" of the reference's stderr; the FM decimation in effect             */
    int32_t L, M, K, N;                  /* header samples, ring length, window length, transform size                       */
    int32_t taps_dec, taps_iq, taps_fm, taps_iqfm;
    float   sps;                         /* samples per bit of the sliced stream                                             */
    int32_t reserved[8];
} sonde_mk2a_info_t;

typedef struct {
    int32_t  channel;
    int32_t  nbits;                            /* <= SONDE_MK2A_MAX_BITS; the first 20 are the `24 52` of the header         */
    int32_t  inv;                              /* polarity option in effect                                                  */
    float    mv;                               /* correlation score of the header                                            */
    double   df;                               /* AFC offset (Hz) when the frame ended                                       */
    uint32_t mv_pos;
    uint32_t reserved;
    uint64_t sample;                           /* output-rate sample count at the end of the frame                           */
    uint8_t  bits[SONDE_MK2A_MAX_BITS];
} sonde_mk2a_frame_t;

typedef struct sonde_mk2a sonde_mk2a_t;

/* fq[c] = --iq / --IQ fq of channel c; max_chunk = most input samples per channel in one process call (rounded down to a multiple of the
 * decimation).  init_buffers_Lband (mk2a1680mod.c:1141-1442) and the option handling of main (:2285-2343). */
int  sonde_mk2a_create(const sonde_mk2a_cfg_t *cfg, int32_t n_channels, const double *fq, int32_t max_chunk, sonde_mk2a_t **out);
void sonde_mk2a_destroy(sonde_mk2a_t *e);
int  sonde_mk2a_info(const sonde_mk2a_t *e, sonde_mk2a_info_t *info);
/* the same numbers from the configuration alone (host code, no GPU) */
int  sonde_mk2a_design(const sonde_mk2a_cfg_t *cfg, sonde_mk2a_info_t *info);
/* n input samples per channel (a multiple of the decimation, SONDE_E_RANGE otherwise), channel-major IQ: channel c's samples start at
 * c * n * 2.  f32buf_sample / find_header / the frame loop of main (:785-948, 1505-1560, 2370-2430).
 * SONDE_E_OVERFLOW: the frame queue of this call overflowed (frames lost; reported once). */
int  sonde_mk2a_process_host(sonde_mk2a_t *e, const void *samples, int32_t n);
int  sonde_mk2a_process_device(sonde_mk2a_t *e, const void *dev_samples, int32_t n);
/* end of the input: a frame in progress is handed out with the bits it has (main prints it after EOF, :2409-2424) */
int  sonde_mk2a_finish(sonde_mk2a_t *e);
/* completed frames in channel / time order; returns their number (<= max) or a SONDE_E_* code.  Frames not fetched stay queued. */
int  sonde_mk2a_fetch_frames(sonde_mk2a_t *e, sonde_mk2a_frame_t *out, int32_t max);

/* ------------------------------------------------------------------ testing taps (host code; not part of the decoding interface)
 * Read-only views of what the kernels left in device memory, for tests that compare every sample with a reference.  Each call waits for the
 * engine's stream and copies from the device; nothing the kernels compute depends on them. */
#define SONDE_MK2A_TAP_IF     0   /* cf32: IF samples of the last process call (behind IQ-dc removal, mixer and decimator)        */
#define SONDE_MK2A_TAP_ZROT   1   /* cf32: behind the AFC rotation                                                               */
#define SONDE_MK2A_TAP_ZLP    2   /* cf32: behind the IF low-pass (the reference's rot_iqbuf)                                    */
#define SONDE_MK2A_TAP_FMR    3   /* f32:  discriminator output per IF sample                                                    */
#define SONDE_MK2A_TAP_SRAW   4   /* f32:  tone correlator output per IF sample (--IQ only)                                      */
#define SONDE_MK2A_TAP_BUFS   5   /* f32:  dsp->bufs, output rate (IF rate / dec_fm), ring of 8192                               */
#define SONDE_MK2A_TAP_FMBUF  6   /* f32:  dsp->fm_buffer, output rate, ring of 8192                                             */

typedef struct {                         /* one channel's state between calls, as the kernels keep it                            */
    double   df, ddf, dc;                /* AFC offset (Hz), its last step, the header's dc                                      */
    double   sum_x, sum_y, f0;           /* IQ-dc block sums; mixer frequency (cycles per input sample)                          */
    uint64_t base;                       /* input samples taken                                                                  */
    uint64_t if_samples, out_samples;    /* IF samples through the front end; output samples written (sample_in)                 */
    uint64_t n_start, n_hdr;             /* sample_in when the header search last restarted / at the header of the frame         */
    float    avg_x, avg_y, mv;           /* IQ-dc average in effect; last correlation score                                      */
    uint32_t cnt, maxcnt, maxlim, mv_pos;/* IQ-dc block position, length, limit; position of the last correlation peak           */
    int32_t  lut_len, locked, mode, inv, buffered0, bitpos;   /* mode 0: searching, 1: in a frame                                */
} sonde_mk2a_state_t;

/* copy `count` samples of one channel's tap starting at absolute sample index `first` (IF-rate index for taps 0-4, output-rate index for
 * 5 and 6); they must still be inside the ring (SONDE_MK2A_TAP_IF: inside the last call), SONDE_E_RANGE otherwise.
 * out: count floats (x2 for the cf32 taps).  Returns count. */
int  sonde_mk2a_read_tap(sonde_mk2a_t *e, int32_t channel, int32_t tap, int64_t first, int32_t count, float *out);
int  sonde_mk2a_read_state(sonde_mk2a_t *e, int32_t channel, sonde_mk2a_state_t *out);

/* ------------------------------------------------------------------ printer (host code) */
typedef struct sonde_mk2a_printer sonde_mk2a_printer_t;

typedef struct {
    int32_t raw;             /* -r                                                                                           */
    int32_t crc;             /* --crc                                                                                        */
    int32_t vbs;             /* -v: 1, -vv: 2, -vvv: 3                                                                       */
    int32_t json;            /* --json (implies crc and vbs >= 1)                                                            */
    int32_t jsn_freq_khz;    /* "freq" of the JSON when > 0                                                                  */
    int32_t show_df;         /* --dc on IQ input: -vv prints Df                                                              */
    int32_t if_rate, sample_rate;   /* for the IF= / IQ= fractions of -vvv                                                   */
    char    version[32];     /* "version" of the JSON; "" = omit                                                             */
    int32_t reserved[4];
} sonde_mk2a_opts_t;

int  sonde_mk2a_printer_create(const sonde_mk2a_opts_t *opts, sonde_mk2a_printer_t **out);
void sonde_mk2a_printer_destroy(sonde_mk2a_printer_t *p);
/* print_frame (mk2a1680mod.c:1950-2071) on nbits frame bits: writes what the reference prints NUL-terminated into out; returns its
 * length or a negative SONDE_E_* code */
int  sonde_mk2a_print_frame(sonde_mk2a_printer_t *p, const uint8_t *bits, int32_t nbits, float mv, double df, char *out, size_t outlen);
/* CRC-16, polynomial 0x1021, initial value 0 (crc16_0, :1773-1792) */
int  sonde_mk2a_crc16(const uint8_t *bytes, int32_t len);

#ifdef __cplusplus
}
#endif
#endif
