/*
 * sonde_fsk.h — C ABI of the batched 2-/4-FSK modem in libsonde_hip.so.
 *
 * Replaces the reference's utils/fsk.c demodulator (the codec2 "fsk_demod" auto_rx pipes IQ into,
 * auto_rx/autorx/decode.py:901,976,1067,1120) for many channels at once.  The reference seam is
 * fsk_create_hbr / fsk_set_freq_est_limits / fsk_set_freq_est_alg / fsk_nin / fsk_demod_sd / fsk_get_demod_stats /
 * fsk_destroy (utils/fsk.h:115-205) over struct FSK (fsk.h:47-95); every channel here is one such struct.
 * host/fsk_demod.c keeps the CLI (utils/fsk_demod.c) on top of it; host/seam/fsk_hip.c is the fsk.h function seam itself (the
 * reference's fsk_demod.c links against it unchanged).  Conventions as sonde_hip.h.
 */
#ifndef SONDE_FSK_H
#define SONDE_FSK_H

#include "sonde_hip.h"
#include "sonde_drop.h"
#include "sonde_lms6.h"
#include "sonde_rs92.h"
#include "sonde_gps.h"
#include "sonde_imet54.h"
#include "sonde_meisei.h"
#include "sonde_mrz.h"
#include "sonde_mts01.h"
#include "sonde_wxr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* input sample formats (fsk_demod.c:103-110,283-311) */
#define SONDE_FSK_S16   1       /* real int16,  x/1000           */
#define SONDE_FSK_CS16  2       /* --cs16: complex int16, x/1000 */
#define SONDE_FSK_CU8   3       /* --cu8: complex uint8, (u-127)/128 */
#define SONDE_FSK_CF32  4       /* complex float32 as is: the COMP fsk_in[] of fsk_demod() / fsk_demod_sd() (fsk.h:176,186) */

typedef struct sonde_fsk sonde_fsk_t;

typedef struct {
    int32_t abi_version;     /* SONDE_ABI_VERSION                                            */
    int32_t device;
    int32_t n_channels;
    int32_t Fs, Rs;          /* sample / symbol rate; Fs % Rs == 0 (fsk.c:127)               */
    int32_t M;               /* 2 or 4 tones (fsk.c:130); 4-FSK yields two soft bits per symbol */
    int32_t P;               /* -p: timing oversampling, (Fs/Rs) % P == 0 (fsk.c:129)        */
    int32_t nsym;            /* --nsym: symbols per modem frame                              */
    int32_t format;          /* SONDE_FSK_*                                                  */
    int32_t fsk_lower, fsk_upper;   /* -b / -u estimator limits in Hz (fsk_set_freq_est_limits) */
    int32_t mask;            /* --mask given: mask estimator (fsk_set_freq_est_alg)          */
    int32_t tone_spacing;    /* --mask <Hz> (tx_tone_separation, default 100)                */
    int32_t max_chunk;       /* largest n_samples per process call                           */
    int32_t burst_mode;      /* fsk_enable_burst_mode: nin never adjusted (fsk.c:724,976)    */
    int32_t raw_eye;         /* fsk_stats_normalise_eye(fsk, 0): eye traces not normalised   */
    int32_t reserved[2];
} sonde_fsk_cfg_t;

/* struct FSK constants (fsk_create_core, fsk.c:114-201) */
typedef struct {
    int32_t Ts, N, Ndft, Nmem, Nbits;
    float   tc;
    int32_t reserved[4];
} sonde_fsk_info_t;

/* per modem frame: what fsk_demod_core leaves in struct FSK / MODEM_STATS (fsk.c:593-915) */
typedef struct {
    int32_t nin;             /* samples this frame consumed                                  */
    int32_t nin_next;        /* fsk_nin() after the frame                                    */
    float   f_est[4];        /* tone estimates used by the demod (peak or mask estimator), M of them */
    float   norm_rx_timing;
    float   ppm;
    float   EbNodB;
    float   snr_est;         /* MODEM_STATS.snr_est (the "EbNodB" of the stats JSON)         */
} sonde_fsk_frame_t;

int  sonde_fsk_create(const sonde_fsk_cfg_t *cfg, sonde_fsk_t **out);     /* fsk_create_hbr + limits + estimator */
void sonde_fsk_destroy(sonde_fsk_t *f);                                   /* fsk_destroy                          */
int  sonde_fsk_info(const sonde_fsk_t *f, sonde_fsk_info_t *info);

/* Push n_samples per channel (channel c at in + c*ch_stride samples); runs every modem frame for which fsk_nin()
 * samples are available (the `while (fread(.., fsk_nin(fsk), ..))` loop of fsk_demod.c:279) — samples left over stay
 * queued.  Synchronous. */
int  sonde_fsk_process_host(sonde_fsk_t *f, const void *h_in, int64_t ch_stride, int32_t n_samples);
int  sonde_fsk_process_device(sonde_fsk_t *f, const void *d_in, int64_t ch_stride, int32_t n_samples);
/* sonde_fsk_process_device in two halves: submit enqueues everything on the engine's stream and returns, wait blocks until the launch is through.
 * Between the two the host is free: the other engines of a mixed batch can be submitted (their launches overlap on the GPU without a host thread
 * each).  Any other call of the engine waits first.  d_in is read by a copy that is only ENQUEUED when submit returns: it must stay untouched until
 * sonde_fsk_wait (or any other call of the engine) has returned. */
int  sonde_fsk_submit_device(sonde_fsk_t *f, const void *d_in, int64_t ch_stride, int32_t n_samples);
int  sonde_fsk_wait(sonde_fsk_t *f);

/* Channels fed independently (the resident broker, host/sonde_broker.c: every client reads exactly fsk_nin() samples of its own
 * stream per frame, and nin differs between channels): channel c gets n_samples[c] samples from h_in[c] (0 = nothing this time).
 * An engine is fed either this way or through sonde_fsk_process_host / _device, not both. */
int  sonde_fsk_process_host_var(sonde_fsk_t *f, const void *const *h_in, const int32_t *n_samples);
/* Back to the state fsk_create_hbr() leaves (oscillators, timing, Sf, nin = N) for one channel; samples queued for it are dropped.
 * The next samples fed to the channel are the first of a new stream. */
int  sonde_fsk_reset_channel(sonde_fsk_t *f, int32_t channel);

/* Soft decisions (fsk_demod_sd: one float per bit — 2-FSK: >0 = the lower tone; 4-FSK: two per symbol, fsk.c:793-802) produced by the last process call for one
 * channel; returns the number of floats written (<= max). frames (optional, may be NULL): per-frame records,
 * max_frames entries; *n_frames receives the count. */
int  sonde_fsk_fetch(sonde_fsk_t *f, int32_t channel, float *sd, int32_t max, sonde_fsk_frame_t *frames, int32_t max_frames,
                     int32_t *n_frames);
/* Hard decisions of the same frames (rx_bits of fsk_demod(): the strictly largest tone, first wins; fsk.c:760-778), one byte per bit */
int  sonde_fsk_fetch_bits(sonde_fsk_t *f, int32_t channel, uint8_t *bits, int32_t max);
/* fsk_get_demod_stats + Sf: smoothed magnitude spectrum (Ndft floats, DC at Ndft/2) and samples consumed so far */
int  sonde_fsk_stats(sonde_fsk_t *f, int32_t channel, sonde_fsk_frame_t *last, float *Sf, int64_t *samples);
/* Eye diagram of the last modem frame as fsk_get_demod_stats() returns it (rx_eye, fsk.c:857-903; modem_stats.h:63-65):
 * neyetr = 8 traces (8/M per tone, interleaved by tone) of neyesamp = 2P/ceil(2P/160) integrator magnitudes, normalised
 * to the largest.  eye receives neyetr * neyesamp floats (row-major; at most 8 * 160); returns that count. */
int  sonde_fsk_eye(sonde_fsk_t *f, int32_t channel, float *eye, int32_t *neyetr, int32_t *neyesamp);
int  sonde_fsk_clear_estimators(sonde_fsk_t *f);                          /* fsk_clear_estimators (fsk.c:981)     */
int  sonde_fsk_kernel_ms(sonde_fsk_t *f, double *avg_ms, int64_t *launches);

/* ---- the consumer of the soft decisions on the device: `rs41mod --softin [-i] [--ecc|--ecc2]` for every channel of a modem engine
 * (auto_rx's pipe `fsk_demod ... | rs41mod --softin -i`, auto_rx/autorx/decode.py:901-909).  find_softbinhead / corr_softhdb
 * (demod/mod/demod_mod.c:1692-1762, threshold 0.7), the bit loop and de-whitening of rs41mod.c:2893-2962 and rs41_ecc() (:1703-1769) run in
 * device memory; only completed frames (518 bytes each) come to the host.  invert_stream = --softinv, opt_inv = -i, opt_auto = --auto.
 * sonde_type: SONDE_RS41; SONDE_DFM09 = `dfm09mod --softin [-i] [--ecc|--ecc2]` (dfm09mod.c:1604-1720: 32 raw header symbols, two soft symbols per bit, eight frames
 * per header hit, de-interleave + Hamming(8,4) incl. the soft 2-bit pass :231-345 on a lane per codeword); SONDE_M10 = `m10mod --softin` (m10mod.c:1405-1510: header
 * threshold 0.8 in either polarity, differential decoding, the rest of the second skipped, checkM10 :594-628); SONDE_RD94RD41 = `rd94rd41drop --softin / --softinv [-i]`
 * (rd94rd41drop.c:1357-1386: the sign of every soft bit, the 40-bit header ring, 2400 raw bits a frame, then Manchester pairs -> bytes -> five chksum16 and seven
 * CRC-16 checks on the device; ecc_level and opt_auto are ignored).  No CPU fallback. */
typedef struct sonde_softin_dev sonde_softin_dev_t;
int  sonde_softin_dev_create(int32_t n_channels, int32_t sonde_type, int32_t ecc_level, int32_t invert_stream, int32_t opt_inv, int32_t opt_auto,
                             sonde_softin_dev_t **out);
void sonde_softin_dev_destroy(sonde_softin_dev_t *s);
/* consume the soft decisions the modem's last process call left in device memory (every channel; n_channels must match).  Synchronous. */
int  sonde_softin_dev_push_fsk(sonde_softin_dev_t *s, sonde_fsk_t *modem);
/* sonde_softin_dev_push_fsk in two halves: submit waits for the modem's launch (sonde_fsk_wait), then puts the consumer's kernels and the copies of its frames on the
 * consumer's OWN stream and returns; collect waits for them.  In between the modem can be given its next second (sonde_fsk_submit_device): the modem keeps the soft
 * decisions of its last two launches, so the consumer of second k runs beside the modem of second k + 1.  Order per second: sonde_fsk_wait(k - 1), collect (k - 2),
 * submit_fsk (k - 1), sonde_fsk_submit_device (k).  The modem's launch that overwrites a buffer of soft decisions waits (on the device) for the consumer that was
 * given that buffer, so another order costs overlap, never frames. */
int  sonde_softin_dev_submit_fsk(sonde_softin_dev_t *s, sonde_fsk_t *modem);
/* the same over the modem's launch BEFORE the one in flight — for the order sonde_fsk_wait (k - 1), sonde_fsk_submit_device (k), collect (k - 2), submit_fsk_behind (k - 1):
 * the modem gets its next second before the host does the decoder's bookkeeping, and nothing here waits for the launch in flight.  With no launch in flight:
 * sonde_softin_dev_submit_fsk. */
int  sonde_softin_dev_submit_fsk_behind(sonde_softin_dev_t *s, sonde_fsk_t *modem);
int  sonde_softin_dev_collect(sonde_softin_dev_t *s);
/* the same over any soft-bit streams in device memory: channel c at d_soft + c * ch_stride, n_bits each */
int  sonde_softin_dev_push_device(sonde_softin_dev_t *s, const float *d_soft, int64_t ch_stride, int32_t n_bits);
/* frames completed by the push calls since the last fetch (all channels, in completion order per call; channel / len / ecc / mv / mv_pos = the header's
 * bit index in the channel's stream); returns the count (<= max) */
int  sonde_softin_dev_fetch(sonde_softin_dev_t *s, sonde_frame_t *out, int32_t max);
/* SONDE_DFM09 / SONDE_M10 consumers: their frames (ecc[3] = hamming()'s value per block; cs_ok / cs_calc = the frame checksum) */
int  sonde_softin_dev_fetch_dfm(sonde_softin_dev_t *s, sonde_dfm_frame_t *out, int32_t max);
int  sonde_softin_dev_fetch_m10(sonde_softin_dev_t *s, sonde_m10_frame_t *out, int32_t max);
/* SONDE_M20 = `m20mod --softin` (m20mod.c:1276-1377; auto_rx's pipe `fsk_demod ... 2 48000 9600 - - | m20mod --json --ptu -vvv --softin -i`, auto_rx/autorx/decode.py:1131-1167):
 * the 32 raw header symbols of m20mod.c:81 at 0.8 in either polarity, two soft symbols per bit, differential decoding with bit0 = '0' at the frame's first bit,
 * (101 + 64) * 8 bits, bits2bytes, and what print_frame derives (:875-907, blk_checkM10 :548-560, checkM10 :562-596): len with its clamp, fw, cs_calc / cs_ok, blk_ok — a
 * length byte of 0 as sonde_m20_frame_finish has it.  ecc_level is ignored, opt_inv / opt_auto mean nothing to the differential code.  A push call holds at most
 * 4 * n_channels + 16 frames over all channels (without the skip a channel completes one per 2672 symbols); frames beyond that are decoded, not delivered, and counted
 * as dropped.
 * set_m20_skip: 1 (default) = verbosity below 3, one symbol per counted bit dropped behind a frame up to 5 * 808 (m20mod.c:1361-1373); 0 = -vvv, auto_rx's form: the
 * search resumes right behind the frame's 2640 symbols.  Takes effect with the next push call.  SONDE_E_ARG for consumers of another kind; so is fetch_m20. */
int  sonde_softin_dev_set_m20_skip(sonde_softin_dev_t *s, int32_t skip);
int  sonde_softin_dev_fetch_m20(sonde_softin_dev_t *s, sonde_m20_frame_t *out, int32_t max);
/* SONDE_RD94RD41 consumers: the frame record of include/sonde_drop.h (sample = soft bits read when the header matched) */
int  sonde_softin_dev_fetch_drop(sonde_softin_dev_t *s, sonde_drop_frame_t *out, int32_t max);

/* ---- SONDE_LMS6 consumers: `lms6Xmod --softin --vit | --vit2 [--ecc] [-r] [--json] [--lms6 | --lmsX]` for every channel (auto_rx's pipe
 * `fsk_demod ... | lms6Xmod --json --softin --vit2 -i`, auto_rx/autorx/decode.py:1209).  Header search, block assembly, the K = 7 Viterbi decoder (one wavefront per
 * channel, a trellis state per lane), deconv and bits2bytes run in device memory (lms6Xmod.c:1352-1433, :232-441); per completed block 308 bytes come to the host, where
 * the consumer's own sonde_lms6_dec_t of that channel does RS(255,223), frame sync, CRC and the text (sonde_lms6_dec_block_bytes).  opts as for sonde_lms6_dec_create,
 * except: vit must be 1 or 2 after the --json rule (the algebraic decoder alone has no device form) and ecc 0 or 1: SONDE_E_ARG otherwise.  invert_stream = --softinv.
 * With opts->typ == 0 (auto detection) the length of a block depends on what the host made of the block before it (lms6Xmod.c:1436-1462): a channel stops at every
 * completed block, and the push call launches the channels with input left again until the call is consumed — the result is the reference's for any cut of the stream.
 * Every one of those launches reads the modem's soft decisions, so with auto detection submit_fsk / submit_fsk_behind complete the call before they tell the modem
 * that its buffer has been read (collect then only hands over the result): any order of calls stays right, the overlap with the modem's next launch is given up.  With
 * a forced type submit queues the one launch and collect waits for it, as for the other kinds.
 * A push call holds at most 4 * n_channels + 16 blocks over all channels (a channel completes one per 4176 / 4800 soft bits, two at most in a second): calls of up to
 * two seconds of soft bits never reach that; blocks beyond it are decoded, not delivered, and counted as dropped (sonde_softin_dev_counts). */
int  sonde_softin_dev_create_lms6(int32_t n_channels, const sonde_lms6_opts_t *opts, int32_t invert_stream, sonde_softin_dev_t **out);
#define SONDE_LMS6_TEXT_MAX 2048   /* the text of a block: at most two frames end in one (their `-r` lines are the longest: 223 x 3 + 6 characters each) */
typedef struct {
    int32_t  channel;
    int32_t  type;           /* the type in effect after the block (6, 0x0206, 10)                                         */
    float    mv;             /* score of the header in front of the block                                                   */
    int32_t  text_len;
    uint64_t hdr_bit;        /* the header's bit index in the channel's stream (soft bits read when it matched)             */
    int32_t  blen, err;      /* bytes the block gave, deconv's error index                                                  */
    char     text[SONDE_LMS6_TEXT_MAX];   /* what the reference prints for this block, NUL-terminated                       */
} sonde_lms6_softin_t;
/* blocks completed by the push calls since the last fetch (per channel in stream order); returns the count (<= max) */
int  sonde_softin_dev_fetch_lms6(sonde_softin_dev_t *s, sonde_lms6_softin_t *out, int32_t max);
/* RS(255,223) of the blocks on the device as well (k_lms6_rs, csrc/sonde_lms6_rs.hip; sonde_lms6_rs_t, sonde_hip.h): with the switch on the kernel runs over a
 * round's block records before they are copied, and the channels' decoders take its results (sonde_lms6_dec_block_rs) instead of decoding.  Off by default;
 * nothing else of the interface changes, the stop-at-block rule of auto detection included.  A call in flight is completed first.  _stats: RS results taken from
 * records / decoded on the host instead, over all channels (sonde_lms6_dec_rs_stats). */
int  sonde_softin_dev_set_lms6_rs(sonde_softin_dev_t *s, int32_t on);
int  sonde_softin_dev_lms6_rs_stats(sonde_softin_dev_t *s, int64_t *used, int64_t *missed);

/* ---- SONDE_RS92 consumers: `rs92mod --softin [-i] --ecc ...` for every channel (auto_rx's pipe `fsk_demod --cs16 -b -20000 -u 20000 -s --stats=N 2 48000 4800 - - |
 * rs92mod -vx -v --crc --ecc --vel --json --softin -i -e <rinex> --ptu`, auto_rx/autorx/decode.py:976-987).  On the device, one wavefront per channel
 * (rs92mod.c:1959-2050, :183-196, :1360-1385): the 60 raw header symbols of 2A 2A 10 at 0.8 (a score of exactly 0.8f and the NaN of an all-zero window are no hits; the
 * ring is emptied on every hit; a hit of the other polarity is dropped, rs92mod has no --auto), 234 bytes of 10 bits from two soft symbols per bit, and RS(255,231) of
 * the finished frame — always on, as --json and the host tier force it.  Per completed frame 264 bytes come to the host, where the consumer's own sonde_rs92_dec_t of
 * that channel (its calibration rows are per sonde) checks the CRCs, solves the position and prints (sonde_rs92_dec_corrected) when the record is fetched.  Only
 * complete frames are delivered: the reference prints a partial frame at end of input alone, and a consumer behind a live modem has none.
 * opts as for sonde_rs92_dec_create; opts->inv = -i, invert_stream = --softinv.  SONDE_E_ARG for what would leave a record's text without a bound: gps_verbose == 8
 * (-gg) and dbg.  sonde_softin_dev_create with SONDE_RS92 is SONDE_E_ARG (the kind needs its options); the other kinds' fetch calls refuse an RS92 consumer and
 * fetch_rs92 / the load calls refuse the other kinds.  One launch per push call: submit_fsk / collect keep the overlap with the modem's next second.
 * A push call holds at most 4 * n_channels + 16 frames over all channels (a channel completes one per 4740 symbols at the least); frames beyond that are decoded, not
 * delivered, and counted as dropped. */
int  sonde_softin_dev_create_rs92(int32_t n_channels, const sonde_rs92_opts_t *opts, int32_t invert_stream, sonde_softin_dev_t **out);
/* orbit data for every channel's decoder; SONDE_E_ARG as sonde_rs92_dec_load_ephemeris / _almanac return it */
int  sonde_softin_dev_rs92_load_ephemeris(sonde_softin_dev_t *s, const char *path);
int  sonde_softin_dev_rs92_load_almanac(sonde_softin_dev_t *s, const char *path);
/* The text of a frame under the accepted options.  Its line: "[%5d] (id) (date) day time" 52, position / (d:) / velocity / a DOP list of 12 PRNs 190, three PTU
 * values 60, aux 22, "  # [crc]" (n) 15, the -vv calibration row with its aux bytes and frequency / kill timer 160: below 500 for values in their physical range;
 * a %f field of a float without one (a temperature from corrupt calibration rows) can take 47 characters, eight of them 380 more.  The JSON object: 360 of fixed
 * text and bounded fields, the same six %f fields again, version 31: below 800.  2048 leaves room for both at their worst. */
#define SONDE_RS92_TEXT_MAX 2048
typedef struct {
    int32_t  channel;
    int32_t  ec;             /* rs_decode's value for the frame: 0, the number of repaired bytes, -1 / -2 / -3 = left as received */
    float    mv;             /* score of the header in front of the frame                                                         */
    int32_t  text_len;       /* SONDE_E_ARG (negative) if the text did not fit: text is "" then                                   */
    uint64_t hdr_bit;        /* symbols read when the header matched                                                             */
    uint8_t  frame[SONDE_RS92_FRAME_LEN];     /* the frame behind rs92_ecc                                                       */
    char     text[SONDE_RS92_TEXT_MAX];       /* what the reference prints for this frame, NUL-terminated                        */
} sonde_rs92_softin_t;
/* frames completed by the push calls since the last fetch (per channel in stream order); returns the count (<= max) */
int  sonde_softin_dev_fetch_rs92(sonde_softin_dev_t *s, sonde_rs92_softin_t *out, int32_t max);
/* on != 0: fetch_rs92 makes the texts of a fetch through sonde_gps_rs92_text_batch (include/sonde_gps.h): the 4-satellite subset search of every fetched frame in
 * one launch on the device, the winning subset alone solved by the channel's decoder.  The texts are the same; off (the state of a new consumer) nothing changes.
 * The first call with on != 0 makes the consumer's solver (SONDE_E_NOMEM / _NOGPU as sonde_gps_dev_create); SONDE_E_ARG for another kind of consumer. */
int  sonde_softin_dev_set_rs92_gps(sonde_softin_dev_t *s, int32_t on);
/* the solver's counts so far (sonde_gps_stats_t, include/sonde_gps.h; all zero for a consumer that never had the switch on) */
int  sonde_softin_dev_rs92_gps_stats(sonde_softin_dev_t *s, sonde_gps_stats_t *out);

/* ---- SONDE_IMET54 consumers: `imet54mod --softin [-i] [--auto] [--ecc] ...` for every channel (auto_rx's pipe `fsk_demod --cs16 -b -10000 -u 10000 -s --stats=N 2 48000
 * 4800 - - | imet54mod --ecc --json --softin -i --ptu`, auto_rx/autorx/decode.py:1215-1250).  On the device, one wavefront per channel (imet54mod.c:1007-1063,
 * :107-133, :162-303, :350-360, :618-660): the 40 header symbols of 00 AA 24 24 at 0.8 (a score of exactly 0.8f and the NaN of an all-zero window are no hits; the ring
 * is left as it is on a hit and frame symbols never enter it; a hit of the other polarity is dropped, or with --auto flips the polarity for good), 220 8N1
 * characters, the 8 x 8 de-interleave, 216 Hamming(8,4) codewords (single errors repaired with --ecc only), the three ecc sums of print_frame and both check sums.
 * Per completed frame 152 bytes come to the host, where the consumer's own sonde_imet54_dec_t of that channel prints from the device's values
 * (sonde_imet54_dec_decoded) when the record is fetched.  Only complete frames are delivered: the reference prints a partial frame at end of input alone, and a
 * consumer behind a live modem has none.
 * opts as for sonde_imet54_dec_create (SONDE_E_ARG as it returns it); opts->inv = -i, opts->aut = --auto, json implies ecc; invert_stream = --softinv.
 * sonde_softin_dev_create with SONDE_IMET54 is SONDE_E_ARG (the kind needs its options); the other kinds' fetch calls refuse an iMet-54 consumer and fetch_imet54
 * refuses the other kinds.  One launch per push call: submit_fsk / collect keep the overlap with the modem's next second.
 * A push call holds at most 4 * n_channels + 16 frames over all channels (a channel completes at most one per 2240 symbols); frames beyond that are decoded, not
 * delivered, and counted as dropped. */
int  sonde_softin_dev_create_imet54(int32_t n_channels, const sonde_imet54_opts_t *opts, int32_t invert_stream, sonde_softin_dev_t **out);
/* The text of a frame under any options.  The -r4 line: 108 x "XX " and a blank per four bytes 351, the tag 5, " # (-1) [-1]" with counts of three digits at most
 * 16, the newline: below 380.  The position line (with -r only beside --json, where --silent suppresses it; counted all the same): serial 15, time 17, lat / lon /
 * alt 49 (printed only inside their ranges, get_GPS), four PTU fields inside theirs 50, tag 5, status 10, ecc 16: below 170.  The JSON object: 250 of fixed text and
 * bounded fields, freq 11, version 31: below 300.  1024 leaves room for all three. */
#define SONDE_IMET54_TEXT_MAX 1024
typedef struct {
    int32_t  channel;
    int32_t  ecc_frm, ecc_tlm, ecc_std;   /* print_frame's sums over the first 104 codewords (ecc_tlm: 88): repaired codewords, -1 behind an uncorrectable one */
    int32_t  crc;            /* 0 neither check sum good, 1 the standard frame's (crc32ok), 2 the continuous frame's (crc32ok_cont)      */
    float    mv;             /* score of the header in front of the frame                                                         */
    uint64_t hdr_bit;        /* symbols read when the header matched                                                             */
    int32_t  text_len;       /* SONDE_E_ARG (negative) if the text did not fit: text is "" then                                   */
    uint8_t  frame[SONDE_IMET54_FRAME_LEN];   /* the frame behind Hamming(8,4)                                                   */
    char     text[SONDE_IMET54_TEXT_MAX];     /* what the reference prints for this frame, NUL-terminated                        */
} sonde_imet54_softin_t;
/* frames completed by the push calls since the last fetch (per channel in stream order); returns the count (<= max) */
int  sonde_softin_dev_fetch_imet54(sonde_softin_dev_t *s, sonde_imet54_softin_t *out, int32_t max);

/* ---- SONDE_MEISEI consumers: `meisei100mod --softin [--ecc] ...` for every channel (auto_rx's pipe `fsk_demod --cs16 -s -b -15000 -u 15000 --stats=N 2 48000 2400 - - |
 * meisei100mod --softin --json --ptu --ecc`, auto_rx/autorx/decode.py:1343-1379).  On the device, one wavefront per channel (meisei100mod.c:654-776, :213-229;
 * bch_ecc_mod.c:968-1043): the 48 header half symbols at 0.8 in either polarity (a score of exactly 0.8f and the NaN of an all-zero window are no hits; there is no
 * polarity rule and no -i, biphase-S compares neighbours; the ring is left as it is on a hit and frame symbols never enter it), 576 biphase-S bits behind the 24
 * known header bits, and with --ecc the 12 BCH(63,51) blocks with the padding and word-parity rules, corrected bits written back only where the block is accepted.
 * Per completed frame 104 bytes come to the host, where the consumer's own sonde_meisei_dec_t of that channel (the variant in effect, the 64-word configuration, the
 * counters) prints from the device's bits and verdicts (sonde_meisei_dec_decoded) when the record is fetched.  Only complete frames are delivered: a consumer
 * behind a live modem has no end of input.
 * opts as for sonde_meisei_dec_create (SONDE_E_ARG as it returns it); json implies ecc; invert_stream = --softinv (it changes the sign of mv, and bits only at exact
 * zeros).  sonde_softin_dev_create with SONDE_MEISEI is SONDE_E_ARG (the kind needs its options); the other kinds' fetch calls refuse a Meisei consumer and
 * fetch_meisei refuses the other kinds.  One launch per push call: submit_fsk / collect keep the overlap with the modem's next second.
 * A push call holds at most 4 * n_channels + 16 frames over all channels (a channel completes at most one per 1200 half symbols — 48 of the header and 1152 behind
 * it — so two seconds at 2400 Bd fit); frames beyond that are decoded, not delivered, and counted as dropped. */
int  sonde_softin_dev_create_meisei(int32_t n_channels, const sonde_meisei_opts_t *opts, int32_t invert_stream, sonde_softin_dev_t **out);
/* The text of a frame under any options.  The -r line: per subframe the header word 7, 12 words of 5 and `#......#  ` 10, the newline: below 160.  The two printers:
 * a counter 8, `--dbg` 30, time 15, date 13, T / RH 20, position 55 (lat / lon / alt are 32-bit integers over 1e7 / 1e2), speeds 45, (ok)[OK] 8, sn 28, fq 15 and
 * the newlines of a hand-over: below 260 for the frame.  The JSON object: 330 of fixed text and bounded fields, freq 11, tx_frequency 25, version 31: below 400.
 * 1024 leaves room for all three. */
#define SONDE_MEISEI_TEXT_MAX 1024
typedef struct {
    int32_t  channel;
    uint8_t  block_err[12];  /* per block, subframe 0 first: 0 / 1 / 2 corrected bits, 0xF padding or word parity failed, 0xE uncorrectable; all 0 without --ecc */
    int32_t  err_frm;        /* blocks 0xE / 0xF                                                                                  */
    int32_t  err_blks;       /* blocks that are not 0                                                                             */
    float    mv;             /* score of the header in front of the frame, with its sign                                          */
    uint64_t hdr_bit;        /* half symbols read when the header matched                                                         */
    int32_t  text_len;       /* SONDE_E_ARG (negative) if the text did not fit: text is "" then                                   */
    uint8_t  bits[SONDE_MEISEI_FRAME_BYTES];  /* the 600 frame bits behind BCH, MSB first: bits2val positions map directly         */
    char     text[SONDE_MEISEI_TEXT_MAX];     /* what the reference prints for this frame, NUL-terminated                          */
} sonde_meisei_softin_t;
/* frames completed by the push calls since the last fetch (per channel in stream order); returns the count (<= max) */
int  sonde_softin_dev_fetch_meisei(sonde_softin_dev_t *s, sonde_meisei_softin_t *out, int32_t max);

/* ---- SONDE_MRZ consumers: `mp3h1mod --softin [-i] [--auto] [--ofs n] ...` for every channel (auto_rx's pipe `fsk_demod --cs16 -s -b -10000 -u 10000 --stats=N 2 48000
 * 2400 - - | mp3h1mod --auto --json --softin --ptu`, auto_rx/autorx/decode.py:1256-1293).  On the device, one wavefront per channel (mp3h1mod.c:1151-1242, :157-183,
 * :280-310, :805-815): the 44 header half symbols at 0.82 (a score of exactly 0.82f and the NaN of an all-zero window are no hits; the ring is left as it is on a
 * hit and frame symbols never enter it; a hit of the other polarity is dropped, or with --auto flips the polarity for good), Manchester bits from two half symbols
 * each (s2 - s1 >= 0, inverted unless the polarity is) behind the 22 known header bits, up to the frame length in effect: 408 bits (ECEF) or 384 (lat / lon).  At
 * the end of a frame (not with -R) the bytes from bit --ofs on, the frame type (FF FF at bytes 30 / 31: CRC over 42 bytes, else 45) and the CRC-16 (0xA001
 * reflected, start value 0xFFFF, from byte 3) are the device's; a good CRC sets the length of the channel's next frame, in the same call or a later one.
 * Per completed frame 80 bytes come to the host, where the consumer's own sonde_mrz_dec_t of that channel (configuration words, serial numbers, --uniq and the
 * JSON time-out state) prints from the device's bits and the device's verdict (sonde_mrz_dec_decoded) when the record is fetched.  Only complete frames are
 * delivered: a consumer behind a live modem has no end of input.
 * opts as for sonde_mrz_dec_create (SONDE_E_ARG as it returns it); opts->inv = -i, opts->aut = --auto; invert_stream = --softinv.  sonde_softin_dev_create with
 * SONDE_MRZ is SONDE_E_ARG (the kind needs its options); the other kinds' fetch calls refuse an MRZ consumer and fetch_mrz refuses the other kinds.  One launch
 * per push call: submit_fsk / collect keep the overlap with the modem's next second.
 * A push call holds at most 8 * n_channels + 16 frames over all channels (a channel completes at most one per 44 + 2 (384 - 22) = 768 half symbols, seven in two
 * seconds at 2400); frames beyond that are decoded — the length switch included — not delivered, and counted as dropped. */
int  sonde_softin_dev_create_mrz(int32_t n_channels, const sonde_mrz_opts_t *opts, int32_t invert_stream, sonde_softin_dev_t **out);
/* The text of a frame under any options.  The -r line: 51 x "XX " 153, the tag 6: below 160.  The -R line: 408 bits and the newline.  The position line: counter 6,
 * time 12, lat / lon / alt 75 (32-bit integers over 1e6 / 1e2, or angles and a height from 32-bit ECEF centimetres), speeds 40, sats 12, d_alt 25, four PTU fields
 * of 16-bit and range-checked values 60, the tag 6 (-c: 24), the -vv configuration word 60 (%.5f of any float: 46), --dbg 40: below 400.  The JSON object: 330 of
 * fixed text and bounded fields, freq 11, version 31: below 450.  1024 leaves room for line and object. */
#define SONDE_MRZ_TEXT_MAX 1024
#define SONDE_MRZ_BITS_BYTES 52
typedef struct {
    int32_t  channel;
    int32_t  nbits;          /* 408 / 384: the frame length in effect for this frame, counted from the header's first bit          */
    int32_t  inv;            /* polarity in effect for the frame's bits (-i, or what --auto made of it)                           */
    int32_t  crc_ok;         /* the device's CRC verdict (0 with -R: never looked at)                                             */
    int32_t  crclen;         /* 42 (lat / lon) / 45 (ECEF) bytes under the CRC (0 with -R)                                        */
    float    mv;             /* score of the header in front of the frame, with its sign                                          */
    uint64_t hdr_bit;        /* half symbols read when the header matched                                                         */
    int32_t  text_len;       /* SONDE_E_ARG (negative) if the text did not fit: text is "" then                                   */
    uint8_t  bits[SONDE_MRZ_BITS_BYTES];      /* the frame bits from the header's first, MSB first; 0 behind nbits                 */
    char     text[SONDE_MRZ_TEXT_MAX];        /* what the reference prints for this frame, NUL-terminated                          */
} sonde_mrz_softin_t;
/* frames completed by the push calls since the last fetch (per channel in stream order); returns the count (<= max) */
int  sonde_softin_dev_fetch_mrz(sonde_softin_dev_t *s, sonde_mrz_softin_t *out, int32_t max);

/* ---- SONDE_MTS01 consumers: `mts01mod --softin ...` for every channel.  On the device, one wavefront per channel (mts01mod.c:543-618, :76-127, :151-162): the 32
 * header symbols AA AA B4 2B at 0.8 in either polarity (a score of exactly 0.8f and the NaN of an all-zero window are no hits; every hit counts; the ring is left as
 * it is on a hit and frame symbols never enter it), 1048 bits read raw, one symbol each (s >= 0) — an inverted stream gives inverted bits and a failing CRC, as the
 * reference does; --softinv puts it right — then the 131 bytes MSB first and the CRC-16 (0x8005, MSB first, start value 0xFFFF, over bytes 1 .. 128, bit-reversed,
 * against bytes[130] << 8 | bytes[129]).  Per completed frame 152 bytes come to the host, where the consumer's own sonde_mts01_dec_t of that channel prints from
 * the device's bytes, CRC value and verdict (sonde_mts01_dec_decoded) when the record is fetched.  Only complete frames are delivered.
 * opts as for sonde_mts01_dec_create (SONDE_E_ARG as it returns it); invert_stream = --softinv.  sonde_softin_dev_create with SONDE_MTS01 is SONDE_E_ARG (the kind
 * needs its options); the other kinds' fetch calls refuse an MTS01 consumer and fetch_mts01 refuses the other kinds.  One launch per push call.
 * A push call holds at most 4 * n_channels + 16 frames over all channels (a channel completes at most one per 32 + 1048 = 1080 symbols of the 1200 a second);
 * frames beyond that are decoded, not delivered, and counted as dropped. */
int  sonde_softin_dev_create_mts01(int32_t n_channels, const sonde_mts01_opts_t *opts, int32_t invert_stream, sonde_softin_dev_t **out);
/* The text of a frame under any options.  The -R line alone: 1048 bits, a blank per byte 131, the newline: 1180.  The -r line: 131 x "XX " 393, " # [XXXX:XXXX]"
 * 14, " # [OK]" 7, the newline: 415.  The text line: the frame's string 130 at the most, the tag 7.  The -v line and the JSON object print numbers read from the
 * frame's own text with %f: a field like 1e308 takes 316 characters, and the printer cuts each of its formatted pieces at 639 — two such pieces in the -v line
 * (below 1500 with the rest of it) and one in the JSON object (below 900).  4096 leaves room for all three at their worst. */
#define SONDE_MTS01_TEXT_MAX 4096
#define SONDE_MTS01_FRAME_BYTES 131
typedef struct {
    int32_t  channel;
    int32_t  crcval;         /* crc16_re over bytes 1 .. 128, as the device computed it                                           */
    int32_t  crcdat;         /* bytes[130] << 8 | bytes[129]                                                                      */
    int32_t  crc_ok;         /* the device's verdict                                                                              */
    float    mv;             /* score of the header in front of the frame, with its sign                                          */
    int32_t  text_len;       /* SONDE_E_ARG (negative) if the text did not fit: text is "" then                                   */
    uint64_t hdr_bit;        /* symbols read when the header matched                                                              */
    uint8_t  bytes[SONDE_MTS01_FRAME_BYTES];  /* the 1048 frame bits, MSB first                                                    */
    char     text[SONDE_MTS01_TEXT_MAX];      /* what the reference prints for this frame, NUL-terminated                          */
} sonde_mts01_softin_t;
/* frames completed by the push calls since the last fetch (per channel in stream order); returns the count (<= max) */
int  sonde_softin_dev_fetch_mts01(sonde_softin_dev_t *s, sonde_mts01_softin_t *out, int32_t max);

/* ---- SONDE_WXR301 consumers: `weathex301d --softin [-i] [--pn9] ...` for every channel (auto_rx's pipe `fsk_demod --cs16 -s -b -40000 -u 40000 --mask 50000
 * --stats=N 2 <96000|100000> <4800|5000> - - | weathex301d --softin -i --json [--pn9]`, auto_rx/autorx/decode.py:1414-1423, :1458-1467).  On the device, one wavefront
 * per channel (weathex301d.c:607-648, :250-256, :272-294, :359-375): bit = (s >= 0), with -i (s <= 0) — +-0.0 is a 1 and a NaN a 0 either way; every bit enters a 40-bit
 * ring that starts holding no bit at all; outside a frame a ring equal to AA AA AA 2D D4 (--pn9: AA AA AA C1 94) opens a frame of the header's 40 bits and the next
 * 512; inside a frame the header is not searched for, and behind the 552nd bit the search resumes on a ring that holds the frame's last 40 bits.  Then the 69 bytes
 * MSB first, with --pn9 bytes 6 .. 68 XORed with the PN9 sequence, chkval = xor8 << 8 | sum8 over the 53 bytes from ofs (6, --pn9: 8) against
 * x[ofs + 53] << 8 | x[ofs + 54], and the frame id, serial and counter.  Per completed frame 176 bytes come to the host; sonde_wxr_print_decoded (include/sonde_wxr.h)
 * prints from the record's bytes and verdict.  Only complete frames are delivered: a header open at the end of the input prints nothing.
 * invert_stream XORs with opts->invert (the two inversions cancel each other, as for the dropsondes).  sonde_softin_dev_create with SONDE_WXR301 is SONDE_E_ARG (the
 * kind needs its options); the other kinds' fetch calls refuse a WxR consumer and fetch_wxr refuses the other kinds.  One launch per push call.
 * A push call holds at most 20 * n_channels + 16 frames over all channels (a call of n bits completes at most n / 552 + 1 per channel: ten for a second at 5000 Bd);
 * frames beyond that are decoded, not delivered, and counted as dropped. */
typedef struct {
    int32_t pn9;             /* --pn9: header AA AA AA C1 94, PN9 de-whitening from byte 6, the check from byte 8                  */
    int32_t invert;          /* -i                                                                                                */
    int32_t reserved[6];
} sonde_wxr_softin_opts_t;
struct sonde_wxr_softin_rec {
    int32_t  channel;
    int32_t  reserved0;
    uint64_t hdr_bit;        /* soft bits read before the one that completed the header (-t prints hdr_bit / 4800 or 5000)        */
    uint8_t  raw[69];        /* the 552 frame bits, MSB first, before PN9 (what -R prints)                                        */
    uint8_t  x[69];          /* behind PN9 (without --pn9 the same bytes): what -r prints and the fields are read from           */
    uint8_t  reserved1[2];
    uint32_t chkval;         /* xor8 << 8 | sum8 over x[ofs .. ofs + 52], as the device computed it                               */
    uint32_t chkdat;         /* x[ofs + 53] << 8 | x[ofs + 54]                                                                    */
    uint8_t  chk_ok;         /* the device's verdict                                                                              */
    uint8_t  frid;           /* x[ofs + 6]                                                                                        */
    uint8_t  reserved2[2];
    uint32_t sn, cnt;        /* serial (x[ofs .. ofs + 3], little endian) and counter (x[ofs + 4], x[ofs + 5])                    */
};                           /* 176 bytes: the sonde_wxr_softin_rec_t of include/sonde_wxr.h                                      */
int  sonde_softin_dev_create_wxr(int32_t n_channels, const sonde_wxr_softin_opts_t *opts, int32_t invert_stream, sonde_softin_dev_t **out);
/* frames completed by the push calls since the last fetch (per channel in stream order); returns the count (<= max) */
int  sonde_softin_dev_fetch_wxr(sonde_softin_dev_t *s, sonde_wxr_softin_rec_t *out, int32_t max);

/* tallies since creation: frames completed (SONDE_LMS6: blocks; accepted = the frames with a good CRC-16 that ended in them, the decoders' own count), frames accepted (RS41: rs41_ecc() >= 0; DFM: no block uncorrectable; M10 / M20: checksum good; RD94RD41: every block of the type print_frame chooses good; RS92: rs_decode >= 0; iMet-54: ecc_frm >= 0 and a check sum good, or ecc_std == 0 — the JSON rule without the status bits; Meisei: no block 0xE / 0xF; MRZ / MTS01: CRC-16 good, WXR301: chk_ok, and their repaired and symbol tallies stay 0), frames repaired (RS92: rs_decode > 0; iMet-54: ecc_frm > 0; Meisei: any block 1 or 2), symbols / codewords repaired (RS92: the sum of the positive rs_decode values; iMet-54: of the positive ecc_frm; Meisei: the sum of the corrected bits), frames lost to a full buffer */
int  sonde_softin_dev_counts(sonde_softin_dev_t *s, int64_t *frames, int64_t *ecc_ok, int64_t *repaired, int64_t *symbols, int64_t *dropped);

#ifdef __cplusplus
}
#endif
#endif
