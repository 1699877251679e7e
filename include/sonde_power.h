/*
 * sonde_power.h — C ABI of the spectrum survey and peak pick in libsonde_hip.so.
 *
 * The first of auto_rx's three steps (survey, detect, decode): an averaged power spectrum of the band, which auto_rx takes from
 * rtl_power / ss_power / ka9q (auto_rx/autorx/sdr_wrappers.py:571-766), and the peaks it picks from it (autorx/scan.py:1007-1063 with
 * autorx/utils.py:437-587 detect_peaks).  There is no in-process API in the reference; auto_rx calls the binary and reads its log
 * file.  host/sonde_power.c keeps that command line on top of this ABI.
 * Conventions as sonde_hip.h (0 / count on success, negative SONDE_E_* on error).
 */
#ifndef SONDE_POWER_H
#define SONDE_POWER_H

#include "sonde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SONDE_POWER_RECT 0      /* rectangular window                                                  */
#define SONDE_POWER_HANN 1      /* periodic Hann: 0.5 - 0.5 cos(2 pi i / nfft)                         */
#define SONDE_POWER_NFFT_MIN 256
#define SONDE_POWER_NFFT_MAX 16384
#define SONDE_POWER_FLOOR_DB (-200.0f)   /* what a bin without power reads                             */

typedef struct sonde_power sonde_power_t;

typedef struct {
    int32_t abi_version;     /* SONDE_ABI_VERSION                                                       */
    int32_t device;
    int32_t n_streams;       /* wideband IQ streams surveyed side by side, one spectrum each            */
    int32_t sample_rate;     /* complex samples per second                                              */
    int32_t bits;            /* 8 (unsigned, (u - 128) / 128), 16 (int16 / 32768) or 32 (float32)       */
    int32_t nfft;            /* segment length: a power of two, 256 .. 16384                            */
    int32_t window;          /* SONDE_POWER_RECT / SONDE_POWER_HANN                                     */
    int32_t max_chunk;       /* largest n_samples per process call                                      */
    double  center_hz;       /* tuned frequency of the stream (bin 0)                                   */
    float   crop;            /* fraction of the bins left out of fetch, half at each edge (rtl_power -c): 0 <= crop < 1 */
    int32_t reserved[3];
} sonde_power_cfg_t;

typedef struct {
    int32_t nfft, bins;          /* bins: what fetch returns per stream (nfft less the cropped edges)    */
    int32_t threads, lds_bytes;  /* workgroup of the transform kernel and its LDS                        */
    int32_t workgroups_per_cu;   /* as the runtime reports its occupancy                                 */
    int32_t max_workgroups;      /* compute units * workgroups_per_cu: the grid never exceeds it         */
    double  step_hz;             /* sample_rate / nfft                                                   */
    double  window_sum;          /* sum of the window weights: |X|^2 / window_sum^2 is what fetch reports */
    int32_t reserved[4];
} sonde_power_info_t;

int  sonde_power_create(const sonde_power_cfg_t *cfg, sonde_power_t **out);
void sonde_power_destroy(sonde_power_t *s);
int  sonde_power_info(const sonde_power_t *s, sonde_power_info_t *info);
/* forget everything: the accumulators, the segment counts and the carried tail of every stream */
int  sonde_power_reset(sonde_power_t *s);

/* Push n_samples complex samples per stream; stream c starts stream_stride samples behind stream c - 1 (stream_stride >= n_samples;
 * pointers aligned to one complex sample).  Segments are consecutive blocks of nfft samples of the STREAM, however the calls cut it:
 * what is left behind the last whole segment stays on the device and goes in front of the next call.  process_host returns when
 * h_in may be reused; process_device only queues the work on the survey's stream: d_in must be complete when it is called and stay
 * unchanged until a later call has waited for that stream (fetch, reset, kernel_ms, the next process call, destroy). */
int  sonde_power_process_host(sonde_power_t *s, const void *h_in, int64_t stream_stride, int32_t n_samples);
int  sonde_power_process_device(sonde_power_t *s, const void *d_in, int64_t stream_stride, int32_t n_samples);
/* segments averaged into the stream's spectrum so far (since create, reset or a fetch with reset) */
int64_t sonde_power_segments(const sonde_power_t *s, int32_t stream);

/* The averaged spectrum of one stream in dB (10 log10 of mean |X|^2 / window_sum^2: a full-scale complex sinusoid centred on a bin
 * reads 0 dB), in ascending frequency, without the cropped edges.  *f_low_hz / *f_high_hz: centre frequencies of the first and the last
 * bin written, so that linspace(low, high, count) gives every bin's centre; *step_hz = sample_rate / nfft.  A bin without power (and
 * every bin before the first whole segment) reads SONDE_POWER_FLOOR_DB; neither inf nor nan is ever written.  reset != 0: the stream's
 * accumulator and segment count start again (its carried tail stays: the stream goes on).  Returns the number of bins written;
 * max smaller than that: SONDE_E_RANGE.  db == NULL: only the count and the frequencies. */
int  sonde_power_fetch(sonde_power_t *s, int32_t stream, float *db, double *f_low_hz, double *f_high_hz, double *step_hz, int32_t max, int reset);
int  sonde_power_kernel_ms(sonde_power_t *s, const char *kernel, double *avg_ms, int64_t *launches);

/* Peak pick of auto_rx (scan.py:1007-1063) on a spectrum of n values whose frequencies are linspace(f_low_hz, f_high_hz, n).  Host only,
 * no GPU.  In the reference's order: noise floor = median; detect_peaks(power, mph = floor + snr_threshold_db, mpd = min_distance_hz /
 * step_hz) — rising edges of plateaus, never the first or last value, nothing at or beside a NaN, lower peaks within mpd of a higher
 * one dropped; by power, descending; quantised to quantization_hz (round half to even); duplicates out, first kept; outside
 * [min_freq_hz - q/2, max_freq_hz + q/2] out; within q/2 of a never_scan_hz entry out; at most max_peaks.
 * Returns the number of peaks (written to peaks_hz, at most max_out of them); *noise_floor_db as np.median gives it. */
int  sonde_power_peaks(const double *db, int32_t n, double f_low_hz, double f_high_hz, double step_hz,
                       double snr_threshold_db, double min_distance_hz, double quantization_hz, double min_freq_hz, double max_freq_hz,
                       const double *never_scan_hz, int32_t n_never_scan, int32_t max_peaks,
                       double *noise_floor_db, double *peaks_hz, int32_t max_out);

/* One line of an rtl_power log: "date, time, Hz low, Hz high, Hz step, samples, dB, dB, ..." and a newline; unix_time in UTC.  Hz low /
 * Hz high are the first and last bin centres (what auto_rx's readers hand to linspace), written with as many digits as they need to read
 * back exactly; powers as %.2f.  Returns strlen, or the length needed if buflen is too small (nothing useful is written then). */
int  sonde_power_csv_line(int64_t unix_time, double f_low_hz, double f_high_hz, double step_hz, int64_t samples,
                          const float *db, int32_t n, char *buf, size_t buflen);

#ifdef __cplusplus
}
#endif
#endif
