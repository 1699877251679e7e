/*
 * sonde_gps.h — the RS92 position solve's 4-satellite subset search on the GPU (C ABI of libsonde_hip.so).
 *
 * An RS92 frame carries raw GPS ranges; the default solver computes the closed-form solution of every 4-satellite subset (up to 495 per frame) and keeps the one
 * with the best GDOP.  Here that search runs on the device, one wavefront per frame (k_gps_subsets), and returns which subset wins — nothing else.  The decoder
 * then solves that one subset with the functions it always used (sonde_rs92_dec_end, include/sonde_rs92.h), so every printed digit comes from the code that
 * prints it without the device.  A frame the device marks as in doubt, or whose winning GDOP the host does not reproduce bit for bit, gets the host's full search.
 * Off unless a caller asks for it; -g2 (Bancroft) and -gg (prints every subset) frames never become jobs.
 */
#ifndef SONDE_GPS_H
#define SONDE_GPS_H

#include "sonde_rs92.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sonde_gps_dev sonde_gps_dev_t;

/* max_jobs (1 .. 65536): jobs of one launch; device and page-locked host memory for that many are allocated here.  SONDE_E_ARG / _NOMEM / _NOGPU. */
int  sonde_gps_dev_create(int32_t max_jobs, sonde_gps_dev_t **out);
void sonde_gps_dev_destroy(sonde_gps_dev_t *g);

/* picks[i] for jobs[i], i < n: synchronous, on the solver's own stream, in chunks of max_jobs.  SONDE_E_ARG (nothing is launched) for a job with n outside
 * 4 .. 12 or a value of its first n satellites that is not finite. */
int  sonde_gps_dev_solve(sonde_gps_dev_t *g, const sonde_gps_job_t *jobs, int32_t n, sonde_gps_pick_t *picks);

typedef struct {
    int64_t jobs;            /* jobs solved on the device                                                            */
    int64_t launches;        /* kernel launches (chunks)                                                             */
    int64_t doubts;          /* picks that came back in doubt                                                        */
    int64_t mismatches;      /* picks a decoder dropped because it did not reproduce their GDOP (text_batch): 0      */
    int64_t picked;          /* frames whose position came from a pick (text_batch)                                  */
    int64_t reserved[3];
} sonde_gps_stats_t;
int  sonde_gps_dev_stats(const sonde_gps_dev_t *g, sonde_gps_stats_t *out);

/* sonde_gps_rs92_text_batch_with (include/sonde_rs92.h) with this solver: n corrected frames in order, several of one decoder allowed, the text of record i at
 * out + i * stride, its length (or SONDE_E_ARG) in len[i].  g == NULL: a plain loop over sonde_rs92_dec_corrected. */
int  sonde_gps_rs92_text_batch(sonde_gps_dev_t *g, sonde_rs92_dec_t *const *decs, const uint8_t (*frames)[SONDE_RS92_FRAME_LEN], const int32_t *ec, int32_t n,
                               char *out, size_t stride, int32_t *len);

#ifdef __cplusplus
}
#endif
#endif
