/*
 * oracle/ref_imet4_harness.c — TEST INFRASTRUCTURE.  Our code around the *reference's own* imet/imet4iq.c, which is compiled where it lies
 * (oracle/Makefile: -I$(REF)/imet, nothing copied).  The file is included with its main() renamed, and that main() is what runs: its
 * argument loop, its option rules, f32_sample, the sliding two-tone DFT and the slicer, over an in-memory capture (raw IQ or a WAV file's
 * bytes).  Nothing of it is restated here.  The values the CLI never prints are copied out while it runs, for the front-end sweep of the GPU
 * engine (tests/test_gpu_imet4_front_sweep.py):
 *   per sample   the decimated IF input, the sample entering the IF low-pass, the sample leaving it, the sample entering the FM low-pass,
 *                the front-end sample; Df, tap set, dc, pre_pos, mv_pos in effect for it; xsum and the two DFT sums behind it;
 *   frames       the 1000 bits and the sample at which print_frame is called;  the IQ-dc means;  the tap and mixer tables.
 * As in ref_mk2a_harness.c the library is built with -finstrument-functions: the compiler calls the two hooks below around every function
 * of the reference; they act on f32_sample, print_frame and the two readers.  fopen() (the capture in memory), fread() (inside a reader its
 * last argument is dsp->fp, which tells where main's dsp_t lies) and fprintf() (stdout swallowed) go through macros.
 * tests/test_imet4_front_cases.py pins the recording: the frames are those the compiled CLI (oracle/_ref/imet4iq) prints under -r.
 *
 * Flags as imet/Makefile (-Ofast on top of the top-level -O3 -w); the _O2 twin is the same source with -O2 alone.
 */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdarg.h>
#include <stddef.h>
#include <string.h>
#include <math.h>
#include <complex.h>
#define NI __attribute__((no_instrument_function))
static FILE *h_fopen(const char *path, const char *mode) NI;
static size_t h_fread(void *p, size_t sz, size_t n, FILE *f, void *where) NI;
static int h_fprintf(FILE *f, const char *fmt, ...) NI;
#define fopen(p, m) h_fopen((p), (m))
#define fread(p, s, n, f) h_fread((p), (s), (n), (f), (void *)&(f))
#define fprintf(...) h_fprintf(__VA_ARGS__)
#define main imet4iq_main
#include "imet4iq.c"
#undef main
#undef fopen
#undef fread
#undef fprintf

typedef struct {
    int    sr, bps;          /* input rate, 8 / 16 (raw IQ); for wav = 1 both come from the file's header    */
    int    wav;              /* the capture is a WAV file (FM audio), no --iq                                  */
    int    lp_iq, lpbw_hz, lp_fm, dc, opt_min, imet1;
    double fq;               /* the --iq argument                                                              */
} ref_imet4_cfg_t;

#define IMET4_NCONST 16
enum { C_IFSR, C_DECM, C_DECTAPS, C_LUTLEN, C_IQTAPS, C_FMTAPS, C_M, C_SPS, C_LP, C_MAXCNT0, C_MAXLIM, C_SRBASE, C_IQ, C_DF_END, C_LOCKED_END, C_N };

typedef struct {
    /* capacities (in) */
    int max_n, max_frames, max_dc, max_lut, max_taps;
    /* counts (out) */
    int n, n_frames, n_dc;
    /* per sample */
    float *ifin;             /* [max_n][2] decimated IF input (a second pass with --iq alone)                                    */
    float *zrot;             /* [max_n][2] lpIQ_buf: the sample entering the IF low-pass (--lpIQ)                                */
    float *zlp;              /* [max_n][2] iqbuf: the sample the discriminator takes (IQ)                                        */
    float *fm;               /* [max_n] lpFM_buf: the sample entering the FM low-pass (--lpFM)                                   */
    float *x;                /* [max_n] the front-end sample (bufs)                                                              */
    double *df;              /* [max_n] Df in effect for the sample                                                              */
    double *dc;              /* [max_n] dsp->dc in effect for the sample                                                         */
    unsigned char *nominal;  /* [max_n] 1: the nominal IF tap set (ws_lpIQ1) is in effect for the sample                         */
    unsigned *pre_pos, *mv_pos;   /* [max_n] in effect for the sample (set by main at a header)                                  */
    float *xsum;             /* [max_n] behind the sample                                                                        */
    double *F;               /* [max_n][4] F1sum, F2sum behind the sample                                                        */
    /* events, frames, tables */
    double *dcev;            /* [max_dc][4]: sample_in when seen, avgIQx, avgIQy, maxcnt behind it                               */
    unsigned char *bits;     /* [max_frames][1000]                                                                               */
    double *fsample;         /* [max_frames] sample_in where print_frame is called                                               */
    unsigned char *bytes;    /* [max_frames][100] byteframe as print_frame's bits2bytes leaves it                                */
    float *lut;              /* [max_lut][2] dsp->ex                                                                             */
    float *ws_dec, *ws_iq0, *ws_iq1, *ws_fm;   /* [max_taps] the duplicated tables (2 x taps entries)                            */
    double consts[IMET4_NCONST];
} ref_imet4_out_t;

static struct {
    ref_imet4_out_t *o;
    const void *raw; size_t nbytes;
    int pass, rc, reading;
    dsp_t *dsp;              /* main's dsp, known from the first sample read on */
    ui32_t done;             /* samples recorded                                */
    ui32_t entered;          /* samples whose state at entry is recorded        */
    float avgx, avgy; ui32_t maxcnt;
} H;

static void NI copy_taps(float *dst, const float *ws, int taps, int cap) {
    int i;
    if (!dst || !ws) return;
    for (i = 0; i < 2 * taps && i < cap; i++) dst[i] = ws[i];
}

static void NI tables(dsp_t *dsp) {
    ref_imet4_out_t *o = H.o;
    const int iq = dsp->opt_iq >= 5;
    int i;
    o->consts[C_IFSR] = dsp->sr; o->consts[C_DECM] = (iq && dsp->decM) ? dsp->decM : 1; o->consts[C_DECTAPS] = iq ? dsp->dectaps : 0;
    o->consts[C_LUTLEN] = iq ? dsp->lut_len : 0;
    o->consts[C_IQTAPS] = (iq && (dsp->opt_lp & LP_IQ)) ? dsp->lpIQtaps : 0; o->consts[C_FMTAPS] = (dsp->opt_lp & LP_FM) ? dsp->lpFMtaps : 0;
    o->consts[C_M] = dsp->M; o->consts[C_SPS] = dsp->sps; o->consts[C_LP] = dsp->opt_lp; o->consts[C_IQ] = iq;
    o->consts[C_MAXCNT0] = IQdc.maxcnt; o->consts[C_MAXLIM] = IQdc.maxlim; o->consts[C_SRBASE] = iq ? dsp->sr_base : dsp->sr;
    H.maxcnt = IQdc.maxcnt;
    if (dsp->decFM != 1) { H.rc = -4; return; }
    if (iq && ((int)dsp->lut_len > o->max_lut || 2 * (int)dsp->dectaps > o->max_taps)) { H.rc = -3; return; }
    if (2 * dsp->lpIQtaps > o->max_taps || 2 * dsp->lpFMtaps > o->max_taps) { H.rc = -3; return; }
    if (iq) {
        for (i = 0; i < (int)dsp->lut_len; i++) { o->lut[2 * i] = crealf(dsp->ex[i]); o->lut[2 * i + 1] = cimagf(dsp->ex[i]); }
        if (dsp->decM > 1) copy_taps(o->ws_dec, ws_dec, dsp->dectaps, o->max_taps);
        if (dsp->opt_lp & LP_IQ) { copy_taps(o->ws_iq0, dsp->ws_lpIQ0, dsp->lpIQtaps, o->max_taps); copy_taps(o->ws_iq1, dsp->ws_lpIQ1, dsp->lpIQtaps, o->max_taps); }
    }
    if (dsp->opt_lp & LP_FM) copy_taps(o->ws_fm, dsp->ws_lpFM, dsp->lpFMtaps, o->max_taps);
}

/* what is in effect for the sample f32_sample is about to make (main may have moved pre_pos since the last one), and the DFT sums main has
   formed behind the one before */
static void NI at_entry(void) {
    ref_imet4_out_t *o = H.o;
    dsp_t *dsp = H.dsp;
    const ui32_t m = dsp->sample_in;
    if (H.pass != 2) return;
    if (m > 0 && (int)m - 1 < o->max_n) {
        double *f = o->F + 4 * (size_t)(m - 1);
        f[0] = creal(F1sum); f[1] = cimag(F1sum); f[2] = creal(F2sum); f[3] = cimag(F2sum);
    }
    if ((int)m < o->max_n && m >= H.entered) {
        o->df[m] = dsp->Df; o->dc[m] = dsp->dc; o->pre_pos[m] = dsp->pre_pos; o->mv_pos[m] = dsp->mv_pos;
        o->nominal[m] = (dsp->opt_iq && (dsp->opt_lp & LP_IQ)) ? (dsp->ws_lpIQ == dsp->ws_lpIQ1) : 1;
        H.entered = m + 1;
    }
}

static void NI at_exit(void) {
    ref_imet4_out_t *o = H.o;
    dsp_t *dsp = H.dsp;
    for (; H.done < dsp->sample_in; H.done++) {          /* one sample per call; every value is still where f32_sample left it */
        const ui32_t n = H.done;
        if ((int)n >= o->max_n) continue;
        if (H.pass == 1) {                               /* --iq alone: iqbuf holds z as it leaves the decimator */
            const float complex z = dsp->iqbuf[n & 1];
            o->ifin[2 * n] = crealf(z); o->ifin[2 * n + 1] = cimagf(z);
            continue;
        }
        o->x[n] = dsp->bufs[n % dsp->M];
        o->xsum[n] = dsp->xsum;
        if (dsp->opt_iq) {
            const float complex z = dsp->iqbuf[n & 1];
            o->zlp[2 * n] = crealf(z); o->zlp[2 * n + 1] = cimagf(z);
            if (dsp->opt_lp & LP_IQ) {
                const float complex y = dsp->lpIQ_buf[n % dsp->lpIQtaps];
                o->zrot[2 * n] = crealf(y); o->zrot[2 * n + 1] = cimagf(y);
            }
        }
        if (dsp->opt_lp & LP_FM) o->fm[n] = dsp->lpFM_buf[n % dsp->lpFMtaps];
    }
    if (H.pass != 2) return;
    if (IQdc.avgIQx != H.avgx || IQdc.avgIQy != H.avgy || IQdc.maxcnt != H.maxcnt) {
        if (o->n_dc < o->max_dc) {
            double *e = o->dcev + 4 * (size_t)o->n_dc;
            e[0] = dsp->sample_in; e[1] = IQdc.avgIQx; e[2] = IQdc.avgIQy; e[3] = IQdc.maxcnt;
        }
        o->n_dc++;
        H.avgx = IQdc.avgIQx; H.avgy = IQdc.avgIQy; H.maxcnt = IQdc.maxcnt;
    }
    o->n = (int)dsp->sample_in;
    o->consts[C_DF_END] = dsp->Df; o->consts[C_LOCKED_END] = dsp->locked; o->consts[C_N] = dsp->sample_in;
}

static FILE * NI h_fopen(const char *path, const char *mode) { (void)path; return fmemopen((void *)H.raw, H.nbytes, mode); }
static size_t NI h_fread(void *p, size_t sz, size_t n, FILE *f, void *where) {
    if (!H.dsp && H.reading) {                           /* inside f32read_sample / f32read_cblock the stream argument is dsp->fp */
        dsp_t *d = (dsp_t *)((char *)where - offsetof(dsp_t, fp));
        if (d->fp != f || d->sample_in != 0 || d->sr <= 0) { H.rc = -5; return 0; }
        H.dsp = d;
        if (H.pass == 2) { tables(d); at_entry(); }
    }
    return fread(p, sz, n, f);
}
static int NI h_fprintf(FILE *f, const char *fmt, ...) {
    va_list ap; int r;
    if (f == stdout) return 0;
    va_start(ap, fmt); r = vfprintf(f, fmt, ap); va_end(ap);
    return r;
}

/* hidden: the C library has empty functions of these names, and a process that loaded it first would bind the calls to them */
#define HOOK __attribute__((no_instrument_function, visibility("hidden")))
void HOOK __cyg_profile_func_enter(void *fn, void *site);
void HOOK __cyg_profile_func_exit(void *fn, void *site);
void __cyg_profile_func_enter(void *fn, void *site) {
    (void)site;
    if (fn == (void *)f32read_sample || fn == (void *)f32read_cblock) { H.reading = 1; return; }
    if (!H.dsp) return;
    if (fn == (void *)f32_sample) at_entry();
    else if (fn == (void *)print_frame && H.pass == 2) {
        ref_imet4_out_t *o = H.o;
        if (o->n_frames < o->max_frames) {
            memcpy(o->bits + (size_t)1000 * o->n_frames, bitframe, 1000);
            o->fsample[o->n_frames] = H.dsp->sample_in;
        }
        o->n_frames++;
    }
}
void __cyg_profile_func_exit(void *fn, void *site) {
    (void)site;
    if (fn == (void *)f32read_sample || fn == (void *)f32read_cblock) { H.reading = 0; return; }
    if (H.dsp && fn == (void *)f32_sample) at_exit();
    else if (H.dsp && fn == (void *)print_frame && H.pass == 2 && H.o->n_frames >= 1 && H.o->n_frames <= H.o->max_frames)
        memcpy(H.o->bytes + (size_t)LEN_BYTEFRAME * (H.o->n_frames - 1), byteframe, LEN_BYTEFRAME);
}

/* the CLI's argument list for a configuration, and one run of its main() over the capture */
static int NI run_main(const ref_imet4_cfg_t *c, int pass) {
    char num[4][40];
    char *argv[24];
    int n = 0;
    argv[n++] = "imet4iq";
    if (!c->wav) { snprintf(num[0], sizeof num[0], "%.17g", c->fq); argv[n++] = "--iq"; argv[n++] = num[0]; }
    if (c->opt_min) argv[n++] = "--min";
    if (c->imet1) argv[n++] = "--imet1";
    if (pass == 2) {
        if (c->lpbw_hz) { snprintf(num[1], sizeof num[1], "%.6f", c->lpbw_hz / 1e3); argv[n++] = "--lpbw"; argv[n++] = num[1]; }
        else if (c->lp_iq) argv[n++] = "--lpIQ";
        if (c->lp_fm) argv[n++] = "--lpFM";
        if (c->dc) argv[n++] = "--dc";
    }
    if (!c->wav) {
        snprintf(num[2], sizeof num[2], "%d", c->sr); snprintf(num[3], sizeof num[3], "%d", c->bps);
        argv[n++] = "-"; argv[n++] = num[2]; argv[n++] = num[3];
    }
    argv[n++] = "capture";
    argv[n] = NULL;
    /* the reference keeps its slicer and DFT state in globals that a second run in one process would inherit */
    F1sum = 0; F2sum = 0; bufpos = -1; bitpos = 0; memset(buf, 0, sizeof buf); buf[0] = 'x'; memset(&gpx, 0, sizeof gpx);
    memset(bitframe + 10, 0, sizeof bitframe - 10);
    H.pass = pass; H.dsp = NULL; H.reading = 0; H.done = 0; H.entered = 0; H.avgx = H.avgy = 0; H.maxcnt = 0;
    return imet4iq_main(n, argv);
}

/* returns 0, or a negative code: -1 arguments, -100 the reference's main gave up, -3 a capacity was too small, -4 an option the harness
   does not record (FM decimation), -5 main's dsp_t was not where the reader's stream argument says */
int NI ref_imet4_run(const ref_imet4_cfg_t *c, const void *raw, size_t nbytes, ref_imet4_out_t *o)
{
    int rc = 0;
    if (!c || !raw || !o || (!c->wav && c->bps != 8 && c->bps != 16)) return -1;
    o->n = o->n_frames = o->n_dc = 0;
    memset(&H, 0, sizeof H);
    H.o = o; H.raw = raw; H.nbytes = nbytes;
    if (!c->wav) rc = run_main(c, 1);        /* pass 1: the decimated IF input, which neither Df nor a tap set enters */
    if (rc == 0) rc = run_main(c, 2);        /* pass 2: the decoder */
    H.pass = 0; H.dsp = NULL;
    if (rc) return -100;
    if (H.rc) return H.rc;
    if (o->n > o->max_n || o->n_frames > o->max_frames || o->n_dc > o->max_dc) return -3;
    return 0;
}
