/*
 * oracle/ref_mk2a_harness.c — TEST INFRASTRUCTURE.  Our code around the *reference's own* mk2a/mk2a1680mod.c, which is compiled where it
 * lies (oracle/Makefile: -I$(REF)/mk2a, nothing copied).  The file is included with its main() renamed, and that main() is what runs: its
 * argument loop, its option rules, its find_header and its frame loop, over an in-memory capture.  Nothing of it is restated here.  The
 * values the CLI never prints are copied out of its buffers while it runs, for the front-end sweep of the GPU engine
 * (tests/test_gpu_mk2a_front_sweep.py):
 *   per IF sample      the decimated IF input, the value written to rot_iqbuf, the discriminator output (and the tone correlator's);
 *   per output sample  bufs and fm_buffer;
 *   the schedule       every correlation window with mv, mv_pos, dc, dDf and the Df / tap set in effect behind it, every change of the
 *                      IQ-dc average;
 *   frames             bits, bytes (the reference's bits2bytes), mv, mv_pos, Df;
 *   tables             the decimator / IF / FM / IQFM tap tables, the mixer table, the tone phasors.
 *
 * How the harness gets in without touching the reference's text:
 *   - the library is built with -finstrument-functions, so the compiler calls on_enter / on_exit below around every function of the
 *     reference, static and inlined ones included; they act on f32buf_sample (one output sample is complete), getCorrDFT (a window),
 *     find_header (a header was accepted if it returns straight behind a window), print_frame (a frame is complete) and free_buffers;
 *   - four library calls are routed through macros: carg() (the one call per IF sample hands over the dsp_t, which lives on main's stack,
 *     and the angle), fopen() (the capture in memory), strncpy() (main's first call hands over where gpx.frame_bits lies) and printf()
 *     (swallowed).
 * tests/test_mk2a_front_cases.py still pins the result: on every sweep capture the frames, mv and Df recorded here are those the compiled
 * CLI (oracle/_ref/mk2a1680mod) prints under -r -vv.
 *
 * Flags as mk2a/Makefile:13 (-Ofast on top of the top-level -O3 -w); the _O2 twin is the same source with -O2 alone.
 */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdarg.h>
#include <stddef.h>
#include <string.h>
#include <math.h>
#include <complex.h>
#define NI __attribute__((no_instrument_function))
struct h_dsp;
static double h_carg(void *dsp, double complex w) NI;
static FILE *h_fopen(const char *path, const char *mode) NI;
static char *h_strncpy(char *dst, const char *src, size_t n) NI;
static int h_printf(const char *fmt, ...) NI;
#define carg(w) h_carg(dsp, (w))
#define fopen(p, m) h_fopen((p), (m))
#define strncpy(d, s, n) h_strncpy((d), (s), (n))
#define printf(...) h_printf(__VA_ARGS__)
#define main mk2a1680mod_main
#include "mk2a1680mod.c"
#undef main
#undef carg
#undef fopen
#undef strncpy
#undef printf

typedef struct {
    int    sr, bps;          /* input rate, 8 / 16                                             */
    int    opt_iq;           /* 5: --IQ fq, 6: --iq fq                                         */
    int    lp_iq;            /* --lpIQ or --lpbw given                                         */
    int    lpbw_hz;          /* --lpbw k in Hz when 100 < k < 240, else 0 (main's default)     */
    int    lp_fm;            /* --lpFM                                                         */
    int    dec_fm;           /* --decFM 4, --decFM2 2, --decFM1 1, none 0                      */
    int    dc;               /* --dc                                                           */
    int    opt_min;          /* --min                                                          */
    int    invert;           /* -i                                                             */
    int    shift;            /* -d                                                             */
    float  thres;            /* --ths (0.7)                                                    */
    float  baud;             /* --br, <= 0: none                                               */
    double fq;               /* the --iq / --IQ argument                                       */
} ref_mk2a_cfg_t;

#define MK2A_NCONST 22
#define MK2A_WCOLS 9
#define MK2A_FCOLS 6

typedef struct {
    /* capacities (in) */
    int max_if, max_out, max_win, max_dc, max_frames, max_lut, max_taps, max_tone;
    /* counts (out) */
    int n_if, n_out, n_win, n_dc, n_frames, n_tone;
    /* streams */
    float *ifin;             /* [max_if][2] decimated IF input (a second pass without --dc, low-passes and FM decimation)   */
    float *zlp;              /* [max_if][2] rot_iqbuf                                                                        */
    float *fm;               /* [max_if] discriminator output per IF sample                                                  */
    float *sraw;             /* [max_if] tone correlator per IF sample (--IQ);                                             */
    float *bufs, *fmbuf;     /* [max_out]                                                                                    */
    /* schedule */
    double *win;             /* [max_win][9]: sample_in at the window, mv, mv_pos, dc, dDf, Df behind it, locked behind it, header found, mv2 */
    double *dcev;            /* [max_dc][4]: sample_in when seen, avgIQx, avgIQy, maxcnt behind it                           */
    /* frames */
    unsigned char *bits;     /* [max_frames][1760] '0' / '1' as 0 / 1                                                        */
    unsigned char *bytes;    /* [max_frames][176] bits2bytes                                                                 */
    double *fmeta;           /* [max_frames][6]: nbits, mv, mv_pos, Df, inv, sample_in behind the frame                      */
    /* tables */
    float *lut;              /* [max_lut][2] dsp->ex                                                                         */
    float *ws_dec, *ws_iq0, *ws_iq1, *ws_fm, *ws_iqfm;   /* [max_taps] each, the duplicated tables (2 x taps entries)        */
    double *tone;            /* [max_tone][5]: n, re / im of cexp(-t iw1), re / im of cexp(-t iw2), t = -n / sr (:893-900)   */
    double consts[MK2A_NCONST];
} ref_mk2a_out_t;

enum { C_IFSR, C_DECM, C_DECFM, C_L, C_M, C_K, C_N, C_DELAY, C_DECTAPS, C_LUTLEN, C_IQTAPS, C_FMTAPS, C_IQFMTAPS, C_LP, C_SPS,
       C_TONESPS, C_MAXCNT0, C_MAXLIM, C_DF_END, C_LOCKED_END, C_NIQBUF, C_MPOFS };


static struct {
    ref_mk2a_out_t *o;
    const void *raw; size_t nbytes;
    int pass;                /* 1: the IF input alone, 2: the decoder                     */
    int rc;
    dsp_t *dsp;              /* main's dsp, known from the first IF sample on             */
    gpx_t *gpx;              /* main's gpx, known before the first sample                 */
    double *arg; int arg_n, arg_max;     /* carg() per IF sample, in order                */
    ui32_t done_out;         /* output samples recorded                                   */
    int pending;             /* a window row waits for what find_header does behind it    */
    float avgx, avgy; ui32_t maxcnt;
} H;

static void NI copy_taps(float *dst, const float *ws, int taps, int cap) {
    int i;
    if (!dst || !ws) return;
    for (i = 0; i < 2 * taps && i < cap; i++) dst[i] = ws[i];
}

/* tables and constants, once main's init_buffers_Lband has run (called at the first IF sample, before anything has moved) */
static void NI tables(dsp_t *dsp) {
    ref_mk2a_out_t *o = H.o;
    int i;
    o->consts[C_IFSR] = dsp->sr; o->consts[C_DECM] = dsp->decM ? dsp->decM : 1; o->consts[C_DECFM] = dsp->opt_fmdec ? dsp->decFM : 1;
    o->consts[C_L] = dsp->L; o->consts[C_M] = dsp->M; o->consts[C_K] = dsp->K; o->consts[C_N] = dsp->DFT.N; o->consts[C_DELAY] = dsp->delay;
    o->consts[C_DECTAPS] = dsp->dectaps; o->consts[C_LUTLEN] = dsp->lut_len;
    o->consts[C_IQTAPS] = (dsp->opt_lp & LP_IQ) ? dsp->lpIQtaps : 0; o->consts[C_FMTAPS] = (dsp->opt_lp & LP_FM) ? dsp->lpFMtaps : 0;
    o->consts[C_IQFMTAPS] = (dsp->opt_lp & LP_IQFM) ? dsp->lpIQFMtaps : 0;
    o->consts[C_LP] = dsp->opt_lp; o->consts[C_SPS] = dsp->sps;
    o->consts[C_MAXCNT0] = IQdc.maxcnt; o->consts[C_MAXLIM] = IQdc.maxlim; o->consts[C_NIQBUF] = dsp->N_IQBUF;
    o->consts[C_MPOFS] = (int)((dsp->lpFMtaps - dsp->lpIQFMtaps - (dsp->sps-1))/(2*dsp->decFM));     /* the offset getCorrDFT takes at :465 */
    H.maxcnt = IQdc.maxcnt;
    if ((int)dsp->lut_len > o->max_lut || 2 * (int)dsp->dectaps > o->max_taps || 2 * dsp->lpIQtaps > o->max_taps || 2 * dsp->lpFMtaps > o->max_taps ||
        2 * dsp->lpIQFMtaps > o->max_taps) { H.rc = -3; return; }
    for (i = 0; i < (int)dsp->lut_len; i++) { o->lut[2 * i] = crealf(dsp->ex[i]); o->lut[2 * i + 1] = cimagf(dsp->ex[i]); }
    copy_taps(o->ws_dec, ws_dec, dsp->dectaps, o->max_taps);
    if (dsp->opt_lp & LP_IQ) { copy_taps(o->ws_iq0, dsp->ws_lpIQ0, dsp->lpIQtaps, o->max_taps); copy_taps(o->ws_iq1, dsp->ws_lpIQ1, dsp->lpIQtaps, o->max_taps); }
    if (dsp->opt_lp & LP_FM) copy_taps(o->ws_fm, dsp->ws_lpFM, dsp->lpFMtaps, o->max_taps);
    if (dsp->opt_lp & LP_IQFM) copy_taps(o->ws_iqfm, dsp->ws_lpIQFM, dsp->lpIQFMtaps, o->max_taps);
    {   /* the tone correlator sums rot_iqbuf[u - n] cexp(+n iw / sr) over the middle of a symbol: n below sps x decFM with sps/2.4 left out at
           either end (:882-902).  The phasors as the reference's cexp gives them. */
        const float span = dsp->sps * (dsp->opt_fmdec ? dsp->decFM : 1), edge = span / 2.4f;
        int n;
        o->consts[C_TONESPS] = span;
        for (n = (int)span - 1; n >= 0; n--) {
            const double t = -n / (double)dsp->sr;
            if (!(n > edge && n < span - edge)) continue;
            if (o->n_tone < o->max_tone) {
                const double complex e1 = cexp(-t*dsp->iw1), e2 = cexp(-t*dsp->iw2);
                double *q = o->tone + 5 * (size_t)o->n_tone;
                q[0] = n; q[1] = creal(e1); q[2] = cimag(e1); q[3] = creal(e2); q[4] = cimag(e2);
            }
            o->n_tone++;
        }
    }
}

static double NI h_carg(void *p, double complex w) {
    const double a = carg(w);
    if (!H.dsp) { H.dsp = (dsp_t *)p; if (H.pass == 2) tables(H.dsp); }
    if (H.arg && H.arg_n < H.arg_max) H.arg[H.arg_n] = a;
    H.arg_n++;
    return a;
}
static FILE * NI h_fopen(const char *path, const char *mode) { (void)path; return fmemopen((void *)H.raw, H.nbytes, mode); }
static char * NI h_strncpy(char *dst, const char *src, size_t n) {
    if (!H.gpx && !H.dsp) H.gpx = (gpx_t *)(dst - offsetof(gpx_t, frame_bits));     /* main's first call, before any sample */
    return strncpy(dst, src, n);
}
static int NI h_printf(const char *fmt, ...) { (void)fmt; return 0; }

/* behind every call of f32buf_sample: what the reference's buffers hold for the output sample it has just finished and for its IF samples.
   Every one of them is still in place: rot_iqbuf keeps 8192, the low-pass buffers at least decFM. */
static void NI record(dsp_t *dsp) {
    ref_mk2a_out_t *o = H.o;
    const ui32_t d = dsp->opt_fmdec ? dsp->decFM : 1;
    for (; H.done_out < dsp->sample_in; H.done_out++) {
        const ui32_t n = H.done_out;
        ui32_t m;
        if ((int)n < o->max_out) { o->bufs[n] = dsp->bufs[n % dsp->M]; o->fmbuf[n] = dsp->fm_buffer[n % dsp->M]; }
        for (m = 0; m < d; m++) {
            const ui32_t u = n * d + m;
            float complex z;
            if ((int)u >= o->max_if) continue;
            z = dsp->rot_iqbuf[u % dsp->N_IQBUF];
            o->zlp[2 * u] = crealf(z); o->zlp[2 * u + 1] = cimagf(z);
            /* the discriminator per IF sample: in lpFM_buf with --lpFM; else only the last of a group reaches fm_buffer, the others are
               formed from the angle noted at carg() as the reference forms them, FM_GAIN x angle / pi in double, stored as float */
            if ((dsp->opt_lp & LP_FM) && (ui32_t)dsp->lpFMtaps >= d) o->fm[u] = dsp->lpFM_buf[u % dsp->lpFMtaps];
            else if (m + 1 == d && !(dsp->opt_lp & LP_FM)) o->fm[u] = dsp->fm_buffer[n % dsp->M];
            else if ((int)u < H.arg_n) o->fm[u] = (float)(FM_GAIN * H.arg[u] / M_PI);
            /* the tone correlator per IF sample: in lpIQFM_buf, or straight in bufs where there is no third low-pass (decFM is 1 then) */
            if (dsp->opt_iq == 5) {
                if ((dsp->opt_lp & LP_IQFM) && (ui32_t)dsp->lpIQFMtaps >= d) o->sraw[u] = dsp->lpIQFM_buf[u % dsp->lpIQFMtaps];
                else if (d == 1) o->sraw[u] = dsp->bufs[n % dsp->M];
                else H.rc = -4;
            }
        }
    }
    if (IQdc.avgIQx != H.avgx || IQdc.avgIQy != H.avgy || IQdc.maxcnt != H.maxcnt) {
        if (o->n_dc < o->max_dc) {
            double *e = o->dcev + 4 * (size_t)o->n_dc;
            e[0] = dsp->sample_in; e[1] = IQdc.avgIQx; e[2] = IQdc.avgIQy; e[3] = IQdc.maxcnt;
        }
        o->n_dc++;
        H.avgx = IQdc.avgIQx; H.avgy = IQdc.avgIQy; H.maxcnt = IQdc.maxcnt;
    }
}

/* a window row is opened when getCorrDFT returns and closed once find_header has acted on it: at the next sample, or where it returns */
static void NI close_window(int found) {
    ref_mk2a_out_t *o = H.o;
    dsp_t *dsp = H.dsp;
    if (!H.pending) return;
    H.pending = 0;
    if (o->n_win <= o->max_win) {
        double *w = o->win + MK2A_WCOLS * (size_t)(o->n_win - 1);
        w[5] = dsp->Df;
        w[6] = (dsp->opt_lp & LP_IQ) ? (dsp->ws_lpIQ == dsp->ws_lpIQ1) : dsp->locked;      /* the tap set in effect: 1 = nominal */
        w[7] = found;
    }
}

static void NI frame_done(void) {
    ref_mk2a_out_t *o = H.o;
    dsp_t *dsp = H.dsp;
    if (H.gpx && dsp && o->n_frames < o->max_frames) {
        char bits[BITFRAME_LEN + 9];
        unsigned char *b = o->bits + (size_t)BITFRAME_LEN * o->n_frames;
        double *m = o->fmeta + MK2A_FCOLS * (size_t)o->n_frames;
        const int nb = (int)strnlen(H.gpx->frame_bits, BITFRAME_LEN);      /* main has closed the bit string with '\0' */
        int i;
        /* where main keeps its bits was learnt from its first strncpy(): a frame of anything but '0' / '1' says that this no longer holds */
        for (i = 0; i < nb; i++) if (H.gpx->frame_bits[i] != '0' && H.gpx->frame_bits[i] != '1') { H.rc = -5; return; }
        if (nb < FRMSTART) { H.rc = -5; return; }
        memset(bits, 0, sizeof bits);
        memcpy(bits, H.gpx->frame_bits, nb);
        for (i = 0; i < BITFRAME_LEN; i++) b[i] = bits[i] == '1';
        bits2bytes(bits, o->bytes + (size_t)FRAME_LEN * o->n_frames);       /* as print_frame applies it, behind zeros from the end on */
        m[0] = nb; m[1] = dsp->mv; m[2] = dsp->mv_pos; m[3] = dsp->Df; m[4] = H.gpx->option.inv; m[5] = dsp->sample_in;
    }
    o->n_frames++;
}

/* hidden: the C library has empty functions of these names, and a process that loaded it first would bind the calls to them */
#define HOOK __attribute__((no_instrument_function, visibility("hidden")))
void HOOK __cyg_profile_func_enter(void *fn, void *site);
void HOOK __cyg_profile_func_exit(void *fn, void *site);
void __cyg_profile_func_enter(void *fn, void *site) {
    (void)site;
    if (H.pass != 2 || !H.dsp) return;
    if (fn == (void *)f32buf_sample) close_window(0);
    else if (fn == (void *)print_frame) frame_done();
    else if (fn == (void *)free_buffers) {
        ref_mk2a_out_t *o = H.o;
        close_window(0);
        o->n_out = (int)H.dsp->sample_in;
        o->n_if = (int)(H.dsp->sample_in * (H.dsp->opt_fmdec ? H.dsp->decFM : 1));
        o->consts[C_DF_END] = H.dsp->Df; o->consts[C_LOCKED_END] = H.dsp->locked;
    }
}

void __cyg_profile_func_exit(void *fn, void *site) {
    dsp_t *dsp = H.dsp;
    ref_mk2a_out_t *o = H.o;
    (void)site;
    if (!dsp) return;
    if (fn == (void *)f32buf_sample) {
        if (H.pass == 2) record(dsp);
        else if (dsp->sample_in > 0) {       /* pass 1: without --dc, low-passes and FM decimation rot_iqbuf holds z as it leaves the decimator */
            const ui32_t u = dsp->sample_in - 1;
            if ((int)u < o->max_if) {
                const float complex z = dsp->rot_iqbuf[u % dsp->N_IQBUF];
                o->ifin[2 * u] = crealf(z); o->ifin[2 * u + 1] = cimagf(z);
            }
        }
    }
    else if (H.pass != 2) return;
    else if (fn == (void *)getCorrDFT) {
        if (o->n_win < o->max_win) {
            double *w = o->win + MK2A_WCOLS * (size_t)o->n_win;
            w[0] = dsp->sample_in; w[1] = dsp->mv; w[2] = dsp->mv_pos; w[3] = dsp->dc; w[4] = dsp->dDf; w[8] = dsp->mv2;
        }
        o->n_win++;
        H.pending = 1;
    }
    else if (fn == (void *)find_header) close_window(1);      /* it returns straight behind a window only with a header */
}

/* the CLI's argument list for a configuration, and one run of its main() over the capture */
static int NI run_main(const ref_mk2a_cfg_t *c, int pass) {
    char num[8][40];
    char *argv[40];
    int n = 0;
    argv[n++] = "mk2a1680mod";
    snprintf(num[0], sizeof num[0], "%.17g", c->fq);
    argv[n++] = (pass == 2 && c->opt_iq == 5) ? "--IQ" : "--iq"; argv[n++] = num[0];
    if (c->opt_min) argv[n++] = "--min";
    if (pass == 2) {
        if (c->lpbw_hz) { snprintf(num[1], sizeof num[1], "%.6f", c->lpbw_hz / 1e3); argv[n++] = "--lpbw"; argv[n++] = num[1]; }
        else if (c->lp_iq) argv[n++] = "--lpIQ";
        if (c->lp_fm) argv[n++] = "--lpFM";
        if (c->dec_fm == 4) argv[n++] = "--decFM";
        else if (c->dec_fm == 2) argv[n++] = "--decFM2";
        else if (c->dec_fm == 1) argv[n++] = "--decFM1";
        if (c->dc) argv[n++] = "--dc";
        if (c->invert) argv[n++] = "-i";
        if (c->shift) { snprintf(num[2], sizeof num[2], "%d", c->shift); argv[n++] = "-d"; argv[n++] = num[2]; }
        if (c->thres > 0) { snprintf(num[3], sizeof num[3], "%.9g", (double)c->thres); argv[n++] = "--ths"; argv[n++] = num[3]; }
        if (c->baud > 0) { snprintf(num[4], sizeof num[4], "%.9g", (double)c->baud); argv[n++] = "--br"; argv[n++] = num[4]; }
    }
    snprintf(num[5], sizeof num[5], "%d", c->sr); snprintf(num[6], sizeof num[6], "%d", c->bps);
    argv[n++] = "-"; argv[n++] = num[5]; argv[n++] = num[6];
    argv[n++] = "capture";
    argv[n] = NULL;
    H.pass = pass; H.dsp = NULL; H.gpx = NULL; H.arg_n = 0; H.done_out = 0; H.pending = 0; H.avgx = H.avgy = 0; H.maxcnt = 0;
    return mk2a1680mod_main(n, argv);
}

/* returns 0, or a negative code: -1 arguments / memory, -100 the reference's main gave up, -3 a capacity was too small, -4 a stream the
   reference keeps no copy of, -5 main's frame bits are not where its first strncpy() pointed */
int NI ref_mk2a_run(const ref_mk2a_cfg_t *c, const void *raw, size_t nbytes, ref_mk2a_out_t *o)
{
    int rc;
    if (!c || !raw || !o || (c->opt_iq != 5 && c->opt_iq != 6) || (c->bps != 8 && c->bps != 16)) return -1;
    o->n_if = o->n_out = o->n_win = o->n_dc = o->n_frames = o->n_tone = 0;
    memset(&H, 0, sizeof H);
    H.o = o; H.raw = raw; H.nbytes = nbytes;
    /* pass 1: the decimated IF input, which neither Df nor a tap set enters */
    rc = run_main(c, 1);
    if (rc == 0) {
        H.arg = (double *)calloc((size_t)o->max_if + 1, sizeof(double)); H.arg_max = o->max_if;
        if (!H.arg) return -1;
        rc = run_main(c, 2);        /* pass 2: the decoder */
        free(H.arg); H.arg = NULL;
    }
    H.pass = 0; H.dsp = NULL; H.gpx = NULL;
    if (rc) return -100;
    if (H.rc) return H.rc;
    if (o->n_if > o->max_if || o->n_out > o->max_out || o->n_win > o->max_win || o->n_dc > o->max_dc || o->n_frames > o->max_frames || o->n_tone > o->max_tone) return -3;
    return 0;
}
