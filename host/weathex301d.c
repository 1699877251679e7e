/*
 * host/weathex301d.c — Weathex WxR-301D decoder with the reference's weathex/weathex301d.c contract, on libsonde_hip.
 *
 * argv  : -h, --pn9, -i / --invert, -v / --verbose, --softin, -b, -t, -r / --raw, -R / --RAW, --json, --jsn_cfq <Hz>, a file name; stdin
 *         without one.  Anything else is taken for a file name, as by the reference.
 * stdin : a WAV stream of FM samples (8 / 16 / 32 bits, first channel) — what `iq_dec --FM --IFbw 64 --lpFM --wav` writes — or with
 *         --softin raw float32 soft bits, one per bit (what `fsk_demod -s` writes)
 * stdout: what the reference prints per frame (sonde_wxr_print_frame; -t: "<seconds> " in front), flushed per frame, and "\n" at EOF
 * stderr: the WAV header lines and "samples/bit:"
 * exit  : 0 at EOF, 255 on argument / input / init errors.  The WAV form runs the FM form of the GPU engine; without a GPU it exits with
 *         255 (there is no CPU fallback).  --softin is host code and needs none.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sonde_hip.h"
#include "sonde_wxr.h"
#include "wav_header.h"

static void json_version(char *dst, size_t cap) {
    const char *ver = getenv("SONDE_JSN_VERSION");
#ifdef VER_JSN_STR
    if (!ver) ver = VER_JSN_STR;
#endif
    if (ver && cap) { strncpy(dst, ver, cap - 1); dst[cap - 1] = 0; }
}

static sonde_wxr_printer_t *pr;
static int opt_b, opt_t;
static double t_rate = 1.0;

static void print(const sonde_wxr_frame_t *f) {
    static char text[1 << 12];
    if (opt_t) printf("<%8.3f> ", f->sample / t_rate);
    if (f->complete || opt_b) {                                   /* a header still open at EOF: only -b prints what it has (:692-704) */
        const int len = sonde_wxr_print_frame(pr, f->bits, text, sizeof text);
        if (len > 0) fwrite(text, 1, len, stdout);
    }
    fflush(stdout);
}

int main(int argc, char **argv) {
    sonde_wxr_cfg_t cfg;
    sonde_wxr_opts_t po;
    memset(&cfg, 0, sizeof cfg);
    memset(&po, 0, sizeof po);
    int softin = 0, cfreq = -1, nch = 1;
    FILE *fp = NULL;
    const char *prog = argv[0];

    for (int i = 1; i < argc && !fp; i++) {
        const char *a = argv[i];
        if (!strcmp(a, "-h") || !strcmp(a, "--help")) {
            fprintf(stderr, "%s [options] audio.wav\n", prog);
            fprintf(stderr, "  options:\n");
            fprintf(stderr, "       -i\n");
            fprintf(stderr, "       -b\n");
            return 0;
        }
        else if (!strcmp(a, "--pn9")) cfg.pn9 = po.pn9 = 1;
        else if (!strcmp(a, "-i") || !strcmp(a, "--invert")) cfg.invert = 1;
        else if (!strcmp(a, "-v") || !strcmp(a, "--verbose")) po.vbs = 1;
        else if (!strcmp(a, "--softin")) softin = 1;
        else if (!strcmp(a, "-b")) cfg.opt_b = opt_b = 1;
        else if (!strcmp(a, "-t")) opt_t = 1;
        else if (!strcmp(a, "-r") || !strcmp(a, "--raw")) po.raw = 1;
        else if (!strcmp(a, "-R") || !strcmp(a, "--RAW")) po.raw = 2;
        else if (!strcmp(a, "--json")) po.json = 1;
        else if (!strcmp(a, "--jsn_cfq")) {
            if (++i >= argc) return -1;
            int frq = atoi(argv[i]);
            if (frq < 300000000) frq = -1;
            cfreq = frq;
        }
        else {
            fp = fopen(a, "rb");
            if (!fp) { fprintf(stderr, "%s konnte nicht geoeffnet werden\n", a); return -1; }
        }
    }
    if (!fp) fp = stdin;
    const float baud = cfg.pn9 ? 5000.0f : 4800.0f;
    if (!softin) {
        if (wav_read_header(fp, &cfg.sample_rate, &cfg.bits, &nch) < 0) return -1;
        fprintf(stderr, "samples/bit: %.2f\n", cfg.sample_rate / baud);
        if (nch < 1) { fprintf(stderr, "%s (sonde_hip): a WAV stream without channels is not supported\n", prog); return -1; }
    }
    if (cfreq > 0) po.jsn_freq_khz = (cfreq + 500) / 1000;
    json_version(po.version, sizeof po.version);
    if (sonde_wxr_printer_create(&po, &pr)) return -1;
    int status = 0;

    if (softin) {
        sonde_wxr_softin_t *si = NULL;
        if (sonde_wxr_softin_create(cfg.pn9, cfg.invert, &si)) return -1;
        static float soft[4096];
        static sonde_wxr_frame_t fr[16];
        opt_b = 0;                                                /* the soft-bit loop knows no -b */
        t_rate = (double)(int)baud;
        size_t got;
        while ((got = fread(soft, 4, 4096, fp)) > 0) {
            int nf = sonde_wxr_softin_push(si, soft, (int)got, fr, 16);
            while (nf > 0) {
                for (int k = 0; k < nf; k++) print(&fr[k]);
                nf = sonde_wxr_softin_push(si, NULL, 0, fr, 16);
            }
        }
        if (sonde_wxr_softin_finish(si, fr) == 1) print(&fr[0]);
        sonde_wxr_softin_destroy(si);
    } else {
        cfg.input = SONDE_WXR_IN_FM;
        t_rate = (double)cfg.sample_rate;
        const int chunk_max = cfg.sample_rate / 4 > 0 ? cfg.sample_rate / 4 : 1;    /* <= 0.25 s per call: frames reach auto_rx live */
        sonde_wxr_t *eng = NULL;
        const int rc0 = sonde_wxr_create(&cfg, 1, NULL, chunk_max, &eng);
        if (rc0) { fprintf(stderr, "%s (sonde_hip): engine init failed (%d)\n", prog, rc0); return -1; }
        const size_t width = (size_t)cfg.bits / 8, stride = width * (size_t)nch;
        unsigned char *raw = malloc(stride * chunk_max), *mono = malloc(width * chunk_max);
        static sonde_wxr_frame_t fr[8];
        int eof = 0;
        if (!raw || !mono) status = -1;
        while (!status) {
            const size_t got = fread(raw, stride, chunk_max, fp);        /* whole sample frames only: a partial one is EOF (:147) */
            for (size_t k = 0; k < got; k++) memcpy(mono + k * width, raw + k * stride, width);       /* wav_channel 0 */
            if (got > 0) {
                const int rc = sonde_wxr_process_host(eng, mono, (int)got);
                if (rc) { fprintf(stderr, "%s (sonde_hip): engine failure (%d)\n", prog, rc); status = -1; break; }
            }
            if (got < (size_t)chunk_max) {
                eof = 1;
                if (sonde_wxr_finish(eng)) { status = -1; break; }
            }
            int nf;
            while ((nf = sonde_wxr_fetch_frames(eng, fr, 8)) > 0)
                for (int k = 0; k < nf; k++) print(&fr[k]);
            if (eof) break;
        }
        free(raw); free(mono);
        sonde_wxr_destroy(eng);
    }
    if (!status) fprintf(stdout, "\n");
    fflush(stdout);
    sonde_wxr_printer_destroy(pr);
    if (fp != stdin) fclose(fp);
    return status;
}
