/*
 * host/imet4iq.c — iMet-4 / iMet-1-RS decoder with the reference's imet/imet4iq.c contract, on libsonde_hip.
 *
 * argv  : --iq <fq>, --lpIQ, --lpbw <kHz>, --lpFM, --dc, --min, --imet1, --json, --jsn_cfq <Hz>, -r, --rawbits, -v, -b,
 *         "- <sr> <8|16>" (headerless IQ on stdin), or a WAV file (IQ with --iq, FM audio otherwise); stdin without a file
 * stdout: what the reference prints per frame (sonde_imet4_print_frame), flushed per frame, and "\n" at EOF
 * stderr: "IF:" / "dec:" for IQ input, the WAV header lines
 * exit  : 0 at EOF, 255 on argument / input / init errors.  Not built (exit 255 with a message): --decFM, --noLUT, 32-bit samples,
 *         rates whose filters do not fit the engine's history rings.  No GPU: exit 255 (there is no CPU fallback).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sonde_hip.h"
#include "sonde_imet4.h"
#include "wav_header.h"

static void json_version(char *dst, size_t cap) {
    const char *ver = getenv("SONDE_JSN_VERSION");
#ifdef VER_JSN_STR
    if (!ver) ver = VER_JSN_STR;
#endif
    if (ver && cap) { strncpy(dst, ver, cap - 1); dst[cap - 1] = 0; }
}

int main(int argc, char **argv) {
    sonde_imet4_cfg_t cfg;
    sonde_imet4_opts_t po;
    memset(&cfg, 0, sizeof cfg);
    memset(&po, 0, sizeof po);
    double fq = 0.0, lpbw = 16e3;
    int pcmraw = 0, cfreq = -1, nch = 1;
    FILE *fp = NULL;
    const char *prog = argv[0];

    for (int i = 1; i < argc && !fp; i++) {
        const char *a = argv[i];
        if (!strcmp(a, "-h") || !strcmp(a, "--help")) {
            fprintf(stderr, "%s [options] audio.wav\n", prog);
            fprintf(stderr, "  options:\n");
            fprintf(stderr, "       -v, --verbose\n");
            fprintf(stderr, "       -r, --raw\n");
            return 0;
        }
        else if (!strcmp(a, "-v") || !strcmp(a, "--verbose")) { }
        else if (!strcmp(a, "-r") || !strcmp(a, "--raw")) po.raw = 1;
        else if (!strcmp(a, "--rawbits")) po.rawbits = 1;
        else if (!strcmp(a, "-b")) { }
        else if (!strcmp(a, "--iq")) {
            if (++i >= argc) return -1;
            fq = atof(argv[i]);
            if (fq < -0.5) fq = -0.5;
            if (fq > 0.5) fq = 0.5;
            cfg.iq = 1;
        }
        else if (!strcmp(a, "--lpIQ")) cfg.lp_iq = 1;
        else if (!strcmp(a, "--lpbw")) {
            if (++i >= argc) return -1;
            const double bw = atof(argv[i]);
            if (bw > 4.0 && bw < 256.0) lpbw = bw * 1e3;
            cfg.lp_iq = 1;
        }
        else if (!strcmp(a, "--lpFM")) cfg.lp_fm = 1;
        else if (!strcmp(a, "--decFM") || !strcmp(a, "--noLUT")) {
            fprintf(stderr, "%s (sonde_hip): %s is not supported\n", prog, a);
            return -1;
        }
        else if (!strcmp(a, "--dc")) cfg.dc = 1;
        else if (!strcmp(a, "--min")) cfg.min = 1;
        else if (!strcmp(a, "--imet1")) cfg.imet1 = 1;
        else if (!strcmp(a, "--json")) po.json = 1;
        else if (!strcmp(a, "--jsn_cfq")) {
            if (++i >= argc) return -1;
            int frq = atoi(argv[i]);
            if (frq < 300000000) frq = -1;
            cfreq = frq;
        }
        else if (!strcmp(a, "-")) {
            if (i + 2 >= argc) return -1;
            cfg.sample_rate = atoi(argv[++i]);
            cfg.bits = atoi(argv[++i]);
            if (cfg.sample_rate < 1 || (cfg.bits != 8 && cfg.bits != 16 && cfg.bits != 32)) { fprintf(stderr, "- <sr> <bs>\n"); return -1; }
            nch = 2;
            pcmraw = 1;
        }
        else {
            fp = fopen(a, "rb");
            if (!fp) { fprintf(stderr, "%s konnte nicht geoeffnet werden\n", a); return -1; }
        }
    }
    if (!fp) fp = stdin;
    if (!cfg.iq && pcmraw) { fprintf(stderr, "error: raw data not IQ\n"); return -1; }
    if (!pcmraw && wav_read_header(fp, &cfg.sample_rate, &cfg.bits, &nch) < 0) { fprintf(stderr, "error: wav header\n"); return -1; }
    if (cfg.bits == 32) { fprintf(stderr, "%s (sonde_hip): 32-bit samples are not supported\n", prog); return -1; }
    if (cfg.iq && nch != 2) { fprintf(stderr, "%s (sonde_hip): IQ input needs 2 channels\n", prog); return -1; }
    if (nch < 1) { fprintf(stderr, "error: wav header\n"); return -1; }
    if (cfreq > 0) po.jsn_freq_khz = (int)((cfreq + fq * cfg.sample_rate + 500) / 1e3);
    json_version(po.version, sizeof po.version);
    cfg.lpbw_hz = (int)(float)lpbw;

    /* the reference's IF rate rule, for its two stderr lines */
    int if_sr = 0, decM = 1;
    int chunk_max = cfg.sample_rate / 4 > 0 ? cfg.sample_rate / 4 : 1;           /* <= 0.25 s per call: frames reach auto_rx live */
    sonde_imet4_t *eng = NULL;
    int rc = sonde_imet4_create(&cfg, 1, &fq, chunk_max, &eng, &if_sr, &decM);
    if (cfg.iq) { fprintf(stderr, "IF: %d\n", if_sr); fprintf(stderr, "dec: %d\n", decM); }
    chunk_max -= chunk_max % decM;                                                 /* whole IF samples per call (the engine's rule) */
    if (rc) { fprintf(stderr, "%s (sonde_hip): engine init failed (%d)\n", prog, rc); return -1; }
    sonde_imet4_printer_t *pr = NULL;
    if (sonde_imet4_printer_create(&po, &pr)) { sonde_imet4_destroy(eng); return -1; }

    const int bps = cfg.bits / 8, comp = cfg.iq ? 2 : 1;
    const size_t frame_bytes = (size_t)bps * nch;             /* one sample of all WAV channels (IQ: the pair) */
    unsigned char *raw = malloc(frame_bytes * chunk_max);
    unsigned char *buf = malloc((size_t)bps * comp * chunk_max);
    static sonde_imet4_frame_t fr[8];
    static char text[1 << 16];
    int status = 0;
    if (!raw || !buf) status = -1;
    while (!status) {
        const size_t got_all = fread(raw, frame_bytes, chunk_max, fp);
        const size_t got = got_all - got_all % decM;         /* a partial decimation block at the end is dropped, as by the reference */
        if (got > 0) {
            const unsigned char *src = raw;
            if (!cfg.iq && nch > 1) {                          /* FM audio: the first channel */
                for (size_t k = 0; k < got; k++) memcpy(buf + k * bps, raw + k * frame_bytes, bps);
                src = buf;
            }
            rc = sonde_imet4_process_host(eng, src, (int)got);
            if (rc) { fprintf(stderr, "%s (sonde_hip): engine failure (%d)\n", prog, rc); status = -1; break; }
            int nf;
            while ((nf = sonde_imet4_fetch_frames(eng, fr, 8)) > 0) {
                for (int k = 0; k < nf; k++) {
                    const int len = sonde_imet4_print_frame(pr, fr[k].bits, fr[k].nbits, text, sizeof text);
                    if (len > 0) fwrite(text, 1, len, stdout);
                    fflush(stdout);
                }
            }
        }
        if (got_all < (size_t)chunk_max) break;
    }
    if (!status) fprintf(stdout, "\n");
    fflush(stdout);
    free(raw); free(buf);
    sonde_imet4_printer_destroy(pr);
    sonde_imet4_destroy(eng);
    if (fp != stdin) fclose(fp);
    return status;
}
