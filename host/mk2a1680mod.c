/*
 * host/mk2a1680mod.c — LMS6-1680 / MkIIa decoder with the reference's mk2a/mk2a1680mod.c contract, on libsonde_hip.
 *
 * argv  : --iq <fq>, --IQ <fq>, --lpIQ, --lpbw <kHz>, --lpFM, --decFM, --decFM2, --decFM1, --dc, --min, -i, --ths <x>, --br <Bd>, -d <shift>,
 *         --crc, --json, --jsn_cfq <Hz>, -r, -v, -vv, -vvv, "- <sr> <8|16>" (headerless IQ on stdin), or an IQ WAV file; stdin without a file
 * stdout: what the reference prints per frame (sonde_mk2a_print_frame), flushed per frame, and "\n" at EOF
 * stderr: "IF:" / "dec:", the low-sample-rate note, the WAV header lines
 * exit  : 0 at EOF, 255 on argument / input / init errors.  Not built (exit 255 with a message): FM-audio input, --iq0, --iqdc, --noLUT,
 *         32-bit samples, rates whose header window does not fit the 8192-point transform.  No GPU: exit 255 (there is no CPU fallback).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sonde_hip.h"
#include "sonde_mk2a.h"
#include "wav_header.h"

static void json_version(char *dst, size_t cap) {
    const char *ver = getenv("SONDE_JSN_VERSION");
#ifdef VER_JSN_STR
    if (!ver) ver = VER_JSN_STR;
#endif
    if (ver && cap) { strncpy(dst, ver, cap - 1); dst[cap - 1] = 0; }
}

int main(int argc, char **argv) {
    sonde_mk2a_cfg_t cfg;
    sonde_mk2a_opts_t po;
    memset(&cfg, 0, sizeof cfg);
    memset(&po, 0, sizeof po);
    double fq = 0.0, lpbw = 180e3;
    float thres = 0.7f, baud = -1;
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
        else if (!strcmp(a, "-v") || !strcmp(a, "--verbose")) po.vbs = 1;
        else if (!strcmp(a, "-vv")) po.vbs = 2;
        else if (!strcmp(a, "-vvv")) po.vbs = 3;
        else if (!strcmp(a, "-r") || !strcmp(a, "--raw")) po.raw = 1;
        else if (!strcmp(a, "-i") || !strcmp(a, "--invert")) cfg.invert = 1;
        else if (!strcmp(a, "--crc")) po.crc = 1;
        else if (!strcmp(a, "--ths")) {
            if (++i >= argc) return -1;
            thres = (float)atof(argv[i]);
        }
        else if (!strcmp(a, "--br")) {
            if (++i >= argc) return -1;
            baud = (float)atof(argv[i]);
            if (baud < 9400 || baud > 9800) baud = 9616.0f;
        }
        else if (!strcmp(a, "-d")) {
            if (++i >= argc) return -1;
            int shift = atoi(argv[i]);
            if (shift > 4) shift = 4;
            if (shift < -4) shift = -4;
            cfg.shift = shift;
        }
        else if (!strcmp(a, "--iq0") || !strcmp(a, "--iqdc") || !strcmp(a, "--noLUT")) {
            fprintf(stderr, "%s (sonde_hip): %s is not supported\n", prog, a);
            return -1;
        }
        else if (!strcmp(a, "--IQ") || !strcmp(a, "--iq")) {
            cfg.opt_iq = !strcmp(a, "--IQ") ? 5 : 6;
            if (++i >= argc) return -1;
            fq = atof(argv[i]);
            if (fq < -0.5) fq = -0.5;
            if (fq > 0.5) fq = 0.5;
        }
        else if (!strcmp(a, "--lpIQ")) cfg.lp_iq = 1;
        else if (!strcmp(a, "--lpbw")) {
            if (++i >= argc) return -1;
            const double bw = atof(argv[i]);
            if (bw > 100.0 && bw < 240.0) lpbw = (float)(bw * 1e3);
            cfg.lp_iq = 1;
        }
        else if (!strcmp(a, "--lpFM")) cfg.lp_fm = 1;
        else if (!strcmp(a, "--decFM")) cfg.dec_fm = 4;
        else if (!strcmp(a, "--decFM2")) cfg.dec_fm = 2;
        else if (!strcmp(a, "--decFM1")) cfg.dec_fm = 1;
        else if (!strcmp(a, "--dc")) cfg.dc = 1;
        else if (!strcmp(a, "--min")) cfg.min = 1;
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
    if (!cfg.opt_iq && pcmraw) { fprintf(stderr, "error: raw data not IQ\n"); return -1; }
    if (!pcmraw && wav_read_header(fp, &cfg.sample_rate, &cfg.bits, &nch) < 0) { fprintf(stderr, "error: wav header\n"); return -1; }
    if (!cfg.opt_iq) { fprintf(stderr, "%s (sonde_hip): FM-audio input is not supported\n", prog); return -1; }
    if (cfg.bits == 32) { fprintf(stderr, "%s (sonde_hip): 32-bit samples are not supported\n", prog); return -1; }
    if (nch != 2) { fprintf(stderr, "error: init buffers\n"); return -1; }
    if (cfreq > 0) po.jsn_freq_khz = (int)((cfreq + fq * cfg.sample_rate + 500) / 1e3);      /* xlt_fq = -fq (:2179, :2270) */
    json_version(po.version, sizeof po.version);
    cfg.lpbw_hz = (int)(float)lpbw;
    cfg.thres = thres;
    cfg.baud = baud;

    int chunk_max = cfg.sample_rate / 4 > 0 ? cfg.sample_rate / 4 : 1;           /* <= 0.25 s per call: frames reach auto_rx live */
    sonde_mk2a_t *eng = NULL;
    sonde_mk2a_info_t inf;
    memset(&inf, 0, sizeof inf);
    int rc = sonde_mk2a_create(&cfg, 1, &fq, chunk_max, &eng);
    if (rc) { fprintf(stderr, "%s (sonde_hip): engine init failed (%d)\n", prog, rc); return -1; }
    sonde_mk2a_info(eng, &inf);
    {
        /* stderr of main and init_buffers_Lband: the note on the sliced rate, "sps corr", IF / dec */
        const float sps0 = (float)cfg.sample_rate / 9616.0f / (float)inf.dec_fm;
        if (sps0 < 8) fprintf(stderr, "note: sample rate low (%.1f sps)\n", sps0);
        if (baud > 0) fprintf(stderr, "sps corr: %.4f\n", (float)cfg.sample_rate / baud);
        fprintf(stderr, "IF: %d\n", inf.if_rate);
        fprintf(stderr, "dec: %d\n", inf.dec_m);
    }
    const int decM = inf.dec_m;
    chunk_max -= chunk_max % decM;                                                 /* whole IF samples per call (the engine's rule) */
    po.show_df = cfg.dc;
    po.if_rate = inf.if_rate;
    po.sample_rate = cfg.sample_rate;
    sonde_mk2a_printer_t *pr = NULL;
    if (sonde_mk2a_printer_create(&po, &pr)) { sonde_mk2a_destroy(eng); return -1; }

    const size_t frame_bytes = (size_t)(cfg.bits / 8) * 2;
    unsigned char *raw = malloc(frame_bytes * chunk_max);
    static sonde_mk2a_frame_t fr[8];
    static char text[1 << 16];
    int status = 0, eof = 0;
    if (!raw) status = -1;
    while (!status) {
        if (!eof) {
            const size_t got_all = fread(raw, frame_bytes, chunk_max, fp);
            const size_t got = got_all - got_all % decM;         /* a partial decimation block at the end is dropped, as by the reference */
            if (got > 0) {
                rc = sonde_mk2a_process_host(eng, raw, (int)got);
                if (rc) { fprintf(stderr, "%s (sonde_hip): engine failure (%d)\n", prog, rc); status = -1; break; }
            }
            if (got_all < (size_t)chunk_max) {
                eof = 1;
                if (sonde_mk2a_finish(eng)) { status = -1; break; }
            }
        }
        int nf;
        while ((nf = sonde_mk2a_fetch_frames(eng, fr, 8)) > 0) {
            for (int k = 0; k < nf; k++) {
                const int len = sonde_mk2a_print_frame(pr, fr[k].bits, fr[k].nbits, fr[k].mv, fr[k].df, text, sizeof text);
                if (len > 0) fwrite(text, 1, len, stdout);
                fflush(stdout);
            }
        }
        if (eof) break;
    }
    if (!status) fprintf(stdout, "\n");
    fflush(stdout);
    free(raw);
    sonde_mk2a_printer_destroy(pr);
    sonde_mk2a_destroy(eng);
    if (fp != stdin) fclose(fp);
    return status;
}
