/*
 * host/rd94rd41drop.c — Vaisala RD94 / RD41 dropsonde decoder with the reference's dropsonde/rd94rd41drop.c contract, on libsonde_hip.
 *
 * argv  : -h, -v, -vv, -r, -R, -i, --rawhex, --rd41, --rd94, --json, --jsn_cfq <Hz>, -b, --br <Bd>, --softin, --softinv, a file name;
 *         stdin without one.  Anything else is taken for a file name, as by the reference.
 * stdin : a WAV stream of FM samples (8 / 16 bits, first channel) — what `iq_dec --FM --lpFM --wav --bo 16` writes —, with --softin /
 *         --softinv raw float32 soft bits, one per raw bit (what `fsk_demod -s` writes), or with --rawhex lines of hex bytes
 * stdout: what the reference prints per frame (sonde_drop_print_frame), flushed per frame
 * stderr: the WAV header lines, "samples/bit:" and with --br "corr:"
 * exit  : 0 at EOF, 255 on argument / input / init errors.  The WAV form runs the FM form of the GPU engine; without a GPU it exits with
 *         255 (there is no CPU fallback).  --softin, --softinv and --rawhex are host code and need none.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sonde_hip.h"
#include "sonde_drop.h"
#include "wav_header.h"

static void json_version(char *dst, size_t cap) {
    const char *ver = getenv("SONDE_JSN_VERSION");
#ifdef VER_JSN_STR
    if (!ver) ver = VER_JSN_STR;
#endif
    if (ver && cap) { strncpy(dst, ver, cap - 1); dst[cap - 1] = 0; }
}

static sonde_drop_printer_t *pr;

static void print(const uint8_t *bytes) {
    static char text[1 << 12];
    const int len = sonde_drop_print_frame(pr, bytes, text, sizeof text);
    if (len > 0) fwrite(text, 1, len, stdout);
    fflush(stdout);
}

int main(int argc, char **argv) {
    sonde_drop_cfg_t cfg;
    sonde_drop_opts_t po;
    memset(&cfg, 0, sizeof cfg);
    memset(&po, 0, sizeof po);
    int softin = 0, rawin = 0, cfreq = -1, nch = 1, inv = 0;
    float baudrate = -1;
    FILE *fp = NULL;
    const char *prog = argv[0];

    for (int i = 1; i < argc && !fp; i++) {
        const char *a = argv[i];
        if (!strcmp(a, "-h") || !strcmp(a, "--help")) {
            fprintf(stderr, "%s [options] <file>\n", prog);
            fprintf(stderr, "  file: audio.wav or raw_data\n");
            fprintf(stderr, "  options:\n");
            fprintf(stderr, "       -v,        (verbose)\n");
            fprintf(stderr, "       -r,        (output: rawbytes)\n");
            fprintf(stderr, "       -R,        (output: raw_bytes)\n");
            fprintf(stderr, "       -i         (invert polarity)\n");
            fprintf(stderr, "       --rawhex   (input: bytes)\n");
            return 0;
        }
        else if (!strcmp(a, "-v")) po.vbs = 1;
        else if (!strcmp(a, "-vv")) po.vbs = 2;
        else if (!strcmp(a, "-r")) po.raw = 1;
        else if (!strcmp(a, "-R")) po.raw = 2;
        else if (!strcmp(a, "-i")) inv = 1;
        else if (!strcmp(a, "--rawhex")) rawin = 2;
        else if (!strcmp(a, "--rd41")) po.type = 41;
        else if (!strcmp(a, "--rd94")) po.type = 94;
        else if (!strcmp(a, "--json")) po.json = 1;
        else if (!strcmp(a, "--jsn_cfq")) {
            if (++i >= argc) return -1;
            int frq = atoi(argv[i]);
            if (frq < 300000000) frq = -1;
            cfreq = frq;
        }
        else if (!strcmp(a, "-b")) cfg.opt_b = 1;
        else if (!strcmp(a, "--br")) {
            if (++i >= argc) return -1;
            baudrate = atof(argv[i]);
            if (baudrate < 4700 || baudrate > 4900) baudrate = 4800;
        }
        else if (!strcmp(a, "--softin")) softin = 1;
        else if (!strcmp(a, "--softinv")) softin = 2;
        else {
            fp = fopen(a, rawin ? "r" : "rb");
            if (!fp) { fprintf(stderr, "error open %s\n", a); return -1; }
        }
    }
    if (!fp) fp = stdin;
    if (cfreq > 0) po.jsn_freq_khz = (cfreq + 500) / 1000;
    json_version(po.version, sizeof po.version);
    if (sonde_drop_printer_create(&po, &pr)) { if (fp != stdin) fclose(fp); return -1; }
    int status = 0;

    if (rawin) {
        static char line[2 * SONDE_DROP_FRAME_LEN + 4];
        static uint8_t bytes[SONDE_DROP_FRAME_LEN];
        while (fgets(line, sizeof line, fp))
            if (sonde_drop_rawhex(line, bytes) == 1) print(bytes);
    } else if (softin) {
        sonde_drop_softin_t *si = NULL;
        if (sonde_drop_softin_create((softin == 2) ^ inv, &si)) { sonde_drop_printer_destroy(pr); if (fp != stdin) fclose(fp); return -1; }
        static float soft[4096];
        static sonde_drop_frame_t fr[16];
        size_t got;
        while ((got = fread(soft, 4, 4096, fp)) > 0) {
            int nf = sonde_drop_softin_push(si, soft, (int)got, fr, 16);
            while (nf > 0) {
                for (int k = 0; k < nf; k++) print(fr[k].bytes);
                nf = sonde_drop_softin_push(si, NULL, 0, fr, 16);
            }
        }
        sonde_drop_softin_destroy(si);
    } else {
        if (wav_read_header(fp, &cfg.sample_rate, &cfg.bits, &nch) < 0 || (cfg.bits != 8 && cfg.bits != 16)) { sonde_drop_printer_destroy(pr); fclose(fp); return -1; }
        fprintf(stderr, "samples/bit: %.2f\n", cfg.sample_rate / (float)4800);
        if (baudrate > 0) { cfg.baud = baudrate; fprintf(stderr, "corr: %.4f\n", cfg.sample_rate / baudrate); }
        cfg.input = SONDE_DROP_IN_FM;
        cfg.invert = inv;
        const int chunk_max = cfg.sample_rate / 4 > 0 ? cfg.sample_rate / 4 : 1;    /* <= 0.25 s per call: frames reach auto_rx live */
        sonde_drop_t *eng = NULL;
        const int rc0 = sonde_drop_create(&cfg, 1, NULL, chunk_max, &eng);
        if (nch < 1) fprintf(stderr, "%s (sonde_hip): a WAV stream without channels is not supported\n", prog);
        if (rc0) fprintf(stderr, "%s (sonde_hip): engine init failed (%d)\n", prog, rc0);
        if (nch < 1 || rc0) { if (eng) sonde_drop_destroy(eng); sonde_drop_printer_destroy(pr); if (fp != stdin) fclose(fp); return -1; }
        const size_t width = (size_t)cfg.bits / 8, stride = width * (size_t)nch;
        unsigned char *raw = malloc(stride * chunk_max), *mono = malloc(width * chunk_max);
        static sonde_drop_frame_t fr[8];
        int eof = 0;
        if (!raw || !mono) status = -1;
        while (!status) {
            const size_t got = fread(raw, stride, chunk_max, fp);        /* whole sample frames only: a partial one is EOF (:182-193) */
            for (size_t k = 0; k < got; k++) memcpy(mono + k * width, raw + k * stride, width);       /* first channel */
            if (got > 0) {
                const int rc = sonde_drop_process_host(eng, mono, (int)got);
                if (rc) { fprintf(stderr, "%s (sonde_hip): engine failure (%d)\n", prog, rc); status = -1; break; }
            }
            if (got < (size_t)chunk_max) {
                eof = 1;
                if (sonde_drop_finish(eng)) { status = -1; break; }
            }
            int nf;
            while ((nf = sonde_drop_fetch_frames(eng, fr, 8)) > 0)
                for (int k = 0; k < nf; k++) print(fr[k].bytes);
            if (eof) break;
        }
        free(raw); free(mono);
        sonde_drop_destroy(eng);
    }
    fflush(stdout);
    sonde_drop_printer_destroy(pr);
    if (fp != stdin) fclose(fp);
    return status;
}
