/*
 * host/sonde_power.c — `rtl_power` command line on top of libsonde_hip's spectrum survey (C).
 *
 * Contract kept: the call auto_rx issues (auto_rx/autorx/sdr_wrappers.py:649-658)
 *     rtl_power [-T] -p <ppm> -d <device> [-g <gain>] -f <start>:<stop>:<step> -i <seconds> -1 -c 25% <logfile>
 * and the log line its readers parse (read_rtl_power_log, scan.py read_rtl_power):
 *     date, time, Hz low, Hz high, Hz step, samples, dB, dB, ...
 * with Hz low / Hz high the centres of the first and last bin written.  -p, -d, -g, -T are accepted and ignored: there is no tuner here.
 * The IQ stream that is already there is named beside it:
 *     --input PATH|-   --cfreq Hz   --sr Hz   --bits 8|16|32        (or SONDE_POWER_INPUT / _CFREQ / _SR / _BITS in the environment,
 * so that auto_rx's fixed command line works with rtl_power_path pointed at this binary).
 *     -w hann|rectangle   window (rtl_power's default: rectangle)
 * The transform length is the smallest power of two with sr / nfft <= step (rtl_power's rule), at least 256; more than 16384 points is an
 * argument error.  Written are the bins of the cropped spectrum whose centres lie in [start, stop].
 * -1: read -i seconds of samples, write one line, exit 0.  Without it: one line per interval until the input ends.
 * Exit codes: 0 ok; 1 the input ended before one whole segment (nothing is written); 2 bad arguments, or [start, stop] does not overlap the
 * stream; 3 the engine failed (no GPU: there is no CPU fallback).
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <time.h>
#include "sonde_power.h"

static const char *opt_or_env(const char *opt, const char *env) { return opt ? opt : getenv(env); }

static int usage(const char *msg) {
    fprintf(stderr, "sonde_power: %s\nusage: sonde_power -f start:stop:step -i seconds [-1] [-c crop%%] [-w hann|rectangle] [--input PATH|-] [--cfreq Hz] [--sr Hz] [--bits 8|16|32] <logfile|->\n", msg);
    return 2;
}

int main(int argc, char **argv) {
    const char *o_input = NULL, *o_cfreq = NULL, *o_sr = NULL, *o_bits = NULL, *o_f = NULL, *logname = NULL;
    double interval = 10.0, crop = 0.0;
    int single = 0, window = SONDE_POWER_RECT;
    for (int i = 1; i < argc; i++) {
        const char *a = argv[i];
        if (!strcmp(a, "-1")) single = 1;
        else if (!strcmp(a, "-T")) { }
        else if (!strcmp(a, "-p") || !strcmp(a, "-d") || !strcmp(a, "-g")) { if (++i >= argc) return usage("option needs a value"); }
        else if (!strcmp(a, "-f")) { if (++i >= argc) return usage("-f needs start:stop:step"); o_f = argv[i]; }
        else if (!strcmp(a, "-i")) {
            if (++i >= argc) return usage("-i needs a time");
            char *end; interval = strtod(argv[i], &end);
            if (*end == 'm') interval *= 60.0; else if (*end == 'h') interval *= 3600.0;
        }
        else if (!strcmp(a, "-c")) { if (++i >= argc) return usage("-c needs a fraction"); char *end; crop = strtod(argv[i], &end); if (*end == '%') crop /= 100.0; }
        else if (!strcmp(a, "-w")) {
            if (++i >= argc) return usage("-w needs a window");
            if (!strncmp(argv[i], "hann", 4)) window = SONDE_POWER_HANN; else if (!strncmp(argv[i], "rect", 4)) window = SONDE_POWER_RECT; else return usage("unknown window");
        }
        else if (!strcmp(a, "--input")) { if (++i >= argc) return usage("--input needs a path"); o_input = argv[i]; }
        else if (!strcmp(a, "--cfreq")) { if (++i >= argc) return usage("--cfreq needs a frequency"); o_cfreq = argv[i]; }
        else if (!strcmp(a, "--sr")) { if (++i >= argc) return usage("--sr needs a rate"); o_sr = argv[i]; }
        else if (!strcmp(a, "--bits")) { if (++i >= argc) return usage("--bits needs 8, 16 or 32"); o_bits = argv[i]; }
        else if (a[0] == '-' && a[1] != 0) return usage("illegal option");
        else logname = a;
    }
    const char *s_input = opt_or_env(o_input, "SONDE_POWER_INPUT"), *s_cfreq = opt_or_env(o_cfreq, "SONDE_POWER_CFREQ");
    const char *s_sr = opt_or_env(o_sr, "SONDE_POWER_SR"), *s_bits = opt_or_env(o_bits, "SONDE_POWER_BITS");
    double f_start = 0, f_stop = 0, f_step = 0;
    if (!o_f || sscanf(o_f, "%lf:%lf:%lf", &f_start, &f_stop, &f_step) != 3 || !(f_step > 0) || !(f_stop >= f_start)) return usage("-f start:stop:step is required");
    if (!logname) return usage("no log file named");
    if (!s_sr || !s_cfreq) return usage("the stream's --sr and --cfreq are required");
    const double srd = atof(s_sr), cfreq = atof(s_cfreq);
    const int bits = s_bits ? atoi(s_bits) : 16;
    if (!(srd >= 1.0) || srd > 2e9 || !(interval > 0) || !(crop >= 0) || !(crop < 1) || (bits != 8 && bits != 16 && bits != 32)) return usage("bad value");
    const int sr = (int)(srd + 0.5);
    int nfft = SONDE_POWER_NFFT_MIN;
    while ((double)sr / nfft > f_step && nfft <= SONDE_POWER_NFFT_MAX) nfft *= 2;
    if (nfft > SONDE_POWER_NFFT_MAX) return usage("step too fine for this sample rate: more than 16384 points");

    /* which bins of the cropped spectrum lie in [start, stop] */
    const double step = (double)sr / nfft;
    const int drop = (int)(crop * nfft / 2.0), bins = nfft - 2 * drop;
    const double f_low = cfreq + (double)(drop - nfft / 2) * step;
    int i0 = (int)ceil((f_start - f_low) / step - 1e-6), i1 = (int)floor((f_stop - f_low) / step + 1e-6);
    if (i0 < 0) i0 = 0;
    if (i1 > bins - 1) i1 = bins - 1;
    if (i1 < i0) { fprintf(stderr, "sonde_power: %.0f .. %.0f Hz does not overlap the stream (%.0f .. %.0f Hz kept)\n", f_start, f_stop, f_low, f_low + (bins - 1) * step); return 2; }

    FILE *in = stdin;
    if (s_input && strcmp(s_input, "-")) { in = fopen(s_input, "rb"); if (!in) { fprintf(stderr, "sonde_power: cannot open %s\n", s_input); return 2; } }

    const int chunk = 1 << 18;
    sonde_power_cfg_t cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.abi_version = SONDE_ABI_VERSION; cfg.n_streams = 1; cfg.sample_rate = sr; cfg.bits = bits; cfg.nfft = nfft; cfg.window = window;
    cfg.max_chunk = chunk; cfg.center_hz = cfreq; cfg.crop = (float)crop;
    sonde_power_t *ps = NULL;
    int rc = sonde_power_create(&cfg, &ps);
    if (rc) { fprintf(stderr, "sonde_power: %s\n", sonde_strerror(rc)); return rc == SONDE_E_ARG ? 2 : 3; }

    const size_t unit = 2 * (size_t)(bits / 8);
    uint8_t *buf = (uint8_t *)malloc((size_t)chunk * unit);
    float *db = (float *)malloc((size_t)bins * sizeof(float));
    const size_t linecap = 96 + (size_t)bins * 12;
    char *line = (char *)malloc(linecap);
    if (!buf || !db || !line) return 3;
    const int64_t per_line = (int64_t)(interval * sr + 0.5);
    FILE *out = NULL;
    int lines = 0, eof = 0, status = 0;
    size_t carry = 0;                                   /* bytes of an incomplete sample at the end of a read */
    while (!eof && status == 0) {
        int64_t left = per_line;
        while (left > 0) {
            const size_t want = (size_t)(left < chunk ? left : chunk) * unit;
            const size_t got = fread(buf + carry, 1, want - carry, in) + carry;
            const int n = (int)(got / unit);
            carry = got - (size_t)n * unit;
            if (n > 0 && (rc = sonde_power_process_host(ps, buf, n, n)) != 0) { fprintf(stderr, "sonde_power: %s\n", sonde_strerror(rc)); status = 3; break; }
            if (carry) memmove(buf, buf + (size_t)n * unit, carry);
            left -= n;
            if (got < want) { eof = 1; break; }
        }
        if (status) break;
        const int64_t segs = sonde_power_segments(ps, 0);
        if (segs < 1) break;                            /* not one whole segment in this interval: no line */
        double st;
        rc = sonde_power_fetch(ps, 0, db, NULL, NULL, &st, bins, 1);
        if (rc < 0) { fprintf(stderr, "sonde_power: %s\n", sonde_strerror(rc)); status = 3; break; }
        const int len = sonde_power_csv_line((int64_t)time(NULL), cfreq + (double)(drop + i0 - nfft / 2) * st, cfreq + (double)(drop + i1 - nfft / 2) * st, st, segs * nfft, db + i0, i1 - i0 + 1, line, linecap);
        if (len < 0 || (size_t)len >= linecap) { status = 3; break; }
        if (!out) { out = strcmp(logname, "-") ? fopen(logname, "w") : stdout; if (!out) { fprintf(stderr, "sonde_power: cannot write %s\n", logname); status = 2; break; } }
        fwrite(line, 1, (size_t)len, out);
        fflush(out);
        lines++;
        if (single) break;
    }
    if (out && out != stdout) fclose(out);
    if (in != stdin) fclose(in);
    sonde_power_destroy(ps);
    free(buf); free(db); free(line);
    if (status) return status;
    return lines ? 0 : 1;
}
