// sonde_design.cpp — host-side filter / table design of the engine (product code, no oracle dependency).
//
// Reproduces the numbers init_buffers() derives (reference demod/mod/demod_mod.c:1208-1474) with the same
// float/double evaluation order, because the taps, the mixer table and the header template are *data* the
// GPU kernels must share with the reference to stay inside the soft-bit tolerance:
//   design_lowpass   Blackman x sinc, 1-norm, float accumulate            demod_mod.c:555-587
//   dup_taps         a tap set twice in a row (+ one 0): the form the single-sonde kernels' ring FIRs read
//   design_decimator IF rate / decM / tap count                            demod_mod.c:1222-1259
//   design_mixer     16-Hz-snapped mixer frequency + table period           demod_mod.c:1262-1296
//   design_match     Gaussian-pulse header template, 2-norm                demod_mod.c:1190-1195,1398-1421
//   design_imet4     imet4iq's IF rate / decM, IF tap sets, FM low-pass    imet4iq.c:600-646,692-741
//   design_mk2a      mk2a1680mod's L-band rates, tap sets, K/L/M, template   mk2a1680mod.c:1141-1442,2285-2343
#include "sonde_host.h"
#include <cmath>

namespace sonde {

static const double kTwoPi = 6.2831853071795864769252867665590;

std::vector<float> design_lowpass(float f, int taps) {
    if (taps % 2 == 0) taps++;
    if (taps < 1) taps = 1;
    std::vector<float> ws(taps);
    double norm = 0.0;
    const int centre = (taps - 1) / 2;
    const float twof = 2 * f;
    for (int n = 0; n < taps; n++) {
        const double w = 7938 / 18608.0 - 9240 / 18608.0 * std::cos(kTwoPi * n / (taps - 1))
                       + 1430 / 18608.0 * std::cos(4 * M_PI * n / (taps - 1));
        const double x = (double)(twof * (float)(n - centre));
        const double sinc = (x == 0) ? 1.0 : std::sin(M_PI * x) / (M_PI * x);
        ws[n] = (float)(w * (twof * sinc));
        norm += ws[n];
    }
    for (int n = 0; n < taps; n++) ws[n] = (float)(ws[n] / norm);
    return ws;
}

std::vector<float> dup_taps(const std::vector<float> &w) {
    std::vector<float> d(2 * w.size() + 1, 0.f);
    for (size_t i = 0; i < w.size(); i++) d[i] = d[w.size() + i] = w[i];
    return d;
}

Decimator design_decimator(int sr_base, bool if_min) {
    Decimator d;
    int if_sr = if_min ? 32000 : 48000;
    d.decM = 1;
    if (if_sr > sr_base) if_sr = sr_base;
    if (if_sr < sr_base) {
        while (sr_base % if_sr) if_sr += 1;
        d.decM = sr_base / if_sr;
    }
    const float f_lp = (float)((if_sr + 20e3) / (4.0 * sr_base));
    float t_bw = (float)(if_sr - 20e3);
    if (if_min) t_bw = (float)(if_sr - 12e3);
    if (t_bw < 0) t_bw = 10e3f;
    t_bw /= sr_base;
    int taps = (int)(4.0 / t_bw);
    if (taps % 2 == 0) taps++;
    d.if_sr = if_sr;
    d.taps = design_lowpass(f_lp, taps);
    return d;
}

// dft_detect's variant (dft_detect.c:1021-1067): --bw above 48 kHz raises the IF rate to that bandwidth; an IF above 60 kHz ("wideIF") gets a wider
// pass band and transition (IF + 60 kHz, IF - 60 kHz)
Decimator design_decimator_scan(int sr_base, bool if_min, float set_lpIQ) {
    Decimator d;
    int if_sr = 48000;
    if (set_lpIQ > (float)if_sr) if_sr = (int)set_lpIQ;
    const bool wide = if_sr > 60e3;
    if (if_min) if_sr = 32000;
    d.decM = 1;
    if (if_sr > sr_base) if_sr = sr_base;
    if (if_sr < sr_base) {
        while (sr_base % if_sr) if_sr += 1;
        d.decM = sr_base / if_sr;
    }
    float f_lp = (float)((if_sr + 20e3) / (4.0 * sr_base));
    float t_bw = (float)(if_sr - 20e3);
    if (wide) { f_lp = (float)((if_sr + 60e3) / (4.0 * sr_base)); t_bw = (float)(if_sr - 60e3); }
    else if (if_min) t_bw = (float)(if_sr - 12e3);
    if (t_bw < 0) t_bw = 10e3f;
    t_bw /= sr_base;
    int taps = (int)(4.0 / t_bw);
    if (taps % 2 == 0) taps++;
    d.if_sr = if_sr;
    d.taps = design_lowpass(f_lp, taps);
    return d;
}

// iq_dec's variant (iq_dec.c:632-666): the IF rate is a parameter (--IFbw), --min only narrows the transition band
Decimator design_decimator_if(int sr_base, int if_target, bool narrow) {
    Decimator d;
    int if_sr = if_target;
    d.decM = 1;
    if (if_sr > sr_base) if_sr = sr_base;
    if (if_sr < sr_base) {
        while (sr_base % if_sr) if_sr += 1;
        d.decM = sr_base / if_sr;
    }
    const float f_lp = (float)((if_sr + 20e3) / (4.0 * sr_base));
    float t_bw = (float)(if_sr - 20e3);
    if (narrow) t_bw = (float)(if_sr - 12e3);
    if (t_bw < 0) t_bw = 10e3f;
    t_bw /= sr_base;
    int taps = (int)(4.0 / t_bw);
    if (taps % 2 == 0) taps++;
    d.if_sr = if_sr;
    d.taps = design_lowpass(f_lp, taps);
    return d;
}

// Mixer: the reference snaps the frequency to a multiple of d Hz (d = largest divisor <= 16 of the sample rate)
// and tabulates ex[n] = cexp(2 pi i * fl32(f0*n)) over one period lut_len = sr/d.  The kernels evaluate the
// same expression on the fly, so only (f0, lut_len) are needed.
Mixer design_mixer(double xlt_fq, int sr_base) {
    const int W = 16;
    int d;
    const int freq = (int)(xlt_fq * (double)sr_base + 0.5);
    int freq0 = freq;
    for (d = W; d > 0; d--) if (sr_base % d == 0) break;
    if (d == 0) d = 1;
    for (int k = 0; k < W / 2; k++) {
        if ((freq + k) % d == 0) { freq0 = freq + k; break; }
        if ((freq - k) % d == 0) { freq0 = freq - k; break; }
    }
    Mixer m;
    m.lut_len = sr_base / d;
    m.f0 = freq0 / (double)sr_base;
    return m;
}

static double gauss_q(double x) { return 0.5 - 0.5 * std::erf(x / 1.4142135624); }
static double gauss_pulse(double t, double sigma) { return gauss_q((t - 0.5) / sigma) - gauss_q((t + 0.5) / sigma); }

std::vector<float> design_match(const std::string &hdr, float sps, float bt) {
    const int hdrlen = (int)hdr.size();
    const int L = (int)(hdrlen * sps + 0.5);
    std::vector<float> m(L);
    const double sigma = std::sqrt(std::log(2)) / (kTwoPi * bt);
    for (int i = 0; i < L; i++) {
        const int pos = (int)(i / sps);
        const float t = (float)((i - pos * sps) / sps - 0.5);
        const float b1 = (float)(((hdr[pos] & 1) - 0.5) * 2.0);
        float b = (float)(b1 * gauss_pulse(t, sigma));
        if (pos > 0) {
            const float b0 = (float)(((hdr[pos - 1] & 1) - 0.5) * 2.0);
            b = (float)(b + b0 * gauss_pulse((double)(t + 1), sigma));
        }
        if (pos < hdrlen - 1) {
            const float b2 = (float)(((hdr[pos + 1] & 1) - 0.5) * 2.0);
            b = (float)(b + b2 * gauss_pulse((double)(t - 1), sigma));
        }
        m[i] = b;
    }
    double n2 = 0.0;
    for (int i = 0; i < L; i++) { const double x = m[i]; n2 += x * x; }
    const float nm = (float)std::sqrt(n2);
    for (int i = 0; i < L; i++) m[i] /= nm;
    return m;
}

// Consumed-sample window of one bit half; host twin of bit_window() in sonde_kernels.hip
// (read_softbit2p, demod_mod.c:1098-1161).
void bit_window(int pos, int half, int symlen, float sps, uint32_t &q0, uint32_t &q1, double &mid) {
    double bg = (pos == 0) ? 0.0 : (double)((float)(pos * symlen) * sps);
    double prev;
    if (half == 0) {
        if (pos == 0) prev = 0.0;
        else {
            prev = (pos == 1) ? 0.0 : (double)((float)((pos - 1) * symlen) * sps);
            prev += (double)sps;
            if (symlen == 2) prev += (double)sps;
        }
    } else {
        bg += (double)sps;
        prev = bg;
    }
    q0 = (uint32_t)std::ceil(prev);
    mid = bg + (double)(sps - 1.0f) / 2.0;
    q1 = (uint32_t)std::ceil(bg + (double)sps);
    if (q1 <= q0) q1 = q0 + 1;
}

// Range [qa, qb) of consumed-sample counts a symbol half actually sums: q in [q0, q1) with mid-l < q < mid+l
// (everything for l < 0) — the `if (l < 0 || (mid-l < dsp->sc && dsp->sc < mid+l))` of read_softbit2p.
void slice_range(uint32_t q0, uint32_t q1, double mid, float l, uint32_t &qa, uint32_t &qb) {
    qa = q0; qb = q1;
    if (!(l < 0.f)) {
        const double lo = mid - (double)l, hi = mid + (double)l;
        const double fa = std::floor(lo) + 1.0, fb = std::ceil(hi);      // smallest q > lo, smallest q >= hi
        if (fa > (double)qa) qa = (uint32_t)fa;
        if (fb < (double)qb) qb = (fb > 0.0) ? (uint32_t)fb : 0u;
    }
    if (qb < qa) qb = qa;
}

// imet4iq's variant of the front-end design: its own IF rate rule (48 kHz, 32 kHz with --min, doubled with --imet1; decM from the
// same search as demod_mod; FM audio stays at its rate) and decimator taps, the IF low-pass as an acquisition set at 1.5x the bandwidth plus the nominal set (both of the nominal
// set's odd tap count), and the 6 kHz FM low-pass with its own tap rule (halved above 100 kHz).
Imet4Design design_imet4(int sr_base, bool iq, bool if_min, bool imet1, float lpiq_bw) {
    Imet4Design d;
    int if_sr = if_min ? 32000 : 48000;
    if (imet1) if_sr *= 2;
    d.decM = 1;
    if (!iq) if_sr = sr_base;                 // FM audio: every filter at the input rate
    if (if_sr > sr_base) if_sr = sr_base;
    if (if_sr < sr_base) {
        while (sr_base % if_sr) if_sr += 1;
        d.decM = sr_base / if_sr;
    }
    if (d.decM > 1) {                         // the decimator's own design, imet4iq.c:618-635
        float f_lp = (float)((if_sr + 20e3) / (4.0 * sr_base));
        float t_bw = (float)(if_sr - 20e3);
        if (imet1) { f_lp = (float)((if_sr + 80e3) / (4.0 * sr_base)); t_bw = (float)(if_sr - 80e3); }
        if (if_min) {
            t_bw = (float)(if_sr - 12e3);
            if (imet1) { f_lp = (float)((if_sr + 60e3) / (4.0 * sr_base)); t_bw = (float)((if_sr - 60e3) / 2); }
        }
        if (t_bw < 0) t_bw = 10e3f;
        t_bw /= sr_base;
        int taps = (int)(4.0 / t_bw);
        if (taps % 2 == 0) taps++;
        d.lp_dec = design_lowpass(f_lp, taps);
    }
    d.if_sr = if_sr;
    const int sr = if_sr;
    const float f_lp = (float)(lpiq_bw / (float)sr / 2.0);
    int taps = (int)(4 * sr / 4e3);
    if (taps % 2 == 0) taps++;
    d.lp_iq0 = design_lowpass((float)(1.5 * f_lp), taps);
    d.lp_iq1 = design_lowpass(f_lp, (int)d.lp_iq0.size());
    const float f_fm = 6e3f / (float)sr;
    int tfm = (int)(4 * sr / 2e3);
    if (tfm % 2 == 0) tfm++;
    if (sr > 100e3) tfm = tfm / 2;
    if (tfm % 2 == 0) tfm++;
    d.lp_fm = design_lowpass(f_fm, tfm);
    return d;
}

// mk2a1680mod: main's option handling (:2285-2343) and init_buffers_Lband (:1141-1442).  The L-band copy of the demod DSP has its own rules:
// designated IF 4 x 48 kHz (4 x 32 kHz with --min) raised to a divisor of the input rate, decimator pass band (IF + 60 kHz) / 4 and
// transition IF - 180 kHz, IF low-pass of 4 sr / 8 kHz taps halved above 100 and again above 200 kHz in an acquisition (1.5 x) and a nominal
// set, FM low-pass 6.8 kHz (--iq) / 8 kHz (--IQ) doubled and shortened under --decFM, the IQFM low-pass of --IQ --decFM, N forced to 8192,
// K <= 790 bits (the header distance), and the header template with t in double.
Mk2aDesign design_mk2a(int sr_base, int opt_iq, bool lp_iq, float lpiq_bw, bool lp_fm, int opt_decFM, bool dc, bool if_min, float baud, int shift) {
    Mk2aDesign d;
    int lp = (lp_iq ? 1 : 0) | (lp_fm ? 2 : 0);
    if (opt_decFM) {
        lp |= opt_iq == 5 ? 4 : 2;
        if (sr_base > 4 * 44000) d.fmdec = 1;
    }
    float sps = (float)sr_base / 9616.0f;
    d.decFM = 1;
    if (d.fmdec) {
        d.decFM = opt_decFM;
        while (sr_base % d.decFM > 0 && d.decFM > 1) d.decFM /= 2;
        sps /= (float)d.decFM;
    }
    if (opt_iq == 5 && dc) lp |= 2;
    d.lp = lp;
    const int lpIQ_bw = (int)lpiq_bw;
    const int lpFM_bw = opt_iq == 6 ? (int)6.8e3 : (int)8e3;
    if (baud > 0) sps = (float)sr_base / baud;                        // (:2321-2325: the FM decimation is not taken into account again)
    // decimator (:1157-1194)
    int if_sr = if_min ? 32000 * 4 : 48000 * 4;
    d.decM = 1;
    if (if_sr > sr_base) if_sr = sr_base;
    if (if_sr < sr_base) {
        while (sr_base % if_sr) if_sr += 1;
        d.decM = sr_base / if_sr;
    }
    if (d.decM > 1) {
        const float f_lp = (float)((if_sr + 60e3) / (4.0 * sr_base));
        float t_bw = (float)(if_sr - 180e3);
        if (if_min) t_bw = (float)(if_sr - 80e3);
        if (t_bw < 0) t_bw = 160e3f;
        t_bw /= sr_base;
        int taps = (int)(4.0 / t_bw);
        if (taps % 2 == 0) taps++;
        d.lp_dec = design_lowpass(f_lp, taps);
    }
    d.if_sr = if_sr;
    const int sr = if_sr;
    sps /= (float)d.decM;
    d.sps = sps;
    if (lp & 1) {                                                     // IF low-pass (:1241-1267)
        float f_lp = (float)(160e3 / (float)sr / 2.0);
        if (lpIQ_bw) f_lp = (float)(lpIQ_bw / (float)sr / 2.0);
        int taps = (int)(4 * sr / 8e3);
        if (sr > 100e3) taps = taps / 2;
        if (sr > 200e3) taps = taps / 2;
        if (taps % 2 == 0) taps++;
        d.lp_iq0 = design_lowpass((float)(1.5 * f_lp), taps);
        d.lp_iq1 = design_lowpass(f_lp, (int)d.lp_iq0.size());
    }
    if (lp & 2) {                                                     // FM low-pass (:1270-1292)
        float f_lp = (float)(10e3 / (float)sr);
        if (lpFM_bw > 0) f_lp = lpFM_bw / (float)sr;
        int taps = (int)(4 * sr / 4e3);
        if (d.decFM > 1) { f_lp *= 2; taps = taps / 2; }
        if (sr > 100e3) taps = taps / 2;
        if (sr > 200e3) taps = taps / 2;
        if (opt_iq == 5) taps = taps / 2;
        if (taps % 2 == 0) taps++;
        d.lp_fm = design_lowpass(f_lp, taps);
    }
    if (lp & 4) {                                                     // IQFM low-pass (:1295-1318)
        float f_lp = (float)(10e3 / (float)sr);
        int taps = (int)(4 * sr / 4e3);
        f_lp = (float)(f_lp * (2.0 * 2));
        taps = taps / 2;
        if (sr > 100e3) taps = taps / 2;
        if (sr > 200e3) taps = taps / 2;
        taps = taps / 2;
        taps = taps / 2;
        if (taps % 2 == 0) taps++;
        d.lp_iqfm = design_lowpass(f_lp, taps);
    }
    // header window (:1330-1353)
    const int hdrlen = 50;
    const int L = (int)(hdrlen * sps + 0.5);
    int M = 3 * L;
    d.delay = L / 16;
    int p2 = 1;
    while (p2 < M) p2 <<= 1;
    while (p2 < 0x2000) p2 <<= 1;
    M = p2;
    int K = M - L - d.delay;
    while (K > 790 * sps) K--;
    d.L = L; d.M = M; d.N = p2; d.K = K;
    // header template (:1366-1389): CA CA CA 24 52 in 8N1, BT = 1.0, t in double
    static const char hdr[] = "0010100111" "0010100111" "0010100111" "0001001001" "0010010101";
    const double sigma = std::sqrt(std::log(2)) / (kTwoPi * 1.0f);
    d.match.resize(L);
    for (int i = 0; i < L; i++) {
        const int pos = (int)(i / sps);
        const double t = (i - pos * sps) / sps - 0.5;
        const float b1 = (float)(((hdr[pos] & 1) - 0.5) * 2.0);
        float b = (float)(b1 * gauss_pulse(t, sigma));
        if (pos > 0) {
            const float b0 = (float)(((hdr[pos - 1] & 1) - 0.5) * 2.0);
            b = (float)(b + b0 * gauss_pulse(t + 1, sigma));
        }
        if (pos < hdrlen - 1) {
            const float b2 = (float)(((hdr[pos + 1] & 1) - 0.5) * 2.0);
            b = (float)(b + b2 * gauss_pulse(t - 1, sigma));
        }
        d.match[i] = b;
    }
    double n2 = 0.0;
    for (int i = 0; i < L; i++) { const double x = d.match[i]; n2 += x * x; }
    const float nm = (float)std::sqrt(n2);
    for (int i = 0; i < L; i++) d.match[i] /= nm;
    // --IQ tone correlator (:881-902, :1433-1439)
    d.f1 = -(d.h * sr) / (2.0 * sps);
    d.tone_sps = sps * d.decFM;
    {
        int n = (int)d.tone_sps;
        const float sk = d.tone_sps / 2.4f;
        while (n > 0) {
            n--;
            if (n > sk && n < d.tone_sps - sk) d.tone_n.push_back(n);
        }
    }
    // header dc offset of the --IQ form while locked (:465)
    d.mp_ofs = (int)(((int)d.lp_fm.size() - (int)d.lp_iqfm.size() - (sps - 1)) / (2 * d.decFM));
    // main (:2339-2343)
    d.bitofs = (d.fmdec ? 0 : 1) + shift;
    float bl = (float)(0.7 * sps / 2.0);
    if (bl < 2.0) bl = -1;
    if (d.fmdec) bl = -1;
    d.bl = bl;
    return d;
}

}  // namespace sonde
