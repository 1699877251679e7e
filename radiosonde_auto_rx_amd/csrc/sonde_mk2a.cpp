// sonde_mk2a.cpp — host side of the LMS6-1680 / MkIIa engine behind include/sonde_mk2a.h (the reference's mk2a/mk2a1680mod.c).
// Design (sonde_design.cpp: design_mk2a, design_mixer, design_lowpass), device state, one k_mk2a_mix + k_mk2a launch per call, the frame queue.
#include "../../include/sonde_mk2a.h"
#include "sonde_frame_engine.h"
#include "sonde_mk2a_dev.h"
#include <cmath>

using namespace sonde;

static sonde_mk2a_frame_t host_frame(const Mk2aFrame &g) {
    sonde_mk2a_frame_t h;
    memset(&h, 0, sizeof h);
    h.channel = g.channel; h.nbits = g.nbits; h.inv = g.inv; h.mv = g.mv; h.df = g.Df; h.mv_pos = g.mv_pos; h.sample = g.sample;
    memcpy(h.bits, g.bits, sizeof h.bits);
    return h;
}

struct sonde_mk2a : FrameEngine<sonde_mk2a_frame_t> {
    Mk2aArgs a{};
    sonde_mk2a_info_t info{};
    int32_t if_last = 0;                 // IF samples per channel of the last call whose kernels ran (the range of the testing tap on ifbuf)

    // one launch pair over n samples per channel at dev_in
    int run(const void *dev_in, int32_t n) {
        Mk2aArgs c = a;
        c.in = dev_in; c.n_base = n; c.n_if = n / c.decM;
        const int rc = launch_drain(c, sonde_launch_mk2a, host_frame);
        if (rc == 0 || rc == SONDE_E_OVERFLOW) if_last = c.n_if;                 // (an overflow loses frames, the samples are written)
        return rc;
    }
};

static Mk2aDesign design_of(const sonde_mk2a_cfg_t *cfg) {
    const float lpbw = cfg->lpbw_hz > 0 ? (float)cfg->lpbw_hz : 180e3f;
    const int shift = std::max(-4, std::min(4, cfg->shift));
    return design_mk2a(cfg->sample_rate, cfg->opt_iq, cfg->lp_iq != 0, lpbw, cfg->lp_fm != 0, cfg->dec_fm, cfg->dc != 0, cfg->min != 0,
                       cfg->baud > 0 ? cfg->baud : -1.f, shift);
}
static void fill_info(const Mk2aDesign &d, sonde_mk2a_info_t &inf) {
    memset(&inf, 0, sizeof inf);
    inf.if_rate = d.if_sr; inf.dec_m = d.decM; inf.dec_fm = d.decFM; inf.L = d.L; inf.M = d.M; inf.K = d.K; inf.N = d.N;
    inf.taps_dec = (int)d.lp_dec.size(); inf.taps_iq = (int)d.lp_iq0.size(); inf.taps_fm = (int)d.lp_fm.size(); inf.taps_iqfm = (int)d.lp_iqfm.size();
    inf.sps = d.sps;
}
static int cfg_ok(const sonde_mk2a_cfg_t *cfg) {
    if (cfg->bits != 8 && cfg->bits != 16) return 0;                             // float32 input: not built
    if (cfg->opt_iq != 5 && cfg->opt_iq != 6) return 0;                          // FM audio, --iq0: not built
    if (cfg->sample_rate < 48000) return 0;
    return cfg->dec_fm == 0 || cfg->dec_fm == 1 || cfg->dec_fm == 2 || cfg->dec_fm == 4;
}

extern "C" int sonde_mk2a_design(const sonde_mk2a_cfg_t *cfg, sonde_mk2a_info_t *info) {
    if (!cfg || !info || !cfg_ok(cfg)) return SONDE_E_ARG;
    fill_info(design_of(cfg), *info);
    return 0;
}

extern "C" int sonde_mk2a_create(const sonde_mk2a_cfg_t *cfg, int32_t n_ch, const double *fq, int32_t max_chunk, sonde_mk2a_t **out) {
    if (!cfg || !out || !fq || n_ch < 1 || max_chunk < 1) return SONDE_E_ARG;
    *out = nullptr;
    if (!cfg_ok(cfg)) return SONDE_E_ARG;
    const Mk2aDesign d = design_of(cfg);
    // what the kernels are built for: the 8192-point window, filters and tone lags inside the history rings
    const int ring = 2 * MK2A_TILE;
    const size_t longest = std::max({d.lp_iq0.size(), d.lp_fm.size(), d.lp_iqfm.size(), (size_t)(d.tone_sps + 1)});
    if (d.N != MK2A_M || d.M != MK2A_M || d.K + d.L > d.N || d.K < 8 || d.L < MK2A_HDRLEN || (int)longest + MK2A_TILE + 8 > ring) return SONDE_E_ARG;
    if (d.delay < d.bitofs || d.sps < 2.f) return SONDE_E_ARG;
    auto pow2 = [](long long v) { long long p = 1; while (p < v) p <<= 1; return p; };
    const long long bring = d.decM > 1 ? pow2(256LL * d.decM + (long long)d.lp_dec.size() + MK2A_THREADS) : 1;
    if (bring > (1 << 20)) return SONDE_E_ARG;
    max_chunk -= max_chunk % d.decM;                                            // calls take whole IF samples
    if (max_chunk < 1) return SONDE_E_RANGE;
    std::unique_ptr<sonde_mk2a> e;
    TRY(engine_new(e));
    Mk2aArgs &a = e->a;
    a.n_ch = n_ch; a.bits = cfg->bits; a.opt_iq = cfg->opt_iq; a.lp = d.lp; a.dc = cfg->dc ? 1 : 0; a.decFM = d.decFM; a.sr = d.if_sr;
    a.K = d.K; a.L = d.L; a.delay = d.delay; a.bitofs = d.bitofs; a.mp_ofs = d.mp_ofs;
    a.sps = d.sps; a.thres = cfg->thres > 0 ? cfg->thres : 0.7f; a.bl = d.bl; a.tone_sps = d.tone_sps;
    a.slice_cap = std::max(1, std::min(MK2A_THREADS, (int)(4096 / d.sps)));     // bits sliced together stay inside half the sample ring
    a.decM = d.decM; a.taps_dec = (int)d.lp_dec.size(); a.taps_iq = (int)d.lp_iq0.size(); a.taps_fm = (int)d.lp_fm.size(); a.taps_iqfm = (int)d.lp_iqfm.size();
    a.ring = ring; a.bring_len = (int)bring; a.if_stride = max_chunk / d.decM;
    e->n_ch = n_ch; e->max_chunk = max_chunk; e->dec_m = d.decM;
    e->in_bytes = (cfg->bits / 8) * 2;
    // frames per channel and call: at most one per correlation window, plus one that was under way
    a.q_cap = n_ch * (a.if_stride / d.decFM / (d.K - 4) + 2);
    fill_info(d, e->info);

    std::vector<Mk2aChan> ch(n_ch);
    for (int c = 0; c < n_ch; c++) {
        Mk2aChan &s = ch[c];
        memset(&s, 0, sizeof s);
        s.inv = cfg->invert ? 1 : 0;
        s.maxlim = (uint32_t)d.if_sr;                                         // IQdc (:1320-1326)
        s.maxcnt = s.maxlim / 32;
        if (d.decM > 1) { s.maxlim *= (uint32_t)d.decM; s.maxcnt *= (uint32_t)d.decM; }
        if (s.maxcnt < 1) s.maxcnt = 1;
        const Mixer m = design_mixer(-std::max(-0.5, std::min(0.5, fq[c])), cfg->sample_rate);
        s.f0 = m.f0; s.lut_len = m.lut_len;
    }
    std::vector<uint8_t> frames((size_t)n_ch * MK2A_FRAME_STRIDE, 0);
    static const uint8_t h2452[MK2A_FRMSTART] = {0,0,0,1,0,0,1,0,0,1, 0,0,1,0,0,1,0,1,0,1};    // header + strlen(header) - FRMSTART (:2365)
    for (int c = 0; c < n_ch; c++) memcpy(&frames[(size_t)c * MK2A_FRAME_STRIDE], h2452, MK2A_FRMSTART);
    // Fm = rdft(time-reversed template) (:1414-1417), natural order and bit-reversed behind it
    std::vector<float> m(2 * MK2A_M, 0.f);
    for (int i = 0; i < d.L; i++) m[2 * (d.L - 1 - i)] = d.match[i];
    ref_dft_8192(m);
    std::vector<float2> Fm(2 * MK2A_M);
    for (int i = 0; i < MK2A_M; i++) {
        Fm[i] = make_float2(m[2 * i], m[2 * i + 1]);
        int r = 0;
        for (int b = 0; b < 13; b++) if (i & (1 << b)) r |= 1 << (12 - b);
        Fm[MK2A_M + i] = make_float2(m[2 * r], m[2 * r + 1]);
    }
    const std::vector<float> twf = ref_twiddle_table();
    std::vector<float2> tw(twf.size() / 2);
    for (size_t k = 0; k < tw.size(); k++) tw[k] = make_float2(twf[2 * k], twf[2 * k + 1]);
    std::vector<Mk2aTone> tone;
    for (int n : d.tone_n) {                                                    // cexp(-t iw), t = -n / sr, iw = 2 pi i f (:897-900)
        const double t = -n / (double)d.if_sr;
        Mk2aTone tn{};
        tn.n = n;
        const double w1 = 6.2831853071795864769252867665590 * d.f1, w2 = 6.2831853071795864769252867665590 * (-d.f1);
        tn.e1r = std::cos((-t) * w1); tn.e1i = std::sin((-t) * w1);
        tn.e2r = std::cos((-t) * w2); tn.e2i = std::sin((-t) * w2);
        tone.push_back(tn);
    }
    a.n_tone = (int)tone.size();

    TRY(e->upload(&a.chan, ch));
    TRY(e->dalloc(&a.zrot, (size_t)n_ch * a.ring));
    TRY(e->dalloc(&a.zlp, (size_t)n_ch * a.ring));
    TRY(e->dalloc(&a.fmr, (size_t)n_ch * a.ring));
    TRY(e->dalloc(&a.sraw, (size_t)n_ch * a.ring));
    TRY(e->dalloc(&a.bring, (size_t)n_ch * a.bring_len));
    TRY(e->dalloc(&a.ifbuf, (size_t)n_ch * a.if_stride));
    TRY(e->dalloc(&a.bufs, (size_t)n_ch * MK2A_M));
    TRY(e->dalloc(&a.fmbuf, (size_t)n_ch * MK2A_M));
    TRY(e->dalloc(&a.Xg, (size_t)n_ch * MK2A_M));
    TRY(e->upload(&a.frames, frames));
    TRY(e->dalloc(&a.q, (size_t)a.q_cap));
    TRY(e->dalloc(&a.q_count, 1));
    TRY(e->upload(&a.ws_iq0, dup_taps(d.lp_iq0)));
    TRY(e->upload(&a.ws_iq1, dup_taps(d.lp_iq1)));
    TRY(e->upload(&a.ws_fm, dup_taps(d.lp_fm)));
    TRY(e->upload(&a.ws_iqfm, dup_taps(d.lp_iqfm)));
    TRY(e->upload(&a.ws_dec, dup_taps(d.lp_dec)));
    TRY(e->upload(&a.Fm, Fm));
    TRY(e->upload(&a.tws, tw));
    TRY(e->upload(&a.tone, tone));
    TRY(e->alloc_input());
    *out = e.release();
    return 0;
}

extern "C" void sonde_mk2a_destroy(sonde_mk2a_t *e) { delete e; }

extern "C" int sonde_mk2a_info(const sonde_mk2a_t *e, sonde_mk2a_info_t *info) {
    if (!e || !info) return SONDE_E_ARG;
    *info = e->info;
    return 0;
}

extern "C" int sonde_mk2a_process_host(sonde_mk2a_t *e, const void *samples, int32_t n) { return engine_process_host(e, samples, n, false); }

extern "C" int sonde_mk2a_process_device(sonde_mk2a_t *e, const void *dev_samples, int32_t n) { return engine_process_device(e, dev_samples, n); }

// EOF inside a frame: read_softbit2p returns EOF, the loop of main breaks and print_frame gets the bits so far (:2409-2424)
extern "C" int sonde_mk2a_finish(sonde_mk2a_t *e) {
    if (!e) return SONDE_E_ARG;
    if (e->finished) return 0;
    e->finished = 1;
    const int n_ch = e->a.n_ch;
    std::vector<Mk2aChan> ch(n_ch);
    std::vector<uint8_t> frames((size_t)n_ch * MK2A_FRAME_STRIDE);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(ch.data(), e->a.chan, ch.size() * sizeof(Mk2aChan), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(frames.data(), e->a.frames, frames.size(), hipMemcpyDeviceToHost));
    for (int c = 0; c < n_ch; c++) {
        if (ch[c].mode != 1) continue;
        Mk2aFrame g;
        memset(&g, 0, sizeof g);
        g.channel = c; g.nbits = MK2A_FRMSTART + ch[c].bitpos; g.inv = ch[c].inv; g.mv = ch[c].mv; g.Df = ch[c].Df; g.mv_pos = ch[c].mv_pos; g.sample = ch[c].N;
        memcpy(g.bits, &frames[(size_t)c * MK2A_FRAME_STRIDE], (size_t)g.nbits);
        e->pending.push_back(host_frame(g));
    }
    return 0;
}

extern "C" int sonde_mk2a_fetch_frames(sonde_mk2a_t *e, sonde_mk2a_frame_t *out, int32_t max) { return engine_fetch_frames(e, out, max); }

// ---- testing taps: host code only, the kernels and their arguments are as without them
static_assert(sizeof(sonde_mk2a_state_t) == sizeof(Mk2aChan), "sonde_mk2a_state_t mirrors Mk2aChan field by field");

extern "C" int sonde_mk2a_read_tap(sonde_mk2a_t *e, int32_t channel, int32_t tap, int64_t first, int32_t count, float *out) {
    if (!e || !out || channel < 0 || channel >= e->a.n_ch || count < 0 || first < 0) return SONDE_E_ARG;
    const Mk2aArgs &a = e->a;
    const char *row; size_t esz; int64_t ring, lo, hi;                          // valid absolute indices: [lo, hi)
    HIPCHK(hipStreamSynchronize(e->stream));
    Mk2aChan st;                                                                // what the kernels have written, from their own record
    HIPCHK(hipMemcpy(&st, a.chan + channel, sizeof st, hipMemcpyDeviceToHost));
    const int64_t U = (int64_t)st.U, N = (int64_t)st.N;
    switch (tap) {
        case SONDE_MK2A_TAP_IF:    row = (const char *)(a.ifbuf + (size_t)channel * a.if_stride); esz = 8; ring = 0; lo = U - e->if_last; hi = U; break;
        case SONDE_MK2A_TAP_ZROT:  row = (const char *)(a.zrot + (size_t)channel * a.ring); esz = 8; ring = a.ring; lo = U - ring; hi = U; break;
        case SONDE_MK2A_TAP_ZLP:   row = (const char *)(a.zlp + (size_t)channel * a.ring); esz = 8; ring = a.ring; lo = U - ring; hi = U; break;
        case SONDE_MK2A_TAP_FMR:   row = (const char *)(a.fmr + (size_t)channel * a.ring); esz = 4; ring = a.ring; lo = U - ring; hi = U; break;
        case SONDE_MK2A_TAP_SRAW:  if (a.opt_iq != 5) return SONDE_E_ARG;
                                   row = (const char *)(a.sraw + (size_t)channel * a.ring); esz = 4; ring = a.ring; lo = U - ring; hi = U; break;
        case SONDE_MK2A_TAP_BUFS:  row = (const char *)(a.bufs + (size_t)channel * MK2A_M); esz = 4; ring = MK2A_M; lo = N - ring; hi = N; break;
        case SONDE_MK2A_TAP_FMBUF: row = (const char *)(a.fmbuf + (size_t)channel * MK2A_M); esz = 4; ring = MK2A_M; lo = N - ring; hi = N; break;
        default: return SONDE_E_ARG;
    }
    if (first < lo || first + count > hi) return SONDE_E_RANGE;
    if (ring == 0) {                                                            // the call's buffer: index from the call's first IF sample
        if (count) HIPCHK(hipMemcpy(out, row + (size_t)(first - lo) * esz, (size_t)count * esz, hipMemcpyDeviceToHost));
        return count;
    }
    int32_t done = 0;
    while (done < count) {
        const int64_t idx = (first + done) & (ring - 1);
        const int32_t run = (int32_t)std::min<int64_t>(count - done, ring - idx);
        HIPCHK(hipMemcpy((char *)out + (size_t)done * esz, row + (size_t)idx * esz, (size_t)run * esz, hipMemcpyDeviceToHost));
        done += run;
    }
    return count;
}

extern "C" int sonde_mk2a_read_state(sonde_mk2a_t *e, int32_t channel, sonde_mk2a_state_t *out) {
    if (!e || !out || channel < 0 || channel >= e->a.n_ch) return SONDE_E_ARG;
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(out, e->a.chan + channel, sizeof *out, hipMemcpyDeviceToHost));
    return 0;
}
