// sonde_wxr.cpp — host side of the Weathex WxR-301D engine behind include/sonde_wxr.h (the reference's weathex/weathex301d.c behind
// `iq_dec --FM --IFbw k --lpFM --iq fq`).  IQ form: a front-end-only engine (SONDE_FRONTEND: iq_dec's IQ-dc removal, mixer, decimator,
// discriminator and FM low-pass) makes the FM stream of every channel in its device ring, and k_wxr_slice reads it there.  FM form: the
// caller's samples go to k_wxr_slice as they are.  One slicer launch per call, then the frames it completed into the host queue.
#include "../../include/sonde_wxr.h"
#include "sonde_frame_engine.h"
#include "sonde_wxr_dev.h"
#include <cmath>

using namespace sonde;

static sonde_wxr_frame_t host_frame(const WxrFrame &g, int complete) {
    sonde_wxr_frame_t h;
    memset(&h, 0, sizeof h);
    h.channel = g.channel; h.nbits = g.nbits; h.complete = complete; h.sample = g.sample;
    memcpy(h.bits, g.bits, sizeof h.bits);
    return h;
}

struct sonde_wxr : FmSliceEngine<WxrArgs, sonde_wxr_frame_t, sonde_wxr_info_t> {
    // the front end (IQ form) and one slicer launch over n input samples per channel at dev_in
    int run(const void *dev_in, int32_t n) {
        WxrArgs c = a;
        TRY(slicer_input(c, dev_in, n));
        return launch_drain(c, sonde_launch_wxr, [](const WxrFrame &g) { return host_frame(g, 1); });
    }
};

static float baud_of(const sonde_wxr_cfg_t *cfg) { return cfg->baud > 0 ? cfg->baud : cfg->pn9 ? 5000.0f : 4800.0f; }
static int if_target(const sonde_wxr_cfg_t *cfg) { return cfg->if_bw_khz * 1000 >= 32000 ? cfg->if_bw_khz * 1000 : 48000; }     // iq_dec.c: --IFbw

static int cfg_ok(const sonde_wxr_cfg_t *cfg) {
    if (cfg->sample_rate < 1) return 0;
    if (cfg->input == SONDE_WXR_IN_IQ) { if (cfg->bits != 8 && cfg->bits != 16) return 0; }
    else if (cfg->input == SONDE_WXR_IN_FM) { if (cfg->bits != 8 && cfg->bits != 16 && cfg->bits != 32) return 0; }
    else return 0;
    return 1;
}

static void design_of(const sonde_wxr_cfg_t *cfg, sonde_wxr_info_t &inf) {
    memset(&inf, 0, sizeof inf);
    int sr = cfg->sample_rate;
    if (cfg->input == SONDE_WXR_IN_IQ) {
        sr = fm_front_design(inf, cfg->sample_rate, if_target(cfg));
    } else {
        if (sr == 900001) sr -= 1;                                                       // weathex301d.c:127
        inf.if_rate = sr; inf.dec_m = 1;
    }
    inf.sps = (float)sr / baud_of(cfg);
}

extern "C" int sonde_wxr_design(const sonde_wxr_cfg_t *cfg, sonde_wxr_info_t *info) {
    if (!cfg || !info || !cfg_ok(cfg)) return SONDE_E_ARG;
    design_of(cfg, *info);
    return 0;
}

extern "C" int sonde_wxr_create(const sonde_wxr_cfg_t *cfg, int32_t n_ch, const double *fq, int32_t max_chunk, sonde_wxr_t **out) {
    if (!cfg || !out || n_ch < 1 || max_chunk < 1) return SONDE_E_ARG;
    *out = nullptr;
    if (!cfg_ok(cfg) || (cfg->input == SONDE_WXR_IN_IQ && !fq)) return SONDE_E_ARG;
    sonde_wxr_info_t inf;
    design_of(cfg, inf);
    if (inf.sps < 2.f || inf.sps > 4096.f) return SONDE_E_ARG;          // the -b bit boundaries are kept in 32 bits: 552 * sps samples
    max_chunk -= max_chunk % inf.dec_m;
    if (max_chunk < 1) return SONDE_E_RANGE;
    std::unique_ptr<sonde_wxr> e;
    TRY(engine_new(e));
    e->info = inf; e->n_ch = n_ch; e->max_chunk = max_chunk; e->dec_m = inf.dec_m;
    WxrArgs &a = e->a;
    a.n_ch = n_ch; a.inv = cfg->invert ? 1 : 0; a.opt_b = cfg->opt_b ? 1 : 0; a.spb = inf.sps;
    static const uint8_t hdr[2][5] = { { 0xAA, 0xAA, 0xAA, 0x2D, 0xD4 }, { 0xAA, 0xAA, 0xAA, 0xC1, 0x94 } };
    for (int i = 0; i < 5; i++) a.hdr = (a.hdr << 8) | hdr[cfg->pn9 ? 1 : 0][i];
    // frames per channel and call: a run of n samples gives at most n / sps + 0.5 bits, a frame takes 512 of them behind its header
    a.q_cap = n_ch * ((int)(2.0 * (max_chunk / inf.dec_m) / (512.0 * inf.sps)) + 2);
    if (cfg->input == SONDE_WXR_IN_IQ) {
        TRY(e->create_front(cfg->sample_rate, cfg->bits, fq, if_target(cfg), WXR_IN_RING));
        e->in_bytes = (cfg->bits / 8) * 2;
    } else {
        a.kind = cfg->bits == 32 ? WXR_IN_F32 : cfg->bits == 16 ? WXR_IN_S16 : WXR_IN_U8;
        a.mask = 0xFFFFFFFFu;
        e->in_bytes = cfg->bits / 8;
    }
    std::vector<WxrChan> ch(n_ch);
    for (WxrChan &s : ch) { memset(&s, 0, sizeof s); s.par = 1; }
    TRY(e->upload(&a.chan, ch));
    TRY(e->upload(&a.frames, std::vector<uint8_t>((size_t)n_ch * WXR_STRIDE, WXR_UNSET)));
    TRY(e->dalloc(&a.q, (size_t)a.q_cap));
    TRY(e->dalloc(&a.q_count, 1));
    TRY(e->alloc_input());
    *out = e.release();
    return 0;
}

extern "C" void sonde_wxr_destroy(sonde_wxr_t *e) { delete e; }

extern "C" int sonde_wxr_info(const sonde_wxr_t *e, sonde_wxr_info_t *info) {
    if (!e || !info) return SONDE_E_ARG;
    *info = e->info;
    return 0;
}

extern "C" int sonde_wxr_process_host(sonde_wxr_t *e, const void *samples, int32_t n) {
    return engine_process_host(e, samples, n, true);                // the front end works on streams of its own
}

extern "C" int sonde_wxr_process_device(sonde_wxr_t *e, const void *dev_samples, int32_t n) { return engine_process_device(e, dev_samples, n); }

// EOF with a header open: main prints the -b frame as frame_bits stands (:692-704); without -b only -t has printed something
extern "C" int sonde_wxr_finish(sonde_wxr_t *e) {
    if (!e) return SONDE_E_ARG;
    if (e->finished) return 0;
    e->finished = 1;
    const int n_ch = e->a.n_ch;
    std::vector<WxrChan> ch(n_ch);
    std::vector<uint8_t> frames((size_t)n_ch * WXR_STRIDE);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(ch.data(), e->a.chan, ch.size() * sizeof(WxrChan), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(frames.data(), e->a.frames, frames.size(), hipMemcpyDeviceToHost));
    for (int c = 0; c < n_ch; c++) {
        if (!ch[c].found) continue;
        WxrFrame g;
        memset(&g, 0, sizeof g);
        g.channel = c; g.nbits = ch[c].bit_count; g.sample = ch[c].t_hdr;
        memcpy(g.bits, &frames[(size_t)c * WXR_STRIDE], WXR_BITS);
        e->pending.push_back(host_frame(g, 0));
    }
    return 0;
}

extern "C" int sonde_wxr_fetch_frames(sonde_wxr_t *e, sonde_wxr_frame_t *out, int32_t max) { return engine_fetch_frames(e, out, max); }
