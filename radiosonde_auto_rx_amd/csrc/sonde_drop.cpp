// sonde_drop.cpp — host side of the RD94 / RD41 dropsonde engine behind include/sonde_drop.h (the reference's dropsonde/rd94rd41drop.c
// behind `iq_dec --FM --lpFM --wav --bo 16 --iq fq`).  IQ form: a front-end-only engine (SONDE_FRONTEND: iq_dec's IQ-dc removal, mixer,
// decimator, discriminator and FM low-pass) makes the FM stream of every channel in its device ring, and k_drop_slice reads it there
// through iq_dec's 16-bit conversion.  FM form: the caller's integer samples go to k_drop_slice as they are.  One slicer launch per call,
// which also completes finished frames (bytes, check masks); then the frame records into the host queue.
// bits = 32 (float32 IQ at a rate iq_dec does not decimate): k_fm_front instead of the SONDE_FRONTEND engine, every channel on a sample clock of its
// own, and channels handed out at run time (restart, release, finish of one channel; k_drop_slice_rt and k_drop_restart).
#include "../../include/sonde_drop.h"
#include "sonde_frame_engine.h"
#include "sonde_drop_dev.h"
#include <cmath>

using namespace sonde;

static sonde_drop_frame_t host_frame(const DropFrame &g) {
    sonde_drop_frame_t h;
    memset(&h, 0, sizeof h);
    h.channel = g.channel; h.nraw = g.nraw; h.complete = g.complete; h.err94 = g.err94; h.err41 = g.err41; h.sample = g.sample;
    memcpy(h.bytes, g.bytes, sizeof h.bytes);
    return h;
}

struct sonde_drop : FmSliceEngine<DropArgs, sonde_drop_frame_t, sonde_drop_info_t> {
    // the front end (IQ form) and one slicer launch over n input samples per channel at dev_in
    int run(const void *dev_in, int32_t n) { return run(dev_in, n, -1); }
    // in_stride: samples between two channels of dev_in (own front end), -1: n
    int run(const void *dev_in, int32_t n, int64_t in_stride) {
        DropArgs c = a;
        TRY(slicer_input(c, dev_in, n, in_stride));
        return launch_drain(c, sonde_launch_drop, host_frame);
    }
    // the -b frame of the open header of channels ch0 .. ch0 + count - 1, completed with '0' bits (main :1430-1445)
    int finish_from(int ch0, int count) {
        DropArgs c = a;
        c.in = own_front ? (const void *)fa.fm : d_in; c.n = 0; c.first = 0; c.finish = 1; c.ch0 = ch0; c.n_ch = count;
        if (!own_front) c.ch_stride = 0;
        return launch_drain(c, sonde_launch_drop, host_frame);
    }
};

static float baud_of(const sonde_drop_cfg_t *cfg) { return cfg->baud > 0 && !(cfg->baud < 4700 || cfg->baud > 4900) ? cfg->baud : 4800.0f; }   // :1323
constexpr int IF_TARGET = 48000;                                                                       // iq_dec.c without --IFbw
constexpr float LPFM_HZ = 6e3f;                                                                        // iq_dec.c: dsp.lpFM_bw

static int cfg_ok(const sonde_drop_cfg_t *cfg) {
    if (cfg->sample_rate < 1) return 0;
    if (cfg->input != SONDE_DROP_IN_IQ && cfg->input != SONDE_DROP_IN_FM) return 0;
    if (cfg->bits == 32) {                                          // float32: IQ at a rate iq_dec does not decimate (the engine's own front end)
        if (cfg->input != SONDE_DROP_IN_IQ) return 0;
        return design_decimator_if(cfg->sample_rate, IF_TARGET, false).decM == 1;
    }
    return cfg->bits == 8 || cfg->bits == 16;
}

static void design_of(const sonde_drop_cfg_t *cfg, sonde_drop_info_t &inf) {
    memset(&inf, 0, sizeof inf);
    int sr = cfg->sample_rate;
    if (cfg->input == SONDE_DROP_IN_IQ) {
        sr = fm_front_design(inf, cfg->sample_rate, IF_TARGET);
    } else {
        inf.if_rate = sr; inf.dec_m = 1;
    }
    inf.sps = (float)sr / baud_of(cfg);
}

extern "C" int sonde_drop_design(const sonde_drop_cfg_t *cfg, sonde_drop_info_t *info) {
    if (!cfg || !info || !cfg_ok(cfg)) return SONDE_E_ARG;
    design_of(cfg, *info);
    return 0;
}

extern "C" int sonde_drop_create(const sonde_drop_cfg_t *cfg, int32_t n_ch, const double *fq, int32_t max_chunk, sonde_drop_t **out) {
    if (!cfg || !out || n_ch < 1 || max_chunk < 1) return SONDE_E_ARG;
    *out = nullptr;
    if (!cfg_ok(cfg) || (cfg->input == SONDE_DROP_IN_IQ && !fq)) return SONDE_E_ARG;
    sonde_drop_info_t inf;
    design_of(cfg, inf);
    if (inf.sps < 2.f || inf.sps > 4096.f) return SONDE_E_ARG;          // the -b bit boundaries are kept in 32 bits: 2400 * sps samples
    max_chunk -= max_chunk % inf.dec_m;
    if (max_chunk < 1) return SONDE_E_RANGE;
    std::unique_ptr<sonde_drop> e;
    TRY(engine_new(e));
    e->info = inf; e->n_ch = n_ch; e->max_chunk = max_chunk; e->dec_m = inf.dec_m;
    DropArgs &a = e->a;
    a.n_ch = n_ch; a.inv = cfg->invert ? 1 : 0; a.opt_b = cfg->opt_b ? 1 : 0; a.spb = inf.sps;
    // frames per channel and call: a run of n samples gives at most n / sps + 0.5 bits, a frame takes 2360 of them behind its header
    a.q_cap = n_ch * ((int)(2.0 * (max_chunk / inf.dec_m) / (2360.0 * inf.sps)) + 2);
    if (cfg->input == SONDE_DROP_IN_IQ && cfg->bits == 32) {
        TRY(e->create_own_front(cfg->sample_rate, fq, LPFM_HZ, DROP_IN_RING));
        e->in_bytes = 8;
    } else if (cfg->input == SONDE_DROP_IN_IQ) {
        TRY(e->create_front(cfg->sample_rate, cfg->bits, fq, IF_TARGET, DROP_IN_RING));
        e->in_bytes = (cfg->bits / 8) * 2;
    } else {
        a.kind = cfg->bits == 16 ? DROP_IN_S16 : DROP_IN_U8;
        a.mask = 0xFFFFFFFFu;
        e->in_bytes = cfg->bits / 8;
    }
    std::vector<DropChan> ch(n_ch);
    for (DropChan &s : ch) { memset(&s, 0, sizeof s); s.par = 1; s.bit_count = DROP_HEADLEN; }
    std::vector<uint8_t> frames((size_t)n_ch * DROP_RAWBITS, 0);          // frame_rawbits: the header in front, as main presets it (:1353)
    for (int c = 0; c < n_ch; c++)
        for (int i = 0; i < DROP_HEADLEN; i++) frames[(size_t)c * DROP_RAWBITS + i] = (uint8_t)((DROP_HDR40 >> (DROP_HEADLEN - 1 - i)) & 1);
    TRY(e->upload(&a.chan, ch));
    TRY(e->upload(&a.frames, frames));
    TRY(e->dalloc(&a.q, (size_t)a.q_cap));
    TRY(e->dalloc(&a.q_count, 1));
    TRY(e->alloc_input());
    *out = e.release();
    return 0;
}

extern "C" void sonde_drop_destroy(sonde_drop_t *e) { delete e; }

extern "C" int sonde_drop_info(const sonde_drop_t *e, sonde_drop_info_t *info) {
    if (!e || !info) return SONDE_E_ARG;
    *info = e->info;
    return 0;
}

extern "C" int sonde_drop_process_host(sonde_drop_t *e, const void *samples, int32_t n) {
    return engine_process_host(e, samples, n, true);                // the front end works on streams of its own
}

extern "C" int sonde_drop_process_device(sonde_drop_t *e, const void *dev_samples, int32_t n) { return engine_process_device(e, dev_samples, n); }

// EOF with a header open: with -b main prints the frame with the missing raw bits as '0' (:1430-1445, :1253); without -b nothing
extern "C" int sonde_drop_finish(sonde_drop_t *e) {
    if (!e) return SONDE_E_ARG;
    if (e->finished) return 0;
    e->finished = 1;
    if (!e->a.opt_b) return 0;
    return e->finish_from(0, e->n_ch);
}

// ---- channels at run time (engines created with bits = 32).  The calls only enqueue on the engine's stream (every process call ends synchronised, so the
// stream is idle between calls and nothing waits here); the host mirror changes at once
static int rt_check(const sonde_drop_t *e, int32_t channel) { return (!e || !e->own_front || channel < 0 || channel >= e->n_ch) ? SONDE_E_ARG : 0; }

extern "C" int sonde_drop_process_device_strided(sonde_drop_t *e, const void *dev_samples, int64_t ch_stride, int32_t n) {
    if (e && !e->own_front) return SONDE_E_ARG;
    TRY(engine_call_check(e, dev_samples, n));
    if (ch_stride < n) return SONDE_E_ARG;
    return n == 0 ? 0 : e->run(dev_samples, n, ch_stride);
}

extern "C" int sonde_drop_restart_channel(sonde_drop_t *e, int32_t channel, double fq) {
    TRY(rt_check(e, channel));
    if (!(fq >= -0.5 && fq <= 0.5) || e->finished) return SONDE_E_ARG;
    const FmFrontChan s = e->fresh_front(fq);
    if (sonde_launch_drop_restart(&e->a, &e->fa, channel, &s, e->stream)) return SONDE_E_NOGPU;
    e->active[(size_t)channel] = 1;
    e->m_start[(size_t)channel] = e->m_done;
    return 0;
}

extern "C" int sonde_drop_release_channel(sonde_drop_t *e, int32_t channel) {
    TRY(rt_check(e, channel));
    HIPCHK(hipMemsetAsync(e->fa.active + channel, 0, sizeof(int), e->stream));
    e->active[(size_t)channel] = 0;
    return 0;
}

extern "C" int sonde_drop_channel_active(const sonde_drop_t *e, int32_t channel) {
    TRY(rt_check(e, channel));
    return e->active[(size_t)channel] ? 1 : 0;
}

extern "C" int sonde_drop_finish_channel(sonde_drop_t *e, int32_t channel) {
    TRY(rt_check(e, channel));
    if (e->finished) return SONDE_E_ARG;
    if (!e->active[(size_t)channel]) return 0;
    const int rc = e->a.opt_b ? e->finish_from(channel, 1) : 0;
    TRY(sonde_drop_release_channel(e, channel));
    return rc;
}

// testing tap: host code only, the kernels and their arguments are as without it
extern "C" int sonde_drop_read_fm(sonde_drop_t *e, int32_t channel, int64_t first, int32_t count, int16_t *out) {
    TRY(rt_check(e, channel));
    if ((!out && count) || count < 0 || first < 0 || !e->active[(size_t)channel]) return SONDE_E_ARG;   // a released channel has no stream to count in
    const int64_t have = (int64_t)(e->m_done - e->m_start[(size_t)channel]), ring = e->fa.ring;
    if (first + count > have || first < have - ring) return SONDE_E_RANGE;
    HIPCHK(hipStreamSynchronize(e->stream));
    std::vector<float> v((size_t)count);
    const float *row = e->fa.fm + (size_t)channel * (size_t)ring;
    int32_t done = 0;
    while (done < count) {
        const int64_t idx = (int64_t)((e->m_start[(size_t)channel] + (uint64_t)(first + done)) & (uint64_t)(ring - 1));
        const int32_t run = (int32_t)std::min<int64_t>(count - done, ring - idx);
        HIPCHK(hipMemcpy(v.data() + done, row + idx, (size_t)run * sizeof(float), hipMemcpyDeviceToHost));
        done += run;
    }
    for (int32_t i = 0; i < count; i++) {                            // fwrite_fm_blk's 16-bit conversion, as DropSlice::load_sample
        float x = v[(size_t)i] * 128.0f;
        x *= 256.0f;
        out[i] = (int16_t)(int)x;
    }
    return count;
}

extern "C" int sonde_drop_fetch_frames(sonde_drop_t *e, sonde_drop_frame_t *out, int32_t max) { return engine_fetch_frames(e, out, max); }
