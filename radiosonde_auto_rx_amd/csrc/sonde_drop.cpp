// sonde_drop.cpp — host side of the RD94 / RD41 dropsonde engine behind include/sonde_drop.h (the reference's dropsonde/rd94rd41drop.c
// behind `iq_dec --FM --lpFM --wav --bo 16 --iq fq`).  IQ form: a front-end-only engine (SONDE_FRONTEND: iq_dec's IQ-dc removal, mixer,
// decimator, discriminator and FM low-pass) makes the FM stream of every channel in its device ring, and k_drop_slice reads it there
// through iq_dec's 16-bit conversion.  FM form: the caller's integer samples go to k_drop_slice as they are.  One slicer launch per call,
// which also completes finished frames (bytes, check masks); then the frame records into the host queue.
#include "../../include/sonde_hip.h"
#include "../../include/sonde_drop.h"
#include "sonde_host.h"
#include "sonde_drop_dev.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "libsonde_hip: %s failed: %s\n", #x, hipGetErrorString(e_)); return SONDE_E_NOGPU; } } while (0)

using namespace sonde;

struct sonde_drop {
    DropArgs a{};
    sonde_drop_cfg_t cfg{};
    sonde_drop_info_t info{};
    hipStream_t stream = nullptr;
    sonde_engine_t *front = nullptr;                 // IQ form
    int max_chunk = 0, in_bytes = 0, finished = 0;
    uint64_t m_done = 0;                             // IF samples the front end has made per channel
    void *d_in = nullptr;
    std::vector<void *> allocs;
    std::vector<sonde_drop_frame_t> pending;          // fetched from the device, not yet handed out
    size_t pending_pos = 0;
    int overflowed = 0;

    template <class T> int dalloc(T **p, size_t n) {
        HIPCHK(hipMalloc((void **)p, (n ? n : 1) * sizeof(T)));
        allocs.push_back(*p);
        HIPCHK(hipMemsetAsync(*p, 0, (n ? n : 1) * sizeof(T), stream));
        return 0;
    }
    ~sonde_drop() {
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
        if (front) sonde_engine_destroy(front);
        for (void *p : allocs) (void)hipFree(p);
    }
};

static float baud_of(const sonde_drop_cfg_t *cfg) { return cfg->baud > 0 && !(cfg->baud < 4700 || cfg->baud > 4900) ? cfg->baud : 4800.0f; }   // :1323
constexpr int IF_TARGET = 48000;                                                                       // iq_dec.c without --IFbw

static int cfg_ok(const sonde_drop_cfg_t *cfg) {
    if (cfg->sample_rate < 1) return 0;
    if (cfg->input != SONDE_DROP_IN_IQ && cfg->input != SONDE_DROP_IN_FM) return 0;
    return cfg->bits == 8 || cfg->bits == 16;
}

static void design_of(const sonde_drop_cfg_t *cfg, sonde_drop_info_t &inf) {
    memset(&inf, 0, sizeof inf);
    int sr = cfg->sample_rate;
    if (cfg->input == SONDE_DROP_IN_IQ) {
        const Decimator d = design_decimator_if(cfg->sample_rate, IF_TARGET, false);
        inf.if_rate = d.if_sr; inf.dec_m = d.decM; inf.taps_dec = d.decM == 1 ? 0 : (int)d.taps.size();
        int taps = (int)(4 * d.if_sr / 2e3); if (taps % 2 == 0) taps++;                  // iq_dec.c: --lpFM
        inf.taps_fm = taps;
        sr = d.if_sr;
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
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); return SONDE_E_NOGPU; }

    auto *e = new (std::nothrow) sonde_drop();
    if (!e) return SONDE_E_NOMEM;
    int rc = 0;
#define TRY(x) do { rc = (x); if (rc) { delete e; return rc; } } while (0)
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) { delete e; return SONDE_E_NOGPU; }
    e->cfg = *cfg; e->info = inf; e->max_chunk = max_chunk;
    DropArgs &a = e->a;
    a.n_ch = n_ch; a.inv = cfg->invert ? 1 : 0; a.opt_b = cfg->opt_b ? 1 : 0; a.spb = inf.sps;
    // frames per channel and call: a run of n samples gives at most n / sps + 0.5 bits, a frame takes 2360 of them behind its header
    const int n_if = max_chunk / inf.dec_m;
    a.q_cap = n_ch * ((int)(2.0 * n_if / (2360.0 * inf.sps)) + 2);
    if (cfg->input == SONDE_DROP_IN_IQ) {
        sonde_cfg_t fc;
        memset(&fc, 0, sizeof fc);
        fc.abi_version = SONDE_ABI_VERSION; fc.sonde_type = SONDE_FRONTEND; fc.n_channels = n_ch; fc.sample_rate = cfg->sample_rate; fc.bits = cfg->bits;
        fc.opt_lp = SONDE_LP_FM; fc.lpiq_bw = 10000; fc.max_chunk = max_chunk; fc.if_rate = IF_TARGET; fc.input = SONDE_IN_IQ;
        std::vector<double> f(fq, fq + n_ch);
        for (double &v : f) v = std::max(-0.5, std::min(0.5, v));
        TRY(sonde_engine_create(&fc, f.data(), &e->front));
        sonde_info_t fi;
        sonde_engine_info(e->front, &fi);
        if (fi.if_sr != inf.if_rate || fi.decM != inf.dec_m || fi.ring_len < n_if) { delete e; return SONDE_E_ARG; }
        a.kind = DROP_IN_RING; a.ch_stride = fi.ring_len; a.mask = (uint32_t)fi.ring_len - 1;
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
    TRY(e->dalloc(&a.chan, n_ch));
    TRY(e->dalloc(&a.frames, frames.size()));
    TRY(e->dalloc(&a.q, (size_t)a.q_cap));
    TRY(e->dalloc(&a.q_count, 1));
    uint8_t *din;
    TRY(e->dalloc(&din, (size_t)n_ch * max_chunk * e->in_bytes));
    e->d_in = din;
    if (hipMemcpyAsync(a.chan, ch.data(), ch.size() * sizeof(DropChan), hipMemcpyHostToDevice, e->stream) != hipSuccess ||
        hipMemcpyAsync(a.frames, frames.data(), frames.size(), hipMemcpyHostToDevice, e->stream) != hipSuccess ||
        hipStreamSynchronize(e->stream) != hipSuccess) { delete e; return SONDE_E_NOGPU; }
#undef TRY
    *out = e;
    return 0;
}

extern "C" void sonde_drop_destroy(sonde_drop_t *e) { delete e; }

extern "C" int sonde_drop_info(const sonde_drop_t *e, sonde_drop_info_t *info) {
    if (!e || !info) return SONDE_E_ARG;
    *info = e->info;
    return 0;
}

// q_count frames of the device queue into the host queue, in channel / time order
static int drain(sonde_drop_t *e) {
    const DropArgs &a = e->a;
    int cnt = 0;
    HIPCHK(hipMemcpyAsync(&cnt, a.q_count, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (cnt > a.q_cap) { e->overflowed = 1; cnt = a.q_cap; }
    if (cnt > 0) {
        std::vector<DropFrame> f(cnt);
        HIPCHK(hipMemcpy(f.data(), a.q, cnt * sizeof(DropFrame), hipMemcpyDeviceToHost));
        std::sort(f.begin(), f.end(), [](const DropFrame &x, const DropFrame &y) {
            return x.channel != y.channel ? x.channel < y.channel : x.sample < y.sample; });
        for (const DropFrame &g : f) {
            sonde_drop_frame_t h;
            memset(&h, 0, sizeof h);
            h.channel = g.channel; h.nraw = g.nraw; h.complete = g.complete; h.err94 = g.err94; h.err41 = g.err41; h.sample = g.sample;
            memcpy(h.bytes, g.bytes, sizeof h.bytes);
            e->pending.push_back(h);
        }
    }
    if (e->overflowed) { e->overflowed = 0; return SONDE_E_OVERFLOW; }     // reported once: frames of this call were lost
    return 0;
}

// the front end (IQ form) and one slicer launch over n input samples per channel at dev_in
static int run(sonde_drop_t *e, const void *dev_in, int32_t n) {
    DropArgs a = e->a;
    if (e->front) {
        int rc = sonde_engine_process_device(e->front, dev_in, n, n);
        if (rc < 0) return rc;
        const float *fm = nullptr; int ring = 0;
        rc = engine_fm_tap_device(e->front, &fm, &ring);
        if (rc) return rc;
        a.in = fm; a.n = n / e->info.dec_m; a.first = (uint32_t)(e->m_done & a.mask);
        e->m_done += (uint64_t)a.n;
    } else {
        a.in = dev_in; a.n = n; a.first = 0; a.ch_stride = n;
    }
    HIPCHK(hipMemsetAsync(a.q_count, 0, sizeof(int), e->stream));
    if (sonde_launch_drop(&a, e->stream)) return SONDE_E_NOGPU;
    return drain(e);
}

extern "C" int sonde_drop_process_host(sonde_drop_t *e, const void *samples, int32_t n) {
    if (!e || (!samples && n) || e->finished) return SONDE_E_ARG;
    if (n < 0 || n > e->max_chunk || n % e->info.dec_m) return SONDE_E_RANGE;
    if (n == 0) return 0;
    HIPCHK(hipMemcpyAsync(e->d_in, samples, (size_t)e->a.n_ch * n * e->in_bytes, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));                     // the front end works on streams of its own
    return run(e, e->d_in, n);
}

extern "C" int sonde_drop_process_device(sonde_drop_t *e, const void *dev_samples, int32_t n) {
    if (!e || (!dev_samples && n) || e->finished) return SONDE_E_ARG;
    if (n < 0 || n > e->max_chunk || n % e->info.dec_m) return SONDE_E_RANGE;
    if (n == 0) return 0;
    return run(e, dev_samples, n);
}

// EOF with a header open: with -b main prints the frame with the missing raw bits as '0' (:1430-1445, :1253); without -b nothing
extern "C" int sonde_drop_finish(sonde_drop_t *e) {
    if (!e) return SONDE_E_ARG;
    if (e->finished) return 0;
    e->finished = 1;
    if (!e->a.opt_b) return 0;
    DropArgs a = e->a;
    a.in = e->d_in; a.n = 0; a.first = 0; a.ch_stride = 0; a.finish = 1;
    HIPCHK(hipMemsetAsync(a.q_count, 0, sizeof(int), e->stream));
    if (sonde_launch_drop(&a, e->stream)) return SONDE_E_NOGPU;
    return drain(e);
}

extern "C" int sonde_drop_fetch_frames(sonde_drop_t *e, sonde_drop_frame_t *out, int32_t max) {
    if (!e || (!out && max > 0) || max < 0) return SONDE_E_ARG;
    int k = 0;
    while (k < max && e->pending_pos < e->pending.size()) out[k++] = e->pending[e->pending_pos++];
    if (e->pending_pos == e->pending.size()) { e->pending.clear(); e->pending_pos = 0; }
    return k;
}
