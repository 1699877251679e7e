// sonde_imet4.cpp — host side of the iMet-4 / iMet-1-RS engine behind include/sonde_imet4.h (the reference's imet/imet4iq.c).
// Design (sonde_design.cpp: design_imet4, design_mixer, design_lowpass), device state, one k_imet4_afsk launch per call, the frame queue.
#include "../../include/sonde_hip.h"
#include "../../include/sonde_imet4.h"
#include "sonde_host.h"
#include "sonde_imet4_dev.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "libsonde_hip: %s failed: %s\n", #x, hipGetErrorString(e_)); return SONDE_E_NOGPU; } } while (0)

using namespace sonde;

struct sonde_imet4 {
    Imet4Args a{};
    hipStream_t stream = nullptr;
    int max_chunk = 0, in_bytes = 0;
    void *d_in = nullptr;
    std::vector<void *> allocs;
    std::vector<sonde_imet4_frame_t> pending;   // fetched from the device, not yet handed out
    size_t pending_pos = 0;
    int overflowed = 0;

    template <class T> int dalloc(T **p, size_t n) {
        HIPCHK(hipMalloc((void **)p, (n ? n : 1) * sizeof(T)));
        allocs.push_back(*p);
        HIPCHK(hipMemsetAsync(*p, 0, (n ? n : 1) * sizeof(T), stream));
        return 0;
    }
    ~sonde_imet4() {
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
        for (void *p : allocs) (void)hipFree(p);
    }
};

static std::vector<float> dup_taps(const std::vector<float> &w) {
    std::vector<float> d(2 * w.size() + 1, 0.f);
    for (size_t i = 0; i < w.size(); i++) d[i] = d[w.size() + i] = w[i];
    return d;
}

extern "C" int sonde_imet4_create(const sonde_imet4_cfg_t *cfg, int32_t n_ch, const double *fq, int32_t max_chunk,
                                  sonde_imet4_t **out, int32_t *if_rate, int32_t *dec_m) {
    if (!cfg || !out || n_ch < 1 || max_chunk < 1) return SONDE_E_ARG;
    *out = nullptr;
    if (cfg->bits != 8 && cfg->bits != 16) return SONDE_E_ARG;                 // float32 input: not built
    if (cfg->sample_rate < 4800) return SONDE_E_ARG;
    if (cfg->iq && !fq) return SONDE_E_ARG;
    float lpbw = cfg->lpbw_hz > 0 ? (float)cfg->lpbw_hz : 16e3f;
    if (cfg->imet1 && lpbw < 60e3f) lpbw = 80e3f;
    // (imet4iq.c:1509-1516: dsp.lpIQ_bw is an int)
    const Imet4Design d = design_imet4(cfg->sample_rate, cfg->iq != 0, cfg->min != 0, cfg->imet1 != 0, (float)(int)lpbw);
    const int if_sr = d.if_sr, decM = d.decM;
    if (if_rate) *if_rate = if_sr;
    if (dec_m) *dec_m = decM;
    max_chunk -= max_chunk % decM;                                              // calls take whole IF samples
    if (max_chunk < 1) return SONDE_E_RANGE;
    auto pow2 = [](long long v) { long long p = 1; while (p < v) p <<= 1; return p; };
    // history rings: a tile of 64 samples plus the longest look-back (IF / FM filter, the tone lag of one bit)
    const long long ring = pow2(std::max<long long>({(long long)d.lp_iq1.size(), (long long)d.lp_fm.size(), (long long)(if_sr / 1200)}) + 128);
    const long long bring = decM > 1 ? pow2(64LL * decM + (long long)d.lp_dec.size() + 64) : 1;
    if (ring > (1 << 16) || bring > (1 << 20)) return SONDE_E_ARG;              // rates far beyond what a sonde channel needs
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); return SONDE_E_NOGPU; }

    auto *e = new (std::nothrow) sonde_imet4();
    if (!e) return SONDE_E_NOMEM;
    int rc = 0;
#define TRY(x) do { rc = (x); if (rc) { delete e; return rc; } } while (0)
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) { delete e; return SONDE_E_NOGPU; }
    Imet4Args &a = e->a;
    const float sps = (float)if_sr / 1200.0f;
    a.n_ch = n_ch; a.iq = cfg->iq ? 1 : 0; a.bits = cfg->bits; a.dc = cfg->dc ? 1 : 0;
    a.lp_iq = (cfg->iq && cfg->lp_iq) ? 1 : 0; a.lp_fm = cfg->lp_fm ? 1 : 0;
    a.sr = if_sr; a.M = (int)(sps * 32);
    a.bitlen = if_sr / 1200.0;
    a.w1 = 6.2831853071795864769252867665590 * 2200.0;
    a.w2 = 6.2831853071795864769252867665590 * 1200.0;
    a.head_sps = 30 * sps;
    a.taps_iq = (int)d.lp_iq1.size(); a.taps_fm = (int)d.lp_fm.size();
    a.ring = (int)ring; a.decM = decM; a.pre = decM > 1; a.taps_dec = (int)d.lp_dec.size(); a.bring_len = (int)bring;
    a.if_stride = max_chunk / decM;
    e->max_chunk = max_chunk;
    e->in_bytes = (cfg->bits / 8) * (a.iq ? 2 : 1);
    // frames per channel and call: one per 990 bit decisions at most, plus one that was under way
    a.q_cap = n_ch * (int)(max_chunk / decM / (990.0 * a.bitlen) + 2);

    std::vector<Imet4Chan> ch(n_ch);
    for (int c = 0; c < n_ch; c++) {
        Imet4Chan &s = ch[c];
        memset(&s, 0, sizeof s);
        s.bit0 = 8;
        s.locked = 0;
        s.maxlim = (uint32_t)if_sr;
        s.maxcnt = s.maxlim / 32;
        s.maxlim *= (uint32_t)decM;                                          // IQ-dc blocks count base-rate samples
        s.maxcnt *= (uint32_t)decM;
        if (s.maxcnt < 1) s.maxcnt = 1;
        s.lut_len = 1;
        if (a.iq) {
            const Mixer m = design_mixer(-std::max(-0.5, std::min(0.5, fq[c])), cfg->sample_rate);
            s.f0 = m.f0; s.lut_len = m.lut_len;
        }
    }
    std::vector<uint8_t> frames((size_t)n_ch * IMET4_FRAME_STRIDE, 0);
    static const uint8_t soh[10] = {0, 1, 0, 0, 0, 0, 0, 0, 0, 1};         // bitframe's initial SOH character, imet4iq.c:847
    for (int c = 0; c < n_ch; c++) memcpy(&frames[(size_t)c * IMET4_FRAME_STRIDE], soh, 10);
    const std::vector<float> w0 = dup_taps(d.lp_iq0), w1 = dup_taps(d.lp_iq1), wf = dup_taps(d.lp_fm), wd = dup_taps(d.lp_dec);

    TRY(e->dalloc(&a.chan, n_ch));
    TRY(e->dalloc(&a.zring, (size_t)n_ch * a.ring));
    TRY(e->dalloc(&a.fmring, (size_t)n_ch * a.ring));
    TRY(e->dalloc(&a.xring, (size_t)n_ch * a.ring));
    TRY(e->dalloc(&a.bring, (size_t)n_ch * a.bring_len));
    TRY(e->dalloc(&a.ifbuf, (size_t)n_ch * (a.pre ? a.if_stride : 1)));
    TRY(e->dalloc(&a.bufs, (size_t)n_ch * a.M));
    TRY(e->dalloc(&a.frames, frames.size()));
    float *ws0, *ws1, *wsf;
    TRY(e->dalloc(&ws0, w0.size())); TRY(e->dalloc(&ws1, w1.size())); TRY(e->dalloc(&wsf, wf.size()));
    float *wsd;
    TRY(e->dalloc(&wsd, wd.size()));
    a.ws_iq0 = ws0; a.ws_iq1 = ws1; a.ws_fm = wsf; a.ws_dec = wsd;
    TRY(e->dalloc(&a.q, (size_t)a.q_cap));
    TRY(e->dalloc(&a.q_count, 1));
    uint8_t *din;
    TRY(e->dalloc(&din, (size_t)n_ch * max_chunk * e->in_bytes));
    e->d_in = din;
    if (hipMemcpyAsync(a.chan, ch.data(), ch.size() * sizeof(Imet4Chan), hipMemcpyHostToDevice, e->stream) != hipSuccess ||
        hipMemcpyAsync(a.frames, frames.data(), frames.size(), hipMemcpyHostToDevice, e->stream) != hipSuccess ||
        hipMemcpyAsync(ws0, w0.data(), w0.size() * sizeof(float), hipMemcpyHostToDevice, e->stream) != hipSuccess ||
        hipMemcpyAsync(ws1, w1.data(), w1.size() * sizeof(float), hipMemcpyHostToDevice, e->stream) != hipSuccess ||
        hipMemcpyAsync(wsf, wf.data(), wf.size() * sizeof(float), hipMemcpyHostToDevice, e->stream) != hipSuccess ||
        hipMemcpyAsync(wsd, wd.data(), wd.size() * sizeof(float), hipMemcpyHostToDevice, e->stream) != hipSuccess ||
        hipStreamSynchronize(e->stream) != hipSuccess) { delete e; return SONDE_E_NOGPU; }
#undef TRY
    *out = e;
    return 0;
}

extern "C" void sonde_imet4_destroy(sonde_imet4_t *e) { delete e; }

// one launch over n samples per channel at dev_in, then the frames it completed into the host queue
static int run(sonde_imet4_t *e, const void *dev_in, int32_t n) {
    Imet4Args a = e->a;
    a.in = dev_in; a.n = n / a.decM;
    HIPCHK(hipMemsetAsync(a.q_count, 0, sizeof(int), e->stream));
    if (sonde_launch_imet4(&a, e->stream)) return SONDE_E_NOGPU;
    int cnt = 0;
    HIPCHK(hipMemcpyAsync(&cnt, a.q_count, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (cnt > a.q_cap) { e->overflowed = 1; cnt = a.q_cap; }
    if (cnt > 0) {
        std::vector<Imet4Frame> f(cnt);
        HIPCHK(hipMemcpy(f.data(), a.q, cnt * sizeof(Imet4Frame), hipMemcpyDeviceToHost));
        std::sort(f.begin(), f.end(), [](const Imet4Frame &x, const Imet4Frame &y) {
            return x.channel != y.channel ? x.channel < y.channel : x.sample < y.sample; });
        for (const Imet4Frame &g : f) {
            sonde_imet4_frame_t h;
            h.channel = g.channel; h.nbits = g.nbits; h.sample = g.sample;
            memcpy(h.bits, g.bits, sizeof h.bits);
            e->pending.push_back(h);
        }
    }
    if (e->overflowed) { e->overflowed = 0; return SONDE_E_OVERFLOW; }     // reported once: frames of this call were lost
    return 0;
}

extern "C" int sonde_imet4_process_host(sonde_imet4_t *e, const void *samples, int32_t n) {
    if (!e || (!samples && n)) return SONDE_E_ARG;
    if (n < 0 || n > e->max_chunk || n % e->a.decM) return SONDE_E_RANGE;
    if (n == 0) return 0;
    HIPCHK(hipMemcpyAsync(e->d_in, samples, (size_t)e->a.n_ch * n * e->in_bytes, hipMemcpyHostToDevice, e->stream));
    return run(e, e->d_in, n);
}

extern "C" int sonde_imet4_process_device(sonde_imet4_t *e, const void *dev_samples, int32_t n) {
    if (!e || (!dev_samples && n)) return SONDE_E_ARG;
    if (n < 0 || n > e->max_chunk || n % e->a.decM) return SONDE_E_RANGE;
    if (n == 0) return 0;
    return run(e, dev_samples, n);
}

extern "C" int sonde_imet4_fetch_frames(sonde_imet4_t *e, sonde_imet4_frame_t *out, int32_t max) {
    if (!e || (!out && max > 0) || max < 0) return SONDE_E_ARG;
    int k = 0;
    while (k < max && e->pending_pos < e->pending.size()) out[k++] = e->pending[e->pending_pos++];
    if (e->pending_pos == e->pending.size()) { e->pending.clear(); e->pending_pos = 0; }
    return k;
}
