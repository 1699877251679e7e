// sonde_imet4.cpp — host side of the iMet-4 / iMet-1-RS engine behind include/sonde_imet4.h (the reference's imet/imet4iq.c).
// Design (sonde_design.cpp: design_imet4, design_mixer, design_lowpass), device state, one k_imet4_afsk launch per call, the frame queue,
// channels released and restarted at run time (the active mask, k_imet4_restart).
#include "../../include/sonde_imet4.h"
#include "sonde_frame_engine.h"
#include "sonde_imet4_dev.h"
#include <cmath>

using namespace sonde;

struct sonde_imet4 : FrameEngine<sonde_imet4_frame_t> {
    Imet4Args a{};
    int32_t if_last = 0;                 // IF samples per channel of the last call whose kernels ran (the range of the testing tap on ifbuf)
    int32_t sample_rate = 0;             // input rate: the mixer table of a channel is designed at it
    std::vector<uint8_t> active;         // host mirror of a.active (the device copy changes on the stream, in order with the calls)

    // the record create builds for a channel at fq (--iq fq; ignored for FM audio)
    Imet4Chan fresh_chan(double fq) const {
        Imet4Chan s;
        memset(&s, 0, sizeof s);
        s.bit0 = 8;
        s.locked = 0;
        s.maxlim = (uint32_t)a.sr;
        s.maxcnt = s.maxlim / 32;
        s.maxlim *= (uint32_t)a.decM;                                            // IQ-dc blocks count base-rate samples
        s.maxcnt *= (uint32_t)a.decM;
        if (s.maxcnt < 1) s.maxcnt = 1;
        s.lut_len = 1;
        if (a.iq) {
            const Mixer m = design_mixer(-std::max(-0.5, std::min(0.5, fq)), sample_rate);
            s.f0 = m.f0; s.lut_len = m.lut_len;
        }
        return s;
    }
    // one launch over n samples per channel at dev_in, channel c's row at c * ch_stride samples
    int run(const void *dev_in, int32_t n) { return run(dev_in, n, n); }
    int run(const void *dev_in, int32_t n, int64_t ch_stride) {
        if (a.bits == 32 && a.iq && ((uintptr_t)dev_in & 7u)) return SONDE_E_ARG;   // float2 loads
        Imet4Args c = a;
        c.in = dev_in; c.n = n / c.decM; c.ch_stride = ch_stride;
        // the kernels as they were before run-time channels serve 8- / 16-bit samples in rows n apart with every channel active
        c.rt = a.bits == 32 || ch_stride != n || std::find(active.begin(), active.end(), 0) != active.end();
        const int rc = drain(c);
        if (rc == 0 || rc == SONDE_E_OVERFLOW) if_last = c.n;                    // (an overflow loses frames, the samples are written)
        return rc;
    }
    int drain(const Imet4Args &c) {
        return launch_drain(c, sonde_launch_imet4, [](const Imet4Frame &g) {
            sonde_imet4_frame_t h;
            h.channel = g.channel; h.nbits = g.nbits; h.sample = g.sample;
            memcpy(h.bits, g.bits, sizeof h.bits);
            return h;
        });
    }
};

extern "C" int sonde_imet4_create(const sonde_imet4_cfg_t *cfg, int32_t n_ch, const double *fq, int32_t max_chunk,
                                  sonde_imet4_t **out, int32_t *if_rate, int32_t *dec_m) {
    if (!cfg || !out || n_ch < 1 || max_chunk < 1) return SONDE_E_ARG;
    *out = nullptr;
    if (cfg->bits != 8 && cfg->bits != 16 && cfg->bits != 32) return SONDE_E_ARG;   // 32: float32
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
    std::unique_ptr<sonde_imet4> e;
    TRY(engine_new(e));
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
    e->n_ch = n_ch; e->max_chunk = max_chunk; e->dec_m = decM; e->sample_rate = cfg->sample_rate;
    e->in_bytes = (cfg->bits / 8) * (a.iq ? 2 : 1);
    // frames per channel and call: one per 990 bit decisions at most, plus one that was under way
    a.q_cap = n_ch * (int)(max_chunk / decM / (990.0 * a.bitlen) + 2);

    std::vector<Imet4Chan> ch(n_ch);
    for (int c = 0; c < n_ch; c++) ch[c] = e->fresh_chan(a.iq ? fq[c] : 0.0);
    e->active.assign((size_t)n_ch, 1);                                          // every channel runs from create on
    std::vector<uint8_t> frames((size_t)n_ch * IMET4_FRAME_STRIDE, 0);
    static const uint8_t soh[10] = {0, 1, 0, 0, 0, 0, 0, 0, 0, 1};         // bitframe's initial SOH character, imet4iq.c:847
    for (int c = 0; c < n_ch; c++) memcpy(&frames[(size_t)c * IMET4_FRAME_STRIDE], soh, 10);

    TRY(e->upload(&a.chan, ch));
    TRY(e->dalloc(&a.zring, (size_t)n_ch * a.ring));
    TRY(e->dalloc(&a.fmring, (size_t)n_ch * a.ring));
    TRY(e->dalloc(&a.xring, (size_t)n_ch * a.ring));
    TRY(e->dalloc(&a.bring, (size_t)n_ch * a.bring_len));
    TRY(e->dalloc(&a.ifbuf, (size_t)n_ch * (a.pre ? a.if_stride : 1)));
    TRY(e->dalloc(&a.bufs, (size_t)n_ch * a.M));
    TRY(e->upload(&a.frames, frames));
    TRY(e->upload(&a.active, std::vector<int>((size_t)n_ch, 1)));
    TRY(e->upload(&a.ws_iq0, dup_taps(d.lp_iq0)));
    TRY(e->upload(&a.ws_iq1, dup_taps(d.lp_iq1)));
    TRY(e->upload(&a.ws_fm, dup_taps(d.lp_fm)));
    TRY(e->upload(&a.ws_dec, dup_taps(d.lp_dec)));
    TRY(e->dalloc(&a.q, (size_t)a.q_cap));
    TRY(e->dalloc(&a.q_count, 1));
    TRY(e->alloc_input());
    *out = e.release();
    return 0;
}

extern "C" void sonde_imet4_destroy(sonde_imet4_t *e) { delete e; }

extern "C" int sonde_imet4_process_host(sonde_imet4_t *e, const void *samples, int32_t n) { return engine_process_host(e, samples, n, false); }

extern "C" int sonde_imet4_process_device(sonde_imet4_t *e, const void *dev_samples, int32_t n) { return engine_process_device(e, dev_samples, n); }

extern "C" int sonde_imet4_process_device_strided(sonde_imet4_t *e, const void *dev_samples, int64_t ch_stride, int32_t n) {
    TRY(engine_call_check(e, dev_samples, n));
    if (ch_stride < n) return SONDE_E_ARG;
    return n == 0 ? 0 : e->run(dev_samples, n, ch_stride);
}

// ---- channels at run time.  Both calls only enqueue on the engine's stream (every process call ends synchronised, so the stream is idle
// between calls and nothing waits here); the host mirror changes at once
extern "C" int sonde_imet4_restart_channel(sonde_imet4_t *e, int32_t channel, double fq) {
    if (!e || channel < 0 || channel >= e->n_ch || (e->a.iq && !(fq == fq))) return SONDE_E_ARG;
    const Imet4Chan s = e->fresh_chan(fq);
    if (sonde_launch_imet4_restart(&e->a, channel, &s, e->stream)) return SONDE_E_NOGPU;
    e->active[(size_t)channel] = 1;
    return 0;
}

extern "C" int sonde_imet4_release_channel(sonde_imet4_t *e, int32_t channel) {
    if (!e || channel < 0 || channel >= e->n_ch) return SONDE_E_ARG;
    HIPCHK(hipMemsetAsync(e->a.active + channel, 0, sizeof(int), e->stream));
    e->active[(size_t)channel] = 0;
    return 0;
}

extern "C" int sonde_imet4_channel_active(const sonde_imet4_t *e, int32_t channel) {
    if (!e || channel < 0 || channel >= e->n_ch) return SONDE_E_ARG;
    return e->active[(size_t)channel] ? 1 : 0;
}

extern "C" int sonde_imet4_fetch_frames(sonde_imet4_t *e, sonde_imet4_frame_t *out, int32_t max) { return engine_fetch_frames(e, out, max); }

// ---- testing taps: host code only, the kernels and their arguments are as without them
static_assert(sizeof(sonde_imet4_state_t) == sizeof(Imet4Chan), "sonde_imet4_state_t mirrors Imet4Chan field by field");

extern "C" int sonde_imet4_tap_ring(sonde_imet4_t *e) { return e ? e->a.ring : SONDE_E_ARG; }

extern "C" int sonde_imet4_read_tap(sonde_imet4_t *e, int32_t channel, int32_t tap, int64_t first, int32_t count, float *out) {
    if (!e || !out || channel < 0 || channel >= e->a.n_ch || count < 0 || first < 0) return SONDE_E_ARG;
    const Imet4Args &a = e->a;
    HIPCHK(hipStreamSynchronize(e->stream));
    Imet4Chan st;                                                               // what the kernels have written, from their own record
    HIPCHK(hipMemcpy(&st, a.chan + channel, sizeof st, hipMemcpyDeviceToHost));
    const int64_t U = (int64_t)(st.sample_hi + st.sample);
    const char *row; size_t esz;
    switch (tap) {
        case SONDE_IMET4_TAP_IF:     if (!a.pre) return SONDE_E_ARG;
                                     row = (const char *)(a.ifbuf + (size_t)channel * a.if_stride); esz = 8; break;
        case SONDE_IMET4_TAP_ZRING:  if (!a.lp_iq) return SONDE_E_ARG;
                                     row = (const char *)(a.zring + (size_t)channel * a.ring); esz = 8; break;
        case SONDE_IMET4_TAP_FMRING: if (!a.lp_fm) return SONDE_E_ARG;
                                     row = (const char *)(a.fmring + (size_t)channel * a.ring); esz = 4; break;
        case SONDE_IMET4_TAP_XRING:  row = (const char *)(a.xring + (size_t)channel * a.ring); esz = 4; break;
        default: return SONDE_E_ARG;
    }
    if (tap == SONDE_IMET4_TAP_IF) {                                            // the call's buffer: index from the call's first IF sample
        const int64_t lo = U - e->if_last;
        if (first < lo || first + count > U) return SONDE_E_RANGE;
        if (count) HIPCHK(hipMemcpy(out, row + (size_t)(first - lo) * esz, (size_t)count * esz, hipMemcpyDeviceToHost));
        return count;
    }
    // a tile cut short at a header has written up to 63 samples past U, over the oldest entries: those no longer count as history
    const int64_t ring = a.ring, lo = U - (ring - 64);
    if (first < lo || first + count > U) return SONDE_E_RANGE;
    int32_t done = 0;
    while (done < count) {
        const int64_t idx = (first + done) & (ring - 1);
        const int32_t run = (int32_t)std::min<int64_t>(count - done, ring - idx);
        HIPCHK(hipMemcpy((char *)out + (size_t)done * esz, row + (size_t)idx * esz, (size_t)run * esz, hipMemcpyDeviceToHost));
        done += run;
    }
    return count;
}

extern "C" int sonde_imet4_read_state(sonde_imet4_t *e, int32_t channel, sonde_imet4_state_t *out) {
    if (!e || !out || channel < 0 || channel >= e->a.n_ch) return SONDE_E_ARG;
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(out, e->a.chan + channel, sizeof *out, hipMemcpyDeviceToHost));
    return 0;
}
