// sonde_frame_engine.h — what the host sides of the four single-sonde engines (sonde_imet4.cpp, sonde_mk2a.cpp, sonde_wxr.cpp,
// sonde_drop.cpp) share: the stream and its device allocations, the frame queue from the device to the caller, the argument checks of a
// call, and for the two FM slicers the iq_dec front end (a SONDE_FRONTEND engine whose FM ring the slicer reads).
#ifndef SONDE_FRAME_ENGINE_H
#define SONDE_FRAME_ENGINE_H
#include "../../include/sonde_hip.h"
#include "sonde_devmem.h"
#include "sonde_host.h"
#include <hip/hip_runtime.h>
#include "sonde_fm_front_dev.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <type_traits>
#include <vector>

namespace sonde {

// Frame: the frame record of the engine's public header
template <class Frame> struct FrameEngine {
    DevMem mem;
    hipStream_t stream = nullptr;
    int n_ch = 0, max_chunk = 0, dec_m = 1, in_bytes = 0, finished = 0;   // in_bytes: of one input sample of one channel
    void *d_in = nullptr;                                                 // process_host's copy of the caller's samples
    std::vector<Frame> pending;                                           // fetched from the device, not yet handed out
    size_t pending_pos = 0;
    int overflowed = 0;

    // zeroed on the stream, in order with what run() enqueues there
    template <class T> int dalloc(T **p, size_t n) { TRY(mem.dalloc(p, n, false)); HIPCHK(hipMemsetAsync(*p, 0, (n ? n : 1) * sizeof(T), stream)); return 0; }
    template <class P, class T> int upload(P **p, const std::vector<T> &v) { return mem.upload(p, v); }       // P: T or const T
    int alloc_input() {
        uint8_t *din;
        TRY(dalloc(&din, (size_t)n_ch * max_chunk * in_bytes));
        d_in = din;
        return 0;
    }
    void close_stream() {
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); stream = nullptr; }
    }
    ~FrameEngine() { close_stream(); }

    // one launch over a's input, then the frames it completed into the host queue in channel / time order.  a: the kernel's argument
    // record with its queue (q, q_count, q_cap); convert: device record -> Frame
    template <class Args, class Convert> int launch_drain(const Args &a, int (*launch)(const Args *, hipStream_t), Convert convert) {
        HIPCHK(hipMemsetAsync(a.q_count, 0, sizeof(int), stream));
        if (launch(&a, stream)) return SONDE_E_NOGPU;
        int cnt = 0;
        HIPCHK(hipMemcpyAsync(&cnt, a.q_count, sizeof(int), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (cnt > a.q_cap) { overflowed = 1; cnt = a.q_cap; }
        if (cnt > 0) {
            std::vector<std::remove_pointer_t<decltype(a.q)>> f(cnt);
            HIPCHK(hipMemcpy(f.data(), a.q, cnt * sizeof f[0], hipMemcpyDeviceToHost));
            std::sort(f.begin(), f.end(), [](const auto &x, const auto &y) { return x.channel != y.channel ? x.channel < y.channel : x.sample < y.sample; });
            for (const auto &g : f) pending.push_back(convert(g));
        }
        if (overflowed) { overflowed = 0; return SONDE_E_OVERFLOW; }      // reported once: frames of this call were lost
        return 0;
    }
};

// the create prologue behind the argument checks: a device, the engine, its stream
template <class E> int engine_new(std::unique_ptr<E> &e) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); return SONDE_E_NOGPU; }
    e.reset(new (std::nothrow) E());
    if (!e) return SONDE_E_NOMEM;
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) return SONDE_E_NOGPU;
    return 0;
}

// process_host / process_device of an engine E with `int run(const void *dev_in, int32_t n)`.  sync: wait for the copy before run (an
// engine whose run starts on other streams than its own)
template <class E> int engine_call_check(const E *e, const void *samples, int32_t n) {
    if (!e || (!samples && n) || e->finished) return SONDE_E_ARG;
    if (n < 0 || n > e->max_chunk || n % e->dec_m) return SONDE_E_RANGE;
    return 0;
}
template <class E> int engine_process_host(E *e, const void *samples, int32_t n, bool sync) {
    TRY(engine_call_check(e, samples, n));
    if (n == 0) return 0;
    HIPCHK(hipMemcpyAsync(e->d_in, samples, (size_t)e->n_ch * n * e->in_bytes, hipMemcpyHostToDevice, e->stream));
    if (sync) HIPCHK(hipStreamSynchronize(e->stream));
    return e->run(e->d_in, n);
}
template <class E> int engine_process_device(E *e, const void *dev_samples, int32_t n) {
    TRY(engine_call_check(e, dev_samples, n));
    return n == 0 ? 0 : e->run(dev_samples, n);
}
template <class E, class Frame> int engine_fetch_frames(E *e, Frame *out, int32_t max) {
    if (!e || (!out && max > 0) || max < 0) return SONDE_E_ARG;
    int k = 0;
    while (k < max && e->pending_pos < e->pending.size()) out[k++] = e->pending[e->pending_pos++];
    if (e->pending_pos == e->pending.size()) { e->pending.clear(); e->pending_pos = 0; }
    return k;
}

// ---- the iq_dec front end of the FM slicers (`iq_dec --FM [--IFbw k] --lpFM --iq fq`) ----

// iq_dec's rates and tap counts for IQ input at sample_rate into Info's if_rate / dec_m / taps_dec / taps_fm; returns the IF rate
template <class Info> int fm_front_design(Info &inf, int sample_rate, int if_target) {
    const Decimator d = design_decimator_if(sample_rate, if_target, false);
    inf.if_rate = d.if_sr; inf.dec_m = d.decM; inf.taps_dec = d.decM == 1 ? 0 : (int)d.taps.size();
    int taps = (int)(4 * d.if_sr / 2e3); if (taps % 2 == 0) taps++;                      // iq_dec.c: --lpFM
    inf.taps_fm = taps;
    return d.if_sr;
}

// k_fm_front (sonde_fm_front.hip) over a->n samples of every active channel
extern "C" int sonde_launch_fm_front(const FmFrontArgs *a, hipStream_t s);

// Args: SliceArgs of the slicer kernel (sonde_slice_dev.h); Info: the info record of the engine's public header
template <class Args, class Frame, class Info> struct FmSliceEngine : FrameEngine<Frame> {
    Args a{};
    Info info{};
    sonde_engine_t *front = nullptr;                 // IQ form
    uint64_t m_done = 0;                             // IF samples the front end has made per channel
    bool own_front = false;                          // IQ form on float32 at decM = 1: k_fm_front instead of a SONDE_FRONTEND engine
    FmFrontArgs fa{};
    int sample_rate = 0;                             // the mixer table of a channel is designed at it
    std::vector<uint8_t> active;                     // host mirror of fa.active (the device copy changes on the stream, in order with the calls)
    std::vector<uint64_t> m_start;                   // m_done at the channel's restart: where its own sample count begins in the FM ring

    ~FmSliceEngine() {
        this->close_stream();
        if (front) sonde_engine_destroy(front);
    }
    // the front-end-only engine for IQ input of `bits` at fq, and a's view of its FM ring (ring_kind: the slicer's input kind for it)
    int create_front(int sample_rate, int bits, const double *fq, int if_target, int ring_kind) {
        sonde_cfg_t fc;
        memset(&fc, 0, sizeof fc);
        fc.abi_version = SONDE_ABI_VERSION; fc.sonde_type = SONDE_FRONTEND; fc.n_channels = this->n_ch; fc.sample_rate = sample_rate; fc.bits = bits;
        fc.opt_lp = SONDE_LP_FM; fc.lpiq_bw = 10000; fc.max_chunk = this->max_chunk; fc.if_rate = if_target; fc.input = SONDE_IN_IQ;
        std::vector<double> f(fq, fq + this->n_ch);
        for (double &v : f) v = std::max(-0.5, std::min(0.5, v));
        TRY(sonde_engine_create(&fc, f.data(), &front));
        sonde_info_t fi;
        sonde_engine_info(front, &fi);
        if (fi.if_sr != info.if_rate || fi.decM != info.dec_m || fi.ring_len < this->max_chunk / info.dec_m) return SONDE_E_ARG;
        a.kind = ring_kind; a.ch_stride = fi.ring_len; a.mask = (uint32_t)fi.ring_len - 1;
        return 0;
    }
    // ---- the engine's own front end (k_fm_front): float32 IQ at a rate iq_dec does not decimate, channels handed out at run time
    // the record create and a restart build for a channel at fq (--iq fq)
    FmFrontChan fresh_front(double fq) const {
        FmFrontChan s;
        memset(&s, 0, sizeof s);
        s.maxlim = (uint32_t)info.if_rate;                                      // iq_dec.c:752-758 at decM = 1
        s.maxcnt = s.maxlim / 32;
        if (s.maxcnt < 1) s.maxcnt = 1;
        const Mixer m = design_mixer(-std::max(-0.5, std::min(0.5, fq)), sample_rate);
        s.f0 = m.f0; s.lut_len = (uint32_t)m.lut_len;
        return s;
    }
    // lpfm_hz: iq_dec's dsp.lpFM_bw; a's view of the FM ring (ring_kind: the slicer's input kind for it) and of the active mask.  The caller has checked
    // that info.dec_m is 1
    int create_own_front(int sample_rate_, const double *fq, float lpfm_hz, int ring_kind) {
        sample_rate = sample_rate_;
        const std::vector<float> w = design_lowpass(lpfm_hz / (float)info.if_rate, info.taps_fm);
        auto pow2 = [](long long v) { long long p = 1; while (p < v) p <<= 1; return p; };
        const long long ring = pow2(std::max(this->max_chunk, 64)), rring = pow2((long long)w.size() + 128);
        if ((int)w.size() > FMF_TAPS_MAX || rring > FMF_RING_MAX || ring > (1LL << 30)) return SONDE_E_ARG;
        fa.n_ch = this->n_ch; fa.taps = (int)w.size(); fa.ring = (int)ring; fa.rring = (int)rring;
        std::vector<FmFrontChan> ch((size_t)this->n_ch);
        for (int c = 0; c < this->n_ch; c++) ch[(size_t)c] = fresh_front(fq[c]);
        TRY(this->upload(&fa.chan, ch));
        TRY(this->dalloc(&fa.fm, (size_t)this->n_ch * (size_t)ring));
        TRY(this->dalloc(&fa.raw, (size_t)this->n_ch * (size_t)rring));
        TRY(this->upload(&fa.ws2, dup_taps(w)));
        TRY(this->upload(&fa.active, std::vector<int>((size_t)this->n_ch, 1)));
        active.assign((size_t)this->n_ch, 1);                                   // every channel runs from create on
        m_start.assign((size_t)this->n_ch, 0);
        own_front = true;
        a.kind = ring_kind; a.ch_stride = ring; a.mask = (uint32_t)ring - 1; a.active = fa.active; a.ch0 = 0;
        return 0;
    }
    // this call's input of the slicer: the front end's FM ring behind n more input samples (IQ form), or dev_in as it is.  in_stride: samples between two
    // channels of dev_in
    int slicer_input(Args &c, const void *dev_in, int32_t n, int64_t in_stride = -1) {
        if (own_front) {
            if ((uintptr_t)dev_in & 7u) return SONDE_E_ARG;                     // 8-byte loads of (I, Q)
            FmFrontArgs f = fa;
            f.in = (const FmfIQ *)dev_in; f.n = n; f.ch_stride = in_stride < 0 ? n : in_stride; f.first = (uint32_t)(m_done & c.mask);
            if (sonde_launch_fm_front(&f, this->stream)) return SONDE_E_NOGPU;
            c.in = fa.fm; c.n = n; c.first = f.first;
            m_done += (uint64_t)n;
            return 0;
        }
        if (!front) { c.in = dev_in; c.n = n; c.first = 0; c.ch_stride = n; return 0; }
        const int rc = sonde_engine_process_device(front, dev_in, n, n);
        if (rc < 0) return rc;
        const float *fm = nullptr; int ring = 0;
        TRY(engine_fm_tap_device(front, &fm, &ring));
        c.in = fm; c.n = n / info.dec_m; c.first = (uint32_t)(m_done & c.mask);
        m_done += (uint64_t)c.n;
        return 0;
    }
};

}  // namespace sonde
#endif
