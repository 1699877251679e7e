// softin_wxr_emu.cpp — test infrastructure: the device WxR-301D soft-bit consumer (csrc/sonde_softin_wxr_dev.h: signs by ballot into the 40-bit ring, 512 bits behind
// a ring that equals the header, the 69 bytes, PN9 and the xor8 / sum8 check on the wave) compiled for the CPU under wave_emu.h, driven the way
// sonde_softin_dev_push_device drives k_softin_wxr: one wave per call, a record buffer of `cap` frames per launch, LDS that does not survive a launch.
//   emu_wxr_run(soft, n, calls, n_calls, invert_stream, invert, pn9, cap, recs, max_recs, n_dropped, end)
//       the stream in calls of calls[0], calls[1], .. soft bits (the last length repeats until the stream is consumed) through one channel; the frames the host would
//       fetch -> recs (returns their number), frames beyond `cap` of a launch -> *n_dropped, the channel's state behind the last call -> *end.  The two inversions
//       are XORed as sonde_softin_dev_create_wxr does.
//   emu_wxr_end(bytes69, pn9, out)
//       the end-of-frame step alone on a caller's 69 frame bytes (as on the air): out[0 .. 5] = chkval, chkdat, chk_ok, frid, sn, cnt; out[6 .. 74] = x
//   emu_wxr_header40(pn9), emu_wxr_lds_bytes(), emu_wxr_rec_bytes()
#include "wave_emu.h"
#include "../../radiosonde_auto_rx_amd/csrc/sonde_softin_wxr_dev.h"
#include <cstring>
#include <vector>

// SoftinWxrChan as the tests read it
struct EmuWxrState { int mode, pos; unsigned long long hist, valid, bits_in, hdr_bit; uint32_t w[WXR_WORDS]; };

extern "C" int emu_wxr_run(const float *soft, int n, const int *calls, int n_calls, int invert_stream, int invert, int pn9, int cap, SoftinWxrRec *recs, int max_recs,
                           int *n_dropped, EmuWxrState *end) {
    if (!soft || n < 0 || !calls || n_calls < 1 || cap < 1 || max_recs < 0 || (max_recs > 0 && !recs)) return SONDE_E_ARG;
    for (int i = 0; i < n_calls; i++) if (calls[i] < 1) return SONDE_E_ARG;
    const int inv = (invert_stream ? 1 : 0) ^ (invert ? 1 : 0);
    std::vector<SoftinWxrChan> chan(1);
    memset((void *)chan.data(), 0, sizeof(SoftinWxrChan));                     // as sonde_softin_dev_create_wxr leaves it: the ring holds no bit
    std::vector<SoftinWxrLds> lds(1);
    std::vector<SoftinWxrRec> rec((size_t)cap);
    int got = 0, dropped = 0, k = 0;
    for (int at = 0; at < n; k++) {
        const int want = calls[k < n_calls ? k : n_calls - 1], nb = n - at < want ? n - at : want;
        std::vector<float> call(soft + at, soft + at + nb);                    // a buffer of exactly the call's length: a read beyond it is the sanitizer's to find
        memset((void *)lds.data(), 0xA5, sizeof(SoftinWxrLds));
        memset((void *)rec.data(), 0xEE, (size_t)cap * sizeof(SoftinWxrRec));
        unsigned count = 0;
        emu::run_workgroup(64, [&](int tid) { wxr_wave_channel(chan.data(), call.data(), nb, inv, pn9 ? 1 : 0, lds.data(), rec.data(), &count, cap, 0, tid); });
        if ((int)count > cap) dropped += (int)count - cap;
        for (unsigned i = 0; i < count && (int)i < cap; i++) {
            if (got < max_recs) recs[got] = rec[i];
            got++;
        }
        at += nb;
    }
    if (n_dropped) *n_dropped = dropped;
    if (end) {
        const SoftinWxrChan &c = chan[0];
        end->mode = c.mode; end->pos = c.pos; end->hist = c.hist; end->valid = c.valid; end->bits_in = c.bits_in; end->hdr_bit = c.hdr_bit;
        memcpy(end->w, c.w, sizeof end->w);
    }
    return got;
}

extern "C" int emu_wxr_end(const unsigned char *bytes69, int pn9, unsigned *out) {
    if (!bytes69 || !out) return SONDE_E_ARG;
    std::vector<SoftinWxrLds> lds(1);
    memset((void *)lds.data(), 0xA5, sizeof(SoftinWxrLds));
    for (int k = 0; k < WXR_WORDS; k++) lds[0].w[k] = 0;
    for (int i = 0; i < WXR_NBITS; i++) if ((bytes69[i >> 3] >> (7 - (i & 7))) & 1) lds[0].w[i >> 5] |= 1u << (i & 31);
    std::vector<WxrVerdict> all(64);
    emu::run_workgroup(64, [&](int tid) { all[(size_t)tid] = wxr_wave_end(lds.data(), pn9 ? 1 : 0, tid); });
    const WxrVerdict v = all[0];
    for (const WxrVerdict &e : all)                                            // the verdict is the same on every lane
        if (e.chkval != v.chkval || e.chkdat != v.chkdat || e.chk_ok != v.chk_ok || e.frid != v.frid || e.sn != v.sn || e.cnt != v.cnt) return SONDE_E_RANGE;
    for (int k = 0; k < WXR_NBYTES; k++) if (lds[0].raw[k] != bytes69[k]) return SONDE_E_RANGE;
    out[0] = v.chkval; out[1] = v.chkdat; out[2] = (unsigned)v.chk_ok; out[3] = (unsigned)v.frid; out[4] = v.sn; out[5] = v.cnt;
    for (int k = 0; k < WXR_NBYTES; k++) out[6 + k] = lds[0].x[k];
    return 0;
}

extern "C" unsigned long long emu_wxr_header40(int pn9) { return wxr_header40(pn9); }
extern "C" int emu_wxr_lds_bytes() { return (int)sizeof(SoftinWxrLds); }
extern "C" int emu_wxr_rec_bytes() { return (int)sizeof(SoftinWxrRec); }
