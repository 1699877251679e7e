// softin_mts01_emu.cpp — test infrastructure: the device MTS01 soft-bit consumer (csrc/sonde_softin_mts01_dev.h: header search at 0.8 in either polarity with the
// ring left as it is, a bit per symbol on a lane per bit packed by ballot, the 131 bytes and the CRC-16 on the wave) compiled for the CPU under wave_emu.h, driven
// the way sonde_softin_dev_push_device drives k_softin_mts01: one wave per call, the call's soft decisions staged up to M10_STAGE_MAX, a record buffer of `cap`
// frames per launch.
//   emu_mts01_run(soft, n, calls, n_calls, invert, cap, recs, max_recs, n_dropped, end)
//       the stream in calls of calls[0], calls[1], .. symbols (the last length repeats until the stream is consumed) through one channel; the frames the host would
//       fetch -> recs (returns their number), frames beyond `cap` of a launch -> *n_dropped, the channel's state behind the last call -> *end
//   emu_mts01_crc(bytes131, out)
//       the end-of-frame step alone on a caller's 131 frame bytes: out[0] = crcval, out[1] = crcdat, out[2] = crc_ok
//   emu_mts01_header_mask()
//       the 32 header symbols as the search holds them, symbol i in bit i
#include "wave_emu.h"
#include "../../radiosonde_auto_rx_amd/csrc/sonde_softin_mts01_dev.h"
#include <cmath>
#include <cstring>
#include <vector>

// SoftinMts01Chan as the tests read it
struct EmuMts01State { int mode, done; float mv; int pad; unsigned long long bits_in, hdr_bit; float hist[MTS01_HEADLEN]; uint32_t w[MTS01_WORDS]; int pad2; };

extern "C" int emu_mts01_run(const float *soft, int n, const int *calls, int n_calls, int invert, int cap, SoftinMts01Rec *recs, int max_recs, int *n_dropped,
                             EmuMts01State *end) {
    if (!soft || n < 0 || !calls || n_calls < 1 || cap < 1 || max_recs < 0 || (max_recs > 0 && !recs)) return SONDE_E_ARG;
    for (int i = 0; i < n_calls; i++) if (calls[i] < 1) return SONDE_E_ARG;
    std::vector<SoftinMts01Chan> chan(1);
    memset((void *)chan.data(), 0, sizeof(SoftinMts01Chan));                   // as sonde_softin_dev_create_mts01 leaves it
    std::vector<SoftinMts01Lds> lds(1);
    std::vector<SoftinMts01Rec> rec((size_t)cap);
    int got = 0, dropped = 0, k = 0;
    for (int at = 0; at < n; k++) {
        const int want = calls[k < n_calls ? k : n_calls - 1], nb = n - at < want ? n - at : want;
        const int stage_cap = nb > M10_STAGE_MAX ? 0 : nb;                     // softin_pass: what the call can hold, or nothing
        std::vector<float> sx((size_t)stage_cap, std::nanf(""));               // LDS does not survive a launch
        memset((void *)lds.data(), 0xA5, sizeof(SoftinMts01Lds));
        memset((void *)rec.data(), 0xEE, (size_t)cap * sizeof(SoftinMts01Rec));
        unsigned count = 0;
        emu::run_workgroup(64, [&](int tid) {
            mts01_wave_channel(chan.data(), soft + at, nb, invert ? -1.f : 1.f, 0.8f, lds.data(), sx.data(), stage_cap, rec.data(), &count, cap, 0, tid);
        });
        if ((int)count > cap) dropped += (int)count - cap;
        for (unsigned i = 0; i < count && (int)i < cap; i++) {
            if (got < max_recs) recs[got] = rec[i];
            got++;
        }
        at += nb;
    }
    if (n_dropped) *n_dropped = dropped;
    if (end) {
        const SoftinMts01Chan &c = chan[0];
        end->mode = c.mode; end->done = c.done; end->mv = c.mv; end->pad = 0; end->bits_in = c.bits_in; end->hdr_bit = c.hdr_bit; end->pad2 = 0;
        memcpy(end->hist, c.hist, sizeof end->hist); memcpy(end->w, c.w, sizeof end->w);
    }
    return got;
}

extern "C" int emu_mts01_crc(const unsigned char *bytes131, int *out) {
    if (!bytes131 || !out) return SONDE_E_ARG;
    std::vector<SoftinMts01Lds> lds(1);
    memset((void *)lds.data(), 0xA5, sizeof(SoftinMts01Lds));
    for (int k = 0; k < MTS01_WORDS; k++) lds[0].w[k] = 0;
    for (int i = 0; i < MTS01_NBITS; i++) if ((bytes131[i >> 3] >> (7 - (i & 7))) & 1) lds[0].w[i >> 5] |= 1u << (i & 31);
    Mts01Verdict v{};
    emu::run_workgroup(64, [&](int tid) { const Mts01Verdict e = mts01_wave_end(lds.data(), tid); if (tid == 63) v = e; });
    out[0] = (int)v.crcval; out[1] = (int)v.crcdat; out[2] = v.crc_ok;
    return 0;
}

extern "C" unsigned long long emu_mts01_header_mask() { return mts01_header_mask(); }
