// softin_meisei_emu.cpp — test infrastructure: the device Meisei soft-bit consumer (csrc/sonde_softin_meisei_dev.h: header search in either polarity with the ring
// left as it is, biphase-S bits on a lane per bit packed by ballot, the 12 BCH(63,51) blocks one at a time on the wave) compiled for the CPU under wave_emu.h,
// driven the way sonde_softin_dev_push_device drives k_softin_meisei: one wave per call, the call's soft decisions staged up to M10_STAGE_MAX, a record buffer of
// `cap` frames per launch.
//   emu_meisei_run(soft, n, calls, n_calls, invert, ecc, cap, recs, max_recs, n_dropped, end)
//       the stream in calls of calls[0], calls[1], .. half symbols (the last length repeats until the stream is consumed) through one channel; the frames the host
//       would fetch -> recs (returns their number), frames beyond `cap` of a launch -> *n_dropped, the channel's state behind the last call -> *end
//   emu_meisei_end(bits75, ecc, rec)
//       the end-of-frame step alone on a caller's 600 bits (MSB first): bits behind the block loop and the 12 verdicts -> *rec
//   emu_meisei_header_mask()
//       the 48 header half symbols as the search holds them, half symbol i in bit i
#include "wave_emu.h"
#include "../../radiosonde_auto_rx_amd/csrc/sonde_softin_meisei_dev.h"
#include <cmath>
#include <cstring>
#include <vector>

// SoftinMeiseiChan as the tests read it
struct EmuMeiseiState { int mode, done; float mv, carry; unsigned long long bits_in, hdr_bit; float hist[MEISEI_HEADLEN]; uint32_t w[MEISEI_WORDS]; int pad; };

extern "C" int emu_meisei_run(const float *soft, int n, const int *calls, int n_calls, int invert, int ecc, int cap, SoftinMeiseiRec *recs, int max_recs, int *n_dropped,
                              EmuMeiseiState *end) {
    if (!soft || n < 0 || !calls || n_calls < 1 || cap < 1 || max_recs < 0 || (max_recs > 0 && !recs)) return SONDE_E_ARG;
    for (int i = 0; i < n_calls; i++) if (calls[i] < 1) return SONDE_E_ARG;
    std::vector<SoftinMeiseiChan> chan(1);
    memset((void *)chan.data(), 0, sizeof(SoftinMeiseiChan));                  // as sonde_softin_dev_create_meisei leaves it
    std::vector<SoftinMeiseiLds> lds(1);
    std::vector<SoftinMeiseiRec> rec((size_t)cap);
    int got = 0, dropped = 0, k = 0;
    for (int at = 0; at < n; k++) {
        const int want = calls[k < n_calls ? k : n_calls - 1], nb = n - at < want ? n - at : want;
        const int stage_cap = nb > M10_STAGE_MAX ? 0 : nb;                     // softin_pass: what the call can hold, or nothing
        std::vector<float> sx((size_t)stage_cap, std::nanf(""));               // LDS does not survive a launch
        memset((void *)lds.data(), 0xA5, sizeof(SoftinMeiseiLds));
        memset((void *)rec.data(), 0xEE, (size_t)cap * sizeof(SoftinMeiseiRec));
        unsigned count = 0;
        emu::run_workgroup(64, [&](int tid) {
            meisei_wave_channel(chan.data(), soft + at, nb, invert ? -1.f : 1.f, ecc ? 1 : 0, 0.8f, lds.data(), sx.data(), stage_cap, rec.data(), &count, cap, 0, tid);
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
        const SoftinMeiseiChan &c = chan[0];
        end->mode = c.mode; end->done = c.done; end->mv = c.mv; end->carry = c.carry; end->bits_in = c.bits_in; end->hdr_bit = c.hdr_bit; end->pad = 0;
        memcpy(end->hist, c.hist, sizeof end->hist); memcpy(end->w, c.w, sizeof end->w);
    }
    return got;
}

extern "C" int emu_meisei_end(const unsigned char *bits75, int ecc, SoftinMeiseiRec *rec) {
    if (!bits75 || !rec) return SONDE_E_ARG;
    std::vector<SoftinMeiseiLds> lds(1);
    memset((void *)lds.data(), 0xA5, sizeof(SoftinMeiseiLds));
    for (int k = 0; k < MEISEI_WORDS; k++) lds[0].w[k] = 0;
    for (int i = 0; i < MEISEI_NBITS; i++) if ((bits75[i >> 3] >> (7 - (i & 7))) & 1) lds[0].w[i >> 5] |= 1u << (i & 31);
    unsigned long long be = 0;
    if (ecc) emu::run_workgroup(64, [&](int tid) { const unsigned long long e = meisei_wave_end(lds.data(), tid); if (tid == 63) be = e; });
    memset((void *)rec, 0, sizeof *rec);
    for (int k = 0; k < MEISEI_BLOCKS; k++) rec->block_err[k] = (uint8_t)((be >> (4 * k)) & 0xF);
    for (int i = 0; i < MEISEI_NBITS; i++) if ((lds[0].w[i >> 5] >> (i & 31)) & 1u) rec->bits[i >> 3] |= (uint8_t)(0x80 >> (i & 7));
    return 0;
}

extern "C" unsigned long long emu_meisei_header_mask() { return meisei_header_mask(); }
