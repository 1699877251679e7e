// softin_mrz_emu.cpp — test infrastructure: the device MRZ soft-bit consumer (csrc/sonde_softin_mrz_dev.h: header search at 0.82 with the polarity rule and the ring
// left as it is, Manchester bits on a lane per bit packed by ballot, bytes, frame type and CRC-16 on the wave, the next frame's length from the verdict) compiled
// for the CPU under wave_emu.h, driven the way sonde_softin_dev_push_device drives k_softin_mrz: one wave per call, the call's soft decisions staged up to
// M10_STAGE_MAX, a record buffer of `cap` frames per launch.
//   emu_mrz_run(soft, n, calls, n_calls, invert, inv, aut, raw2, bits_ofs, cap, recs, max_recs, n_dropped, end)
//       the stream in calls of calls[0], calls[1], .. half symbols (the last length repeats until the stream is consumed) through one channel; the frames the host
//       would fetch -> recs (returns their number), frames beyond `cap` of a launch -> *n_dropped, the channel's state behind the last call -> *end
//   emu_mrz_crc(bytes51, out)
//       the end-of-frame step alone on a caller's 51 frame bytes (handed over as 408 bits at offset 0): out[0] = crclen, out[1] = crcval, out[2] = crcdat,
//       out[3] = crc_ok
//   emu_mrz_header_mask()
//       the 44 header half symbols as the search holds them, half symbol i in bit i
#include "wave_emu.h"
#include "../../radiosonde_auto_rx_amd/csrc/sonde_softin_mrz_dev.h"
#include <cmath>
#include <cstring>
#include <vector>

// SoftinMrzChan as the tests read it
struct EmuMrzState { int mode, done, inv, bitfrm_len; float mv, carry; unsigned long long bits_in, hdr_bit; float hist[MRZ_HEADLEN]; uint32_t w[MRZ_WORDS]; int pad; };

extern "C" int emu_mrz_run(const float *soft, int n, const int *calls, int n_calls, int invert, int inv, int aut, int raw2, int bits_ofs, int cap, SoftinMrzRec *recs,
                           int max_recs, int *n_dropped, EmuMrzState *end) {
    if (!soft || n < 0 || !calls || n_calls < 1 || cap < 1 || max_recs < 0 || (max_recs > 0 && !recs) || bits_ofs < 0 || bits_ofs > 64) return SONDE_E_ARG;
    for (int i = 0; i < n_calls; i++) if (calls[i] < 1) return SONDE_E_ARG;
    std::vector<SoftinMrzChan> chan(1);
    memset((void *)chan.data(), 0, sizeof(SoftinMrzChan));                     // as sonde_softin_dev_create_mrz leaves it
    chan[0].inv = inv ? 1 : 0; chan[0].bitfrm_len = MRZ_MAXBITS;
    std::vector<SoftinMrzLds> lds(1);
    std::vector<SoftinMrzRec> rec((size_t)cap);
    int got = 0, dropped = 0, k = 0;
    for (int at = 0; at < n; k++) {
        const int want = calls[k < n_calls ? k : n_calls - 1], nb = n - at < want ? n - at : want;
        const int stage_cap = nb > M10_STAGE_MAX ? 0 : nb;                     // softin_pass: what the call can hold, or nothing
        std::vector<float> sx((size_t)stage_cap, std::nanf(""));               // LDS does not survive a launch
        memset((void *)lds.data(), 0xA5, sizeof(SoftinMrzLds));
        memset((void *)rec.data(), 0xEE, (size_t)cap * sizeof(SoftinMrzRec));
        unsigned count = 0;
        emu::run_workgroup(64, [&](int tid) {
            mrz_wave_channel(chan.data(), soft + at, nb, invert ? -1.f : 1.f, aut ? 1 : 0, raw2 ? 0 : 1, bits_ofs, 0.82f, lds.data(), sx.data(), stage_cap, rec.data(), &count,
                             cap, 0, tid);
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
        const SoftinMrzChan &c = chan[0];
        end->mode = c.mode; end->done = c.done; end->inv = c.inv; end->bitfrm_len = c.bitfrm_len; end->mv = c.mv; end->carry = c.carry; end->bits_in = c.bits_in;
        end->hdr_bit = c.hdr_bit; end->pad = 0;
        memcpy(end->hist, c.hist, sizeof end->hist); memcpy(end->w, c.w, sizeof end->w);
    }
    return got;
}

extern "C" int emu_mrz_crc(const unsigned char *bytes51, int *out) {
    if (!bytes51 || !out) return SONDE_E_ARG;
    std::vector<SoftinMrzLds> lds(1);
    memset((void *)lds.data(), 0xA5, sizeof(SoftinMrzLds));
    for (int k = 0; k < MRZ_WORDS; k++) lds[0].w[k] = 0;
    for (int i = 0; i < MRZ_MAXBITS; i++) if ((bytes51[i >> 3] >> (7 - (i & 7))) & 1) lds[0].w[i >> 5] |= 1u << (i & 31);
    MrzVerdict v{};
    emu::run_workgroup(64, [&](int tid) { const MrzVerdict e = mrz_wave_end(lds.data(), MRZ_MAXBITS, 0, tid); if (tid == 63) v = e; });
    out[0] = v.crclen; out[1] = (int)v.crcval; out[2] = (int)v.crcdat; out[3] = v.crc_ok;
    return 0;
}

extern "C" unsigned long long emu_mrz_header_mask() { return mrz_header_mask(); }
