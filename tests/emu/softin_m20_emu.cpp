// softin_m20_emu.cpp — test infrastructure: the device M20 soft-bit consumer (csrc/sonde_softin_mxx_dev.h: header search, bit pairs, differential code, bits2bytes,
// print_frame's verdicts) compiled for the CPU under wave_emu.h, driven the way sonde_softin_dev_push_device drives k_softin_m20: one wave per call, the call's
// soft decisions staged up to M10_STAGE_MAX, a record buffer of `cap` frames per launch.
//   emu_m20_run(soft, n, calls, n_calls, invert, doskip, cap, recs, max_recs, n_dropped, end)
//       the stream in calls of calls[0], calls[1], .. symbols (the last length repeats until the stream is consumed) through one channel; the frames the host
//       would fetch -> recs (returns their number), frames beyond `cap` of a launch -> *n_dropped, the channel's state behind the last call -> *end
//   emu_m20_verdicts(frame, rec)
//       m20_wave_verdicts alone on a caller's 165 frame bytes (a symbol stream cannot carry a byte 0 of 0x80 or more: the frame's first bit always decodes as 0)
#include "wave_emu.h"
#include "../../radiosonde_auto_rx_amd/csrc/sonde_softin_mxx_dev.h"
#include <cmath>
#include <cstring>
#include <vector>

// SoftinM20Chan without the ring and the bit characters
struct EmuM20State { int mode, inv, mpos, mhalf, mbit0, mskip; float ms1, mv; unsigned long long bits_in, hdr_bit; };

extern "C" int emu_m20_run(const float *soft, int n, const int *calls, int n_calls, int invert, int doskip, int cap, sonde_m20_frame_t *recs, int max_recs, int *n_dropped,
                           EmuM20State *end) {
    if (!soft || n < 0 || !calls || n_calls < 1 || cap < 1 || max_recs < 0 || (max_recs > 0 && !recs)) return SONDE_E_ARG;
    for (int i = 0; i < n_calls; i++) if (calls[i] < 1) return SONDE_E_ARG;
    std::vector<SoftinM20Chan> chan(1);
    memset((void *)chan.data(), 0, sizeof(SoftinM20Chan));
    chan[0].mbit0 = '0';                                                       // as sonde_softin_dev_create leaves it
    std::vector<SoftinM20Lds> lds(1);
    std::vector<sonde_m20_frame_t> rec((size_t)cap);
    int got = 0, dropped = 0, k = 0;
    for (int at = 0; at < n; k++) {
        const int want = calls[k < n_calls ? k : n_calls - 1], nb = n - at < want ? n - at : want;
        const int stage_cap = nb > M10_STAGE_MAX ? 0 : nb;                     // softin_pass: what the call can hold, or nothing
        std::vector<float> sx((size_t)stage_cap, std::nanf(""));               // LDS does not survive a launch
        memset((void *)lds.data(), 0xA5, sizeof(SoftinM20Lds));
        memset((void *)rec.data(), 0xEE, (size_t)cap * sizeof(sonde_m20_frame_t));
        unsigned count = 0;
        emu::run_workgroup(64, [&](int tid) {
            m20_wave_channel(chan.data(), soft + at, nb, invert ? -1.f : 1.f, 0.8f, doskip, lds.data(), sx.data(), stage_cap, rec.data(), &count, cap, 0, tid);
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
        const SoftinM20Chan &c = chan[0];
        end->mode = c.mode; end->inv = c.inv; end->mpos = c.mpos; end->mhalf = c.mhalf; end->mbit0 = c.mbit0; end->mskip = c.mskip; end->ms1 = c.ms1; end->mv = c.mv;
        end->bits_in = c.bits_in; end->hdr_bit = c.hdr_bit;
    }
    return got;
}

extern "C" int emu_m20_verdicts(const unsigned char *frame, sonde_m20_frame_t *o) {
    if (!frame || !o) return SONDE_E_ARG;
    memset(o, 0, sizeof *o);
    memcpy(o->frame, frame, M20_NBYTES);
    std::vector<unsigned char> fr(frame, frame + M20_NBYTES);                  // (exactly the bytes a frame has: a read behind them is the sanitizer's to see)
    emu::run_workgroup(64, [&](int tid) { m20_wave_verdicts(fr.data(), o, tid); });
    return 0;
}
