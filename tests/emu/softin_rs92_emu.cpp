// softin_rs92_emu.cpp — test infrastructure: the device RS92 soft-bit consumer (csrc/sonde_softin_rs92_dev.h: header search with the ring emptied on every hit, 8N1
// bytes on a lane per byte, RS(255,231) of the finished frame on the wave) compiled for the CPU under wave_emu.h, driven the way sonde_softin_dev_push_device drives
// k_softin_rs92: one wave per call, the call's soft decisions staged up to M10_STAGE_MAX, a record buffer of `cap` frames per launch.
//   emu_rs92_run(soft, n, calls, n_calls, invert, inv, cap, recs, max_recs, n_dropped, end)
//       the stream in calls of calls[0], calls[1], .. symbols (the last length repeats until the stream is consumed) through one channel; the frames the host
//       would fetch -> recs (returns their number), frames beyond `cap` of a launch -> *n_dropped, the channel's state behind the last call -> *end
//   emu_rs92_ecc(frame[240])
//       the end-of-frame step alone (codeword layout, syndromes, rs255_wave_decode, write-back) on a caller's frame, in place; returns rs_decode's value
#include "wave_emu.h"
#include "../../radiosonde_auto_rx_amd/csrc/sonde_softin_rs92_dev.h"
#include <cmath>
#include <cstring>
#include <vector>

static uint8_t g_gf[768];                                                      // exp[512] ++ log[256], as sonde_softin_dev_create_rs92 uploads them
static void gf_init() {
    static bool ready = false;
    if (ready) return;
    unsigned x = 1;
    for (int i = 0; i < 255; i++) { g_gf[i] = (uint8_t)x; g_gf[512 + x] = (uint8_t)i; x <<= 1; if (x & 0x100) x ^= 0x11D; }   // GF_genTab, f = 0x11D (bch_ecc_mod.c:136)
    for (int i = 255; i < 512; i++) g_gf[i] = g_gf[i - 255];
    g_gf[512] = 0;
    ready = true;
}

// SoftinRs92Chan without the frame in progress
struct EmuRs92State { int mode, done, carry_n; float mv; unsigned long long bits_in, hdr_bit; float carry[RS92_BYTESYM]; float hist[RS92_HEADLEN]; };

extern "C" int emu_rs92_run(const float *soft, int n, const int *calls, int n_calls, int invert, int inv, int cap, SoftinRs92Rec *recs, int max_recs, int *n_dropped,
                            EmuRs92State *end) {
    if (!soft || n < 0 || !calls || n_calls < 1 || cap < 1 || max_recs < 0 || (max_recs > 0 && !recs)) return SONDE_E_ARG;
    for (int i = 0; i < n_calls; i++) if (calls[i] < 1) return SONDE_E_ARG;
    gf_init();
    std::vector<SoftinRs92Chan> chan(1);
    memset((void *)chan.data(), 0, sizeof(SoftinRs92Chan));                    // as sonde_softin_dev_create_rs92 leaves it
    std::vector<SoftinRs92Lds> lds(1);
    std::vector<SoftinRs92Rec> rec((size_t)cap);
    int got = 0, dropped = 0, k = 0;
    for (int at = 0; at < n; k++) {
        const int want = calls[k < n_calls ? k : n_calls - 1], nb = n - at < want ? n - at : want;
        const int stage_cap = nb > M10_STAGE_MAX ? 0 : nb;                     // softin_pass: what the call can hold, or nothing
        std::vector<float> sx((size_t)stage_cap, std::nanf(""));               // LDS does not survive a launch
        memset((void *)lds.data(), 0xA5, sizeof(SoftinRs92Lds));
        memset((void *)rec.data(), 0xEE, (size_t)cap * sizeof(SoftinRs92Rec));
        unsigned count = 0;
        emu::run_workgroup(64, [&](int tid) {
            rs92_wave_channel(chan.data(), soft + at, nb, invert ? -1.f : 1.f, inv ? 1 : 0, 0.8f, g_gf, lds.data(), sx.data(), stage_cap, rec.data(), &count, cap, 0, tid);
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
        const SoftinRs92Chan &c = chan[0];
        end->mode = c.mode; end->done = c.done; end->carry_n = c.carry_n; end->mv = c.mv; end->bits_in = c.bits_in; end->hdr_bit = c.hdr_bit;
        memcpy(end->carry, c.carry, sizeof end->carry); memcpy(end->hist, c.hist, sizeof end->hist);
    }
    return got;
}

extern "C" int emu_rs92_ecc(unsigned char *frame) {
    if (!frame) return SONDE_E_ARG;
    gf_init();
    std::vector<SoftinRs92Lds> lds(1);
    memset((void *)lds.data(), 0xA5, sizeof(SoftinRs92Lds));
    memcpy(lds[0].frame, frame, RS92_FRAME_LEN);
    memcpy(lds[0].gexp, g_gf, 512); memcpy(lds[0].glog, g_gf + 512, 256);
    int ret = 0;
    emu::run_workgroup(64, [&](int tid) { const int e = rs92_wave_ecc(lds.data(), tid); if (tid == 0) ret = e; });
    memcpy(frame, lds[0].frame, RS92_FRAME_LEN);
    return ret;
}
