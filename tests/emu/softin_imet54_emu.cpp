// softin_imet54_emu.cpp — test infrastructure: the device iMet-54 soft-bit consumer (csrc/sonde_softin_imet54_dev.h: header search with the ring left as it is, 8N1
// characters on a lane per character, de-interleave + Hamming(8,4) on a lane per codeword, both check sums as XOR sums over the wave) compiled for the CPU under
// wave_emu.h, driven the way sonde_softin_dev_push_device drives k_softin_imet54: one wave per call, the call's soft decisions staged up to M10_STAGE_MAX, a record
// buffer of `cap` frames per launch.
//   emu_imet54_run(soft, n, calls, n_calls, invert, inv, aut, ecc, cap, recs, max_recs, n_dropped, end)
//       the stream in calls of calls[0], calls[1], .. symbols (the last length repeats until the stream is consumed) through one channel; the frames the host
//       would fetch -> recs (returns their number), frames beyond `cap` of a launch -> *n_dropped, the channel's state behind the last call -> *end
//   emu_imet54_end(chars[220], ecc, rec)
//       the end-of-frame step alone on a caller's 220 characters: frame bytes, ecc sums and check-sum verdicts -> *rec
//   emu_imet54_header_mask()
//       the 40 header symbols as the search holds them, symbol i in bit i
#include "wave_emu.h"
#include "../../radiosonde_auto_rx_amd/csrc/sonde_softin_imet54_dev.h"
#include <cmath>
#include <cstring>
#include <vector>

static uint32_t g_tab[IMET54_TAB_N];                                           // as sonde_softin_dev_create_imet54 uploads it
static void tab_init() {
    static bool ready = false;
    if (ready) return;
    imet54_crc_table(g_tab);
    ready = true;
}

// SoftinImet54Chan without the characters of the frame in progress
struct EmuImet54State { int mode, inv, done, carry_n; float mv; int pad; unsigned long long bits_in, hdr_bit; float carry[IMET54_CHARSYM]; float hist[IMET54_HEADLEN]; };

extern "C" int emu_imet54_run(const float *soft, int n, const int *calls, int n_calls, int invert, int inv, int aut, int ecc, int cap, SoftinImet54Rec *recs, int max_recs,
                              int *n_dropped, EmuImet54State *end) {
    if (!soft || n < 0 || !calls || n_calls < 1 || cap < 1 || max_recs < 0 || (max_recs > 0 && !recs)) return SONDE_E_ARG;
    for (int i = 0; i < n_calls; i++) if (calls[i] < 1) return SONDE_E_ARG;
    tab_init();
    std::vector<SoftinImet54Chan> chan(1);
    memset((void *)chan.data(), 0, sizeof(SoftinImet54Chan));                  // as sonde_softin_dev_create_imet54 leaves it
    chan[0].inv = inv ? 1 : 0;
    std::vector<SoftinImet54Lds> lds(1);
    std::vector<SoftinImet54Rec> rec((size_t)cap);
    int got = 0, dropped = 0, k = 0;
    for (int at = 0; at < n; k++) {
        const int want = calls[k < n_calls ? k : n_calls - 1], nb = n - at < want ? n - at : want;
        const int stage_cap = nb > M10_STAGE_MAX ? 0 : nb;                     // softin_pass: what the call can hold, or nothing
        std::vector<float> sx((size_t)stage_cap, std::nanf(""));               // LDS does not survive a launch
        memset((void *)lds.data(), 0xA5, sizeof(SoftinImet54Lds));
        memset((void *)rec.data(), 0xEE, (size_t)cap * sizeof(SoftinImet54Rec));
        unsigned count = 0;
        emu::run_workgroup(64, [&](int tid) {
            imet54_wave_channel(chan.data(), soft + at, nb, invert ? -1.f : 1.f, aut ? 1 : 0, ecc ? 1 : 0, 0.8f, g_tab, lds.data(), sx.data(), stage_cap, rec.data(), &count, cap, 0, tid);
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
        const SoftinImet54Chan &c = chan[0];
        end->mode = c.mode; end->inv = c.inv; end->done = c.done; end->carry_n = c.carry_n; end->mv = c.mv; end->pad = 0; end->bits_in = c.bits_in; end->hdr_bit = c.hdr_bit;
        memcpy(end->carry, c.carry, sizeof end->carry); memcpy(end->hist, c.hist, sizeof end->hist);
    }
    return got;
}

extern "C" int emu_imet54_end(const unsigned char *chars, int ecc, SoftinImet54Rec *rec) {
    if (!chars || !rec) return SONDE_E_ARG;
    tab_init();
    std::vector<SoftinImet54Lds> lds(1);
    memset((void *)lds.data(), 0xA5, sizeof(SoftinImet54Lds));
    memcpy(lds[0].chr, chars, IMET54_CHARS);
    Imet54Verdict v{};
    emu::run_workgroup(64, [&](int tid) { const Imet54Verdict e = imet54_wave_end(lds.data(), ecc ? 1 : 0, g_tab, tid); if (tid == 63) v = e; });
    memset((void *)rec, 0, sizeof *rec);
    rec->ecc_frm = v.ecc_frm; rec->ecc_tlm = v.ecc_tlm; rec->ecc_std = v.ecc_std; rec->crc_std = v.crc_std; rec->crc_cont = v.crc_cont;
    memcpy(rec->frame, lds[0].fr, IMET54_FRAME);
    return 0;
}

extern "C" unsigned long long emu_imet54_header_mask() { return imet54_header_mask(); }
