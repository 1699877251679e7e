// softin_lms6_emu.cpp — test infrastructure: the device LMS6 / LMS-X soft-bit consumer (csrc/sonde_vit_dev.h: header search, block assembly, wave Viterbi, deconv,
// bits2bytes) compiled for the CPU under wave_emu.h, driven the way sonde_softin_dev_push_device drives k_softin_lms6: one wave per call, and with auto detection
// a relaunch per completed block after the host decoder (sonde_lms6_dec_block_bytes) has said how long the next block is.
//   emu_lms6_run(soft, n, call, invert, opts, out, outlen)   the stream in calls of `call` soft bits through one channel; the text of all blocks -> out
// Built together with csrc/sonde_lms6_fields.cpp and csrc/sonde_ecc.cpp (host code, no GPU runtime).
#include "wave_emu.h"
#include "../../radiosonde_auto_rx_amd/csrc/sonde_vit_dev.h"
#include "../../include/sonde_hip.h"
#include "../../include/sonde_lms6.h"
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

extern "C" int emu_lms6_run(const float *soft, int n, int call, int invert, const sonde_lms6_opts_t *opts, char *out, size_t outlen, int *n_blocks, int *n_launches) {
    if (!soft || n < 0 || call < 1 || !opts || !out) return SONDE_E_ARG;
    sonde_lms6_opts_t o = *opts;
    if (o.json) { if (!o.ecc) o.ecc = 1; if (!o.vit) o.vit = 1; }
    if (o.vit != 1 && o.vit != 2) return SONDE_E_ARG;
    sonde_lms6_dec_t *dec = nullptr;
    { const int rc = sonde_lms6_dec_create(&o, &dec); if (rc) return rc; }
    std::vector<Lms6Chan> chan(1);
    memset((void *)chan.data(), 0, sizeof(Lms6Chan));
    chan[0].pos = LMS6_BLOCKSTART; chan[0].rawblk_len = sonde_lms6_dec_block_bits(dec) + LMS6_BLOCKSTART;
    std::vector<Lms6Lds> lds(1);
    const int cap = 8;
    std::vector<Lms6Block> rec((size_t)cap);
    std::string text;
    char buf[4096];
    int blocks = 0, launches = 0, rc = 0;
    for (int at = 0; at < n && rc == 0; at += call) {
        const int nb = n - at < call ? n - at : call;
        for (;;) {
            unsigned count = 0;
            memset((void *)lds.data(), 0xA5, sizeof(Lms6Lds));                     // LDS does not survive a launch
            emu::run_workgroup(64, [&](int tid) {
                lms6_wave_channel(chan.data(), soft + at, nb, invert ? -1.f : 1.f, o.vit, o.typ == 0, (const unsigned char *)sonde_lms6_raw_header(), lds.data(), rec.data(), &count, cap, 0, tid);
            });
            launches++;
            bool more = false;
            for (unsigned i = 0; i < count && (int)i < cap; i++) {
                const Lms6Block &b = rec[i];
                const int len = sonde_lms6_dec_block_bytes(dec, b.bytes, b.blen, b.pos, b.mv, std::nanf(""), std::nan(""), buf, sizeof buf);
                if (len < 0) { rc = len; break; }
                text += buf; blocks++;
                chan[0].rawblk_len = sonde_lms6_dec_block_bits(dec) + LMS6_BLOCKSTART;
                more = more || b.more;
            }
            if (!more || rc) break;
        }
    }
    sonde_lms6_dec_destroy(dec);
    if (n_blocks) *n_blocks = blocks;
    if (n_launches) *n_launches = launches;
    if (rc) return rc;
    if (text.size() + 1 > outlen) return SONDE_E_ARG;
    memcpy(out, text.c_str(), text.size() + 1);
    return (int)text.size();
}
