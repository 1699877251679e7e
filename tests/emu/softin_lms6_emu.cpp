// softin_lms6_emu.cpp — test infrastructure: the device LMS6 / LMS-X soft-bit consumer (csrc/sonde_vit_dev.h: header search, block assembly, wave Viterbi, deconv,
// bits2bytes) compiled for the CPU under wave_emu.h, driven the way sonde_softin_dev_push_device drives k_softin_lms6: one wave per call, and with auto detection
// a relaunch per completed block after the host decoder (sonde_lms6_dec_block_bytes) has said how long the next block is.
//   emu_lms6_run(soft, n, call, invert, opts, out, outlen)   the stream in calls of `call` soft bits through one channel; the text of all blocks -> out
//   emu_lms6_run_rec(..., cap, recs, max_recs, n_dropped)     the same with a record buffer of `cap` blocks per launch; what the device hands the host per block -> recs
//   emu_lms6_decode(sb, len, bytes, blen, err)                lms6_wave_decode alone on a caller's block sb[0 .. len): every position is the caller's, the first 80 too
// Built together with csrc/sonde_lms6_fields.cpp and csrc/sonde_ecc.cpp (host code, no GPU runtime).
#include "wave_emu.h"
#include "../../radiosonde_auto_rx_amd/csrc/sonde_vit_dev.h"
#include "../../include/sonde_hip.h"
#include "../../include/sonde_lms6.h"
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

// what a Lms6Block says besides its bytes
struct EmuLms6Rec { int pos, err, blen, more, type; float mv; unsigned long long hdr_bit; };      // type: the host decoder's, in effect after the block

extern "C" int emu_lms6_decode(const float *sb, int len, unsigned char *bytes, int *blen, int *err) {
    if (!sb || !bytes || !blen || !err || len < 12 || len > LMS6_RAWBLKX) return SONDE_E_ARG;
    std::vector<Lms6Lds> lds(1);
    memset((void *)lds.data(), 0xA5, sizeof(Lms6Lds));
    memcpy(lds[0].sb, sb, (size_t)len * sizeof(float));
    std::vector<unsigned char> by(LMS6_BB_LEN + 4, 0xEE);
    int bl[64], er[64];
    emu::run_workgroup(64, [&](int tid) { bl[tid] = lms6_wave_decode(lds.data(), len, by.data(), &er[tid], tid); });
    for (int l = 1; l < 64; l++) if (bl[l] != bl[0] || er[l] != er[0]) return SONDE_E_ARG;      // (wave-uniform results)
    memcpy(bytes, by.data(), LMS6_BB_LEN);
    *blen = bl[0]; *err = er[0];
    return 0;
}

extern "C" int emu_lms6_run_rec(const float *soft, int n, int call, int invert, const sonde_lms6_opts_t *opts, int cap, char *out, size_t outlen, int *n_blocks, int *n_launches,
                                EmuLms6Rec *recs, int max_recs, int *n_dropped) {
    if (!soft || n < 0 || call < 1 || !opts || !out || cap < 1 || (max_recs > 0 && !recs)) return SONDE_E_ARG;
    sonde_lms6_opts_t o = *opts;
    if (o.json) { if (!o.ecc) o.ecc = 1; if (!o.vit) o.vit = 1; }
    if (o.vit != 1 && o.vit != 2) return SONDE_E_ARG;
    sonde_lms6_dec_t *dec = nullptr;
    { const int rc = sonde_lms6_dec_create(&o, &dec); if (rc) return rc; }
    std::vector<Lms6Chan> chan(1);
    memset((void *)chan.data(), 0, sizeof(Lms6Chan));
    chan[0].pos = LMS6_BLOCKSTART; chan[0].rawblk_len = sonde_lms6_dec_block_bits(dec) + LMS6_BLOCKSTART;
    std::vector<Lms6Lds> lds(1);
    std::vector<Lms6Block> rec((size_t)cap);
    std::string text;
    char buf[4096];
    int blocks = 0, launches = 0, rc = 0, dropped = 0;
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
            if ((int)count > cap) dropped += (int)count - cap;
            for (unsigned i = 0; i < count && (int)i < cap; i++) {
                const Lms6Block &b = rec[i];
                const int len = sonde_lms6_dec_block_bytes(dec, b.bytes, b.blen, b.pos, b.mv, std::nanf(""), std::nan(""), buf, sizeof buf);
                if (len < 0) { rc = len; break; }
                if (blocks < max_recs) { EmuLms6Rec &r = recs[blocks]; r.pos = b.pos; r.err = b.err; r.blen = b.blen; r.more = b.more; r.type = sonde_lms6_dec_type(dec, nullptr); r.mv = b.mv; r.hdr_bit = b.hdr_bit; }
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
    if (n_dropped) *n_dropped = dropped;
    if (rc) return rc;
    if (text.size() + 1 > outlen) return SONDE_E_ARG;
    memcpy(out, text.c_str(), text.size() + 1);
    return (int)text.size();
}

extern "C" int emu_lms6_run(const float *soft, int n, int call, int invert, const sonde_lms6_opts_t *opts, char *out, size_t outlen, int *n_blocks, int *n_launches) {
    return emu_lms6_run_rec(soft, n, call, invert, opts, 8, out, outlen, n_blocks, n_launches, nullptr, 0, nullptr);
}
