// m20_hits_emu.cpp — test infrastructure: the per-hit M20 decoder of base-rate and mixed engines (csrc/sonde_m20_hits_dev.h: differential decoding into the channel's
// persistent bit characters, bits2bytes, frame and block checksum) compiled for the CPU under wave_emu.h, driven the way k_m20_hits (sonde_m20_hits.hip) is
// launched: `grid` workgroups of one wave, each over the ring records [done[0], end) of the channels it owns, then the {done, ticket} hand-over.
//   emu_m20_hits_run(bits, nbits, channel, mv, n_channels, max_frames, end, grid, chars, out, done)
//       bits / nbits / channel / mv (null: 0) by ring SLOT (max_frames of them): the hit in slot s has nbits[s] valid hard bits, 8 a byte, LSB first, in the 165
//       bytes at bits + 165 s.  chars = the channels' characters, n_channels x 1328, before and after.  Records of the counter values [done[0], end) -> out[slot]; the
//       caller fills `out` beforehand, so a slot nothing wrote keeps that.  LDS does not survive a workgroup: every workgroup starts on 0xA5 bytes.
//   emu_m20_verdicts(frame172, out): m20_wave_verdicts alone on the bytes given (every length byte is reachable this way).
#include "wave_emu.h"
#include "../../radiosonde_auto_rx_amd/csrc/sonde_m20_hits_dev.h"
#include <cstring>

namespace {
struct EmuRecs {
    const uint8_t *bits; const int *nbits, *channel; const float *mv;
    M20HitIn operator()(const unsigned slot) const {
        M20HitIn h; h.channel = channel[slot]; h.nv = nbits[slot]; h.mv_pos = 0u; h.mv = mv ? mv[slot] : 0.f; h.bits = bits + (size_t)slot * M20_NBYTES; return h;
    }
};
}  // namespace

extern "C" int emu_m20_hits_run(const uint8_t *bits, const int *nbits, const int *channel, const float *mv, int n_channels, int max_frames, unsigned end, int grid,
                                char *chars, sonde_m20_frame_t *out, unsigned *done) {
    if (!bits || !nbits || !channel || !chars || !out || !done || n_channels < 1 || max_frames < 1 || grid < 1) return SONDE_E_ARG;
    for (int s = 0; s < max_frames; s++) if (nbits[s] < 0 || nbits[s] > M20_NBITS || channel[s] < 0 || channel[s] >= n_channels) return SONDE_E_ARG;
    const M20HitsArgs a{n_channels, max_frames, chars, out};
    const EmuRecs recs{bits, nbits, channel, mv};
    for (int block = 0; block < grid; block++) {
        unsigned char lds[M20_REC_BYTES];
        memset(lds, 0xA5, sizeof lds);
        const unsigned start = done[0];                                // (only the last workgroup to finish moves it)
        emu::run_workgroup(64, [&](int tid) {
            m20_wave_records(a, recs, start, end, block, grid, lds, tid);
            m20_wave_ticket(done, end, grid, tid);
        });
    }
    return 0;
}

extern "C" int emu_m20_verdicts(const uint8_t *frame172, sonde_m20_frame_t *out) {
    if (!frame172 || !out) return SONDE_E_ARG;
    emu::run_workgroup(64, [&](int tid) { m20_wave_verdicts(frame172, out, tid); });
    return 0;
}

extern "C" int emu_m20_hits_lds_bytes() { return M20_REC_BYTES; }
extern "C" int emu_m20_chan_chars() { return M20_CHAN_CHARS; }
