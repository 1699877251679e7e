// mrz_hits_emu.cpp — test infrastructure: the per-hit MRZ decoder of generic engines (csrc/sonde_mrz_hits_dev.h: the bit stage of sonde_mrz_dec_frame, then the
// soft-bit consumer's mrz_wave_end under both frame lengths) compiled for the CPU under wave_emu.h, driven the way k_mrz_hits (sonde_mrz_hits.hip) is launched:
// `grid` workgroups of one wave, each over the ring records [start, end) it owns, then the {done, ticket} hand-over.
//   emu_mrz_hits_run(bits_ofs, soft, stride, nbits, mv, max_frames, start, end, grid, out, done)
//       soft / nbits / mv (null: 0) by ring SLOT (max_frames of them): the hit in slot s has nbits[s] valid soft bits at soft + s * stride and the header score mv[s];
//       its channel is s.  Records of the counter values [start, end) -> out[slot]; the caller fills `out` beforehand, so a slot nothing wrote keeps that.  done[2]
//       = {done, ticket} before and after.  LDS does not survive a workgroup: every workgroup starts on 0xA5 bytes.
#include "wave_emu.h"
#include "../../radiosonde_auto_rx_amd/csrc/sonde_mrz_hits_dev.h"
#include <cstring>
#include <vector>

namespace {
struct EmuRecs {
    const int *nbits; const float *mv;
    FamilyHitIn operator()(const unsigned slot) const { FamilyHitIn h; h.channel = (int32_t)slot; h.nv = nbits[slot]; h.mv_pos = 0u; h.mv = mv ? mv[slot] : 0.f; return h; }
};
}  // namespace

extern "C" int emu_mrz_hits_run(int bits_ofs, const float *soft, long long stride, const int *nbits, const float *mv, int max_frames, unsigned start, unsigned end,
                                int grid, sonde_family_hit_t *out, unsigned *done) {
    if (bits_ofs < 0 || bits_ofs > 64 || !soft || !nbits || !out || !done || max_frames < 1 || grid < 1 || stride < MRZ_HIT_BITS) return SONDE_E_ARG;
    for (int s = 0; s < max_frames; s++) if (nbits[s] < 0 || nbits[s] > stride) return SONDE_E_ARG;
    const MrzHitsArgs a{soft, stride, bits_ofs, max_frames, out};
    const EmuRecs recs{nbits, mv};
    for (int block = 0; block < grid; block++) {
        std::vector<SoftinMrzLds> lds(1);
        memset((void *)lds.data(), 0xA5, sizeof(SoftinMrzLds));
        emu::run_workgroup(64, [&](int tid) {
            mrz_wave_records(a, recs, start, end, block, grid, lds.data(), tid);
            family_wave_ticket(done, end, grid, tid);
        });
    }
    return 0;
}

extern "C" int emu_mrz_hits_bits(void) { return MRZ_HIT_BITS; }
extern "C" int emu_mrz_hits_lds_bytes(void) { return (int)sizeof(SoftinMrzLds); }
