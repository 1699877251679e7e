// lms6_hits_emu.cpp — test infrastructure: the per-hit LMS6 / LMS-X decoder of generic engines (csrc/sonde_lms6_hits_dev.h: the bit stage of sonde_lms6_dec_block,
// then the soft-bit consumer's lms6_wave_decode) compiled for the CPU under wave_emu.h, driven the way k_lms6_hits (sonde_lms6_hits.hip) is launched: `grid`
// workgroups of one wave, each over the ring records [start, end) it owns, then the {done, ticket} hand-over.
//   emu_lms6_hits_run(vit, nb, soft, stride, nbits, mv, max_frames, start, end, grid, out, done)
//       nb = the engine's block length, 4096 or 4720.  soft / nbits / mv by ring SLOT (max_frames of them): the hit in slot s has nbits[s] valid soft bits at
//       soft + s * stride and the header score mv[s]; its channel is s.  Records of the counter values [start, end) -> out[slot]; the caller fills `out`
//       beforehand, so a slot nothing wrote keeps that.  done[2] = {done, ticket} before and after.  LDS does not survive a workgroup: every workgroup starts on
//       0xA5 bytes.
#include "wave_emu.h"
#include "../../radiosonde_auto_rx_amd/csrc/sonde_lms6_hits_dev.h"
#include <cstring>
#include <vector>

namespace {
struct EmuRecs {
    const int *nbits; const float *mv;
    FamilyHitIn operator()(const unsigned slot) const { FamilyHitIn h; h.channel = (int32_t)slot; h.nv = nbits[slot]; h.mv_pos = 0u; h.mv = mv[slot]; return h; }
};
}  // namespace

extern "C" int emu_lms6_hits_run(int vit, int nb, const float *soft, long long stride, const int *nbits, const float *mv, int max_frames, unsigned start, unsigned end,
                                 int grid, sonde_lms6_hit_t *out, unsigned *done) {
    if ((vit != 1 && vit != 2) || (nb != LMS6_HIT_BITS6 && nb != LMS6_HIT_BITSX) || !soft || !nbits || !mv || !out || !done || max_frames < 1 || grid < 1 || stride < nb)
        return SONDE_E_ARG;
    for (int s = 0; s < max_frames; s++) if (nbits[s] < 0 || nbits[s] > stride) return SONDE_E_ARG;
    const Lms6HitsArgs a{soft, stride, vit, nb, max_frames, out};
    const EmuRecs recs{nbits, mv};
    for (int block = 0; block < grid; block++) {
        std::vector<Lms6Lds> lds(1);
        memset((void *)lds.data(), 0xA5, sizeof(Lms6Lds));
        emu::run_workgroup(64, [&](int tid) {
            lms6_wave_records(a, recs, start, end, block, grid, lds.data(), tid);
            family_wave_ticket(done, end, grid, tid);
        });
    }
    return 0;
}

extern "C" int emu_lms6_hits_lds_bytes(void) { return (int)sizeof(Lms6Lds); }
extern "C" int emu_lms6_hits_record_bytes(void) { return (int)sizeof(sonde_lms6_hit_t); }
