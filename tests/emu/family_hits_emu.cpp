// family_hits_emu.cpp — test infrastructure: the per-hit device decoders of generic engines (csrc/sonde_family_hits_dev.h: per kind the bit stage of the sample form,
// then the end-of-frame routine of the kind's soft-bit consumer) compiled for the CPU under wave_emu.h, driven the way k_family_hits (sonde_family_hits.hip) is
// launched: `grid` workgroups of one wave, each over the ring records [start, end) it owns, then the {done, ticket} hand-over.
//   emu_family_run(kind, ecc, soft, stride, nbits, mv, max_frames, start, end, grid, out, done)
//       soft / nbits / mv (null: 0) by ring SLOT (max_frames of them): the hit in slot s has nbits[s] valid soft bits at soft + s * stride and the header score mv[s];
//       its channel is s.  Records of the counter values [start, end) -> out[slot]; the caller fills `out` beforehand, so a slot nothing wrote keeps that.  done[2]
//       = {done, ticket} before and after.  LDS does not survive a workgroup: every workgroup starts on 0xA5 bytes.
#include "wave_emu.h"
#include "../../radiosonde_auto_rx_amd/csrc/sonde_family_hits_dev.h"
#include <cstring>
#include <vector>

namespace {
struct EmuRecs {
    const int *nbits; const float *mv;
    FamilyHitIn operator()(const unsigned slot) const { FamilyHitIn h; h.channel = (int32_t)slot; h.nv = nbits[slot]; h.mv_pos = 0u; h.mv = mv ? mv[slot] : 0.f; return h; }
};

template <class K>
void run_grid(const FamilyArgs &a, const EmuRecs &recs, const unsigned start, const unsigned end, const int grid, unsigned *done) {
    for (int block = 0; block < grid; block++) {
        std::vector<typename K::Lds> lds(1);
        memset((void *)lds.data(), 0xA5, sizeof(typename K::Lds));
        emu::run_workgroup(64, [&](int tid) {
            family_wave_records<K>(a, recs, start, end, block, grid, lds.data(), tid);
            family_wave_ticket(done, end, grid, tid);
        });
    }
}
}  // namespace

extern "C" int emu_family_run(int kind, int ecc, const float *soft, long long stride, const int *nbits, const float *mv, int max_frames, unsigned start, unsigned end,
                              int grid, sonde_family_hit_t *out, unsigned *done) {
    const int NB = family_kind_bits(kind);
    if (!NB || !soft || !nbits || !out || !done || max_frames < 1 || grid < 1 || stride < NB || (kind == SONDE_RS92 && !ecc)) return SONDE_E_ARG;
    for (int s = 0; s < max_frames; s++) if (nbits[s] < 0 || nbits[s] > stride) return SONDE_E_ARG;
    std::vector<uint32_t> tab((size_t)IMET54_TAB_N);
    imet54_crc_table(tab.data());
    // GF(2^8) / 0x11D, alpha = 2: the tables of sonde::gf_exp_table() / gf_log_table() (RS(255,231) of RS41 and RS92)
    std::vector<uint8_t> gf(768, 0);
    { unsigned x = 1; for (int i = 0; i < 255; i++) { gf[i] = (uint8_t)x; gf[512 + x] = (uint8_t)i; x <<= 1; if (x & 0x100) x ^= 0x11D; } }      // GF_genTab, f = 0x11D
    for (int i = 255; i < 512; i++) gf[i] = gf[i - 255];
    gf[512] = 0;
    const FamilyArgs a{soft, stride, ecc, max_frames, tab.data(), gf.data(), out};
    const EmuRecs recs{nbits, mv};
    switch (kind) {
        case SONDE_MEISEI: run_grid<FamilyMeisei>(a, recs, start, end, grid, done); break;
        case SONDE_IMET54: run_grid<FamilyImet54>(a, recs, start, end, grid, done); break;
        case SONDE_MTS01:  run_grid<FamilyMts01>(a, recs, start, end, grid, done); break;
        default:           run_grid<FamilyRs92>(a, recs, start, end, grid, done); break;
    }
    return 0;
}

extern "C" int emu_family_kind_bits(int kind) { return family_kind_bits(kind); }
extern "C" int emu_family_lds_bytes(int kind) {
    return kind == SONDE_MEISEI ? (int)sizeof(SoftinMeiseiLds) : kind == SONDE_IMET54 ? (int)sizeof(SoftinImet54Lds) : kind == SONDE_MTS01 ? (int)sizeof(SoftinMts01Lds)
         : kind == SONDE_RS92 ? (int)sizeof(SoftinRs92Lds) : SONDE_E_ARG;
}
