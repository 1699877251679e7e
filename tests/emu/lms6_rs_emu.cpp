// lms6_rs_emu.cpp — test infrastructure: the device RS(255,223) decoder of LMS6 / LMS-X blocks (csrc/sonde_rs223_dev.h) compiled for the CPU under wave_emu.h, driven
// the way k_lms6_rs (sonde_lms6_rs.hip) is launched: `grid` workgroups of one wave, each over the records it owns.  The field tables are the product's own: the
// codec of csrc/sonde_ecc.cpp is compiled in (plain host C++), sonde_ecc_tables() of SONDE_ECC_RS255CCSDS.
//   emu_rs223_decode(cw[255], pos[16], val[16])    one word on one wave: syndromes and decoder; returns rs_decode's value, cw repaired in place on success
//   emu_lms6_rs_run(bytes, stride, blen, decoded | null, n, grid, out)
//       record i = 308 bytes at bytes + i * stride with blen[i] and decoded[i] (null: all decoded) -> out[i]; the caller fills `out` beforehand, so a byte nothing
//       wrote keeps that.  LDS does not survive a workgroup: every workgroup starts on 0xA5 bytes.
//   emu_lms6_rs_lds_bytes()                        sizeof(Lms6RsLds): what the kernel's static LDS must be
#include "wave_emu.h"
#include "../../radiosonde_auto_rx_amd/csrc/sonde_rs223_dev.h"
#include "../../radiosonde_auto_rx_amd/csrc/sonde_ecc.cpp"
#include <cstring>
#include <vector>

namespace {
struct EmuRec { int32_t blen, decoded; uint8_t bytes[LMS6_RS_BB]; };
const uint8_t *tables() {
    static uint8_t tab[768];
    static bool ready = false;
    if (!ready) {
        sonde_ecc_t *c = sonde_ecc_create(SONDE_ECC_RS255CCSDS);
        const uint8_t *e = nullptr, *l = nullptr;
        sonde_ecc_tables(c, &e, &l);
        memcpy(tab, e, 512); memcpy(tab + 512, l, 256);
        sonde_ecc_destroy(c);
        ready = true;
    }
    return tab;
}
}  // namespace

extern "C" int emu_rs223_decode(uint8_t *cw_io, uint8_t *pos, uint8_t *val) {
    std::vector<Lms6RsLds> lds(1);
    memset((void *)lds.data(), 0xA5, sizeof(Lms6RsLds));
    Lms6RsLds *L = lds.data();
    const uint8_t *tab = tables();
    int ret = 0;
    emu::run_workgroup(64, [&](int tid) {
        lms6_rs_wave_tables(L, tab, tid);
        for (int j = tid; j < 256; j += 64) L->cw[j] = j < 255 ? cw_io[j] : 0;
        rsw_wave_sync();
        const RsGf g{L->exp, L->log};
        const int syn = rs223_wave_syndromes(L->cw, L->scr, g, tid);
        const int e = rs223_wave_decode(L->cw, syn, pos, val, L->scr, g, tid);
        if (tid == 0) ret = e;
    });
    memcpy(cw_io, L->cw, 255);
    return ret;
}

extern "C" int emu_lms6_rs_run(const uint8_t *bytes, long long stride, const int32_t *blen, const int32_t *decoded, int n, int grid, sonde_lms6_rs_t *out) {
    if (!bytes || !blen || !out || n < 0 || grid < 1 || stride < LMS6_RS_BB) return SONDE_E_ARG;
    if (n == 0) return 0;
    std::vector<EmuRec> recs((size_t)n);
    for (int i = 0; i < n; i++) {
        recs[(size_t)i].blen = blen[i]; recs[(size_t)i].decoded = decoded ? decoded[i] : 1;
        memcpy(recs[(size_t)i].bytes, bytes + (size_t)i * (size_t)stride, LMS6_RS_BB);
    }
    const Lms6RsArgs a{(const uint8_t *)recs.data(), (long long)sizeof(EmuRec), (int)offsetof(EmuRec, bytes), (int)offsetof(EmuRec, blen), (int)offsetof(EmuRec, decoded), n, out};
    const uint8_t *tab = tables();
    for (int block = 0; block < grid; block++) {
        std::vector<Lms6RsLds> lds(1);
        memset((void *)lds.data(), 0xA5, sizeof(Lms6RsLds));
        emu::run_workgroup(64, [&](int tid) {
            lms6_rs_wave_tables(lds.data(), tab, tid);
            lms6_rs_wave_records(a, 0u, (unsigned)n, block, grid, lds.data(), tid);
        });
    }
    for (int i = 0; i < n; i++) if (memcmp(recs[(size_t)i].bytes, bytes + (size_t)i * (size_t)stride, LMS6_RS_BB)) return -100;      // the input is read only
    return 0;
}

extern "C" int emu_lms6_rs_lds_bytes(void) { return (int)sizeof(Lms6RsLds); }
extern "C" int emu_lms6_rs_record_bytes(void) { return (int)sizeof(sonde_lms6_rs_t); }
