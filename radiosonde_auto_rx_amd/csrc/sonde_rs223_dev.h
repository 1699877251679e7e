// sonde_rs223_dev.h — RS(255,223) CCSDS on the device: the errors-only decoder of LMS6-403 / LMS-X blocks on ONE wavefront (a polynomial coefficient per lane), and
// what proc_frame asks of it per block (k_lms6_rs, sonde_lms6_rs.hip).  Behaviour reproduced (not code): bch_ecc_mod.c rs_decode :877-965 with nera = 0 (syndromes
// :638-649, polyGF_lfsr :547-578, poly_divmod :410-454, poly_mul :469-490, Chien loop :926-940, forney :596-612 with b = 112 > 1) for the code of bch_ecc_mod.h:99:
// GF(2^8) / 0x187, generator roots (alpha^11)^(112 + i), t = 16, positions through ip = 116; and lms6Xmod.c proc_frame :881-989 as far as it depends on the block
// bytes alone.  The key equation is solved by the same extended Euclid on (S, x^32) with the same stop rule and the same acceptance tests as sonde_rs_dev.h does for
// RS(255,231), so a word the reference cannot repair fails here with the same code, and a word it miscorrects is miscorrected into the same bytes.
//
//   rs223_wave_syndromes   S_i = cw((alpha^11)^(112 + i)), i < 32: lane l does syndrome l & 31 over the coefficients [128 (l >> 5), 128 (l >> 5) + 128) by Horner,
//                          the upper half scaled by x^128; the two halves meet through 32 bytes of LDS.  Field arithmetic is exact: any split gives the same bytes.
//   rs223_wave_decode      rs_decode of one word; error positions / values in the reference's order (ascending x of the Chien search), found by a prefix
//                          population count of the root ballots.
//   lms6_rs_wave_record    one block record -> one sonde_lms6_rs_t (include/sonde_hip.h): the decoder under each hypothesis the host decoder can ask for.
//   lms6_rs_wave_records   the grid-stride loop of k_lms6_rs with the slot and ring rules of lms6_wave_records (sonde_lms6_hits_dev.h).
//
// Compiled twice, like sonde_rs_dev.h: by hipcc into k_lms6_rs and by g++ under tests/emu/wave_emu.h (tests/emu/lms6_rs_emu.cpp).  Control flow around every rsw_*
// call is wave-uniform.  No indexed local arrays: the four x a lane looks at are unrolled.
#ifndef SONDE_RS223_DEV_H
#define SONDE_RS223_DEV_H
#include "../../include/sonde_hip.h"                                    // sonde_lms6_rs_t
#include "sonde_rs_dev.h"

#define RS223_T       16
#define RS223_2T      32
#define RS223_B       112                                              // first root (bch_ecc_mod.h:99)
#define RS223_P       11                                               // beta = alpha^11
#define RS223_IP      116                                              // 11 * 116 = 1 mod 255
#define LMS6_RS_BB    308                                              // block_bytes[FRAME_LEN + 8]
#define LMS6_RS_SYNC  5                                                // SYNC_LEN: the codeword of a block starts here (lms6Xmod.c:885)

// LDS of a wave: tables 768 + codeword 256 + Lambda / Omega 64 + staged block bytes 320 = 1408 B
struct Lms6RsLds {
    uint8_t exp[512], log[256];                    // GF(256) / 0x187: sonde_ecc_tables() of SONDE_ECC_RS255CCSDS
    uint8_t cw[256];                               // the word in polynomial order, cw[255] = 0
    uint8_t scr[64];                               // syndrome halves; then Lambda [0, 32) and Omega [32, 64)
    uint8_t bb[320];                               // the block bytes, zero behind blen
};

// S[lane] for lane < 32 (0 above) of the word in cw[0 .. 255)
static RSW_DEV int rs223_wave_syndromes(const uint8_t *cw, uint8_t *scr, const RsGf g, const int lane) {
    const int j = lane & 31, half = lane >> 5;
    const int lx = (RS223_P * (RS223_B + j)) % 255;                     // log of the evaluation point (:641)
    int h = 0;
    for (int i = 127; i >= 0; i--) {
        const int n = 128 * half + i;
        h = rs_gf_mul_l(g, h, lx) ^ (n < 255 ? cw[n] : 0);
    }
    if (half) scr[j] = (uint8_t)rs_gf_mul_l(g, h, (128 * lx) % 255);
    rsw_wave_sync();
    const int s = half ? 0 : (h ^ scr[j]);
    rsw_wave_sync();                                                   // scr is Lambda / Omega next
    return s;
}

// Lambda(x) at the x of logarithm lx, by Horner from scr
static RSW_DEV int rs223_eval_lambda(const uint8_t *scr, const int dL, const int lx, const RsGf g) {
    int y = 0;
    for (int n = dL; n >= 0; n--) y = rs_gf_mul_l(g, y, lx) ^ scr[n];
    return y;
}
// forney (:596-612) for b > 1: Y = x^(b-1) Omega(x) / Lambda'(x), 0 when Lambda'(x) = 0; Lambda' keeps the odd coefficients, one degree down
static RSW_DEV int rs223_forney(const uint8_t *scr, const int dL, const int dO, const int lx, const RsGf g) {
    int w = 0, z = 0;
    for (int n = dO; n >= 0; n--) w = rs_gf_mul_l(g, w, lx) ^ scr[32 + n];
    for (int n = dL - 1; n >= 0; n--) z = rs_gf_mul_l(g, z, lx) ^ ((n & 1) ? 0 : scr[n + 1]);
    if (!z) return 0;
    return rs_gf_mul_l(g, rs_gf_mul(g, w, rs_gf_inv(g, z)), ((RS223_B - 1) * lx) % 255);
}
// one root of the Chien search: its place `rank` in the reference's order -> pos / val, the word patched
static RSW_DEV void rs223_root(uint8_t *cw, uint8_t *pos, uint8_t *val, const uint8_t *scr, const int dL, const int dO, const int lx, const int rank, const RsGf g) {
    const int p = (((255 - lx) % 255) * RS223_IP) % 255;                // err_pos = log(1 / x) ip mod 255 (:930)
    const int v = rs223_forney(scr, dL, dO, lx, g);
    pos[rank] = (uint8_t)p; val[rank] = (uint8_t)v;
    cw[p] ^= (uint8_t)v;                                               // (x -> p is one to one: a byte has one writer)
}

// rs_decode() of one codeword on one wave.  syn = S[lane] for lane < 32 (0 above), cw = the 255 codeword bytes in LDS (repaired in place on success, untouched
// otherwise), pos / val = 16 bytes each, written here whatever the outcome: the error positions (the reference's codeword indices) and values in the reference's
// order on success, zero behind them and on failure.  scr = 64 bytes of LDS owned by this wave.  Returns what rs_decode returns: 0 (clean), the number of repaired
// symbols, -1 (fewer roots than the locator's degree), -2 (Lambda(0) = 0), -3 (deg Omega >= deg Lambda).
static RSW_DEV int rs223_wave_decode(uint8_t *cw, const int syn, uint8_t *pos, uint8_t *val, uint8_t *scr, const RsGf g, const int lane) {
    int ret = 0, dL = 0, dO = -1;
    int lam = 0, om = 0;
    if (rsw_ballot(syn != 0) != 0) {
        // polyGF_lfsr: r0 = S, r1 = x^32, s0 = 1, s1 = 0; while deg r1 >= 16: (quo, rem) = r0 / r1; r0 = r1; r1 = rem; s2 = quo s1 + s0; ..
        int r0 = syn, r1 = (lane == RS223_2T) ? 1 : 0, s0 = (lane == 0) ? 1 : 0, s1 = 0;
        int d1 = RS223_2T;
        while (d1 >= RS223_T) {
            int dp = rsw_deg(r0);
            int quo = 0, rem = r0;                                     // deg p < deg q: d = 0, r = p (:433)
            if (dp >= d1) {
                const int lqi = g.log[rs_gf_inv(g, rsw_bcast(r1, d1))];
                while (dp >= d1) {
                    const int c = rs_gf_mul_l(g, rsw_bcast(rem, dp), lqi);
                    const int sh = dp - d1;
                    if (lane == sh) quo = c;
                    rem ^= rs_gf_mul_l(g, rsw_shfl_up(r1, sh, lane), g.log[c]);
                    dp = rsw_deg(rem);
                }
            }
            r0 = r1; r1 = rem;
            int s2 = s0;                                               // poly_mul(quo, s1) + s0
            const int dq = rsw_deg(quo);
            for (int i = 0; i <= dq; i++) {
                const int q = rsw_bcast(quo, i);
                const int t = rsw_shfl_up(s1, i, lane);
                if (q) s2 ^= rs_gf_mul_l(g, t, g.log[q]);
            }
            s0 = s1; s1 = s2;
            d1 = rsw_deg(r1);
        }
        dL = rsw_deg(s1); dO = d1;                                     // Lambda = s1, Omega = r1
        const int gamma = rsw_bcast(s1, 0);
        if (dO >= dL) ret = -3;
        else if (!gamma) ret = -2;
        else {
            const int lgi = g.log[rs_gf_inv(g, gamma)];
            lam = rs_gf_mul_l(g, s1, lgi); om = rs_gf_mul_l(g, r1, lgi);
            ret = 1;                                                   // (so far)
        }
    }
    int nroots = 0;
    if (ret > 0) {
        // Chien search over x = 1 .. 255 in this order (:926): lane l looks at x = l+1, l+65, l+129, l+193; the reference stops at the dL-th root, and a polynomial
        // of degree dL has no more
        if (lane < 32) { scr[lane] = (uint8_t)lam; scr[32 + lane] = (uint8_t)om; }
        rsw_wave_sync();
        const int lx0 = g.log[(lane + 1) & 255], lx1 = g.log[(lane + 65) & 255], lx2 = g.log[(lane + 129) & 255], lx3 = g.log[(lane + 193) & 255];
        const bool t0 = rs223_eval_lambda(scr, dL, lx0, g) == 0, t1 = rs223_eval_lambda(scr, dL, lx1, g) == 0, t2 = rs223_eval_lambda(scr, dL, lx2, g) == 0;
        const bool t3 = lane + 193 <= 255 && rs223_eval_lambda(scr, dL, lx3, g) == 0;
        const unsigned long long m0 = rsw_ballot(t0), m1 = rsw_ballot(t1), m2 = rsw_ballot(t2), m3 = rsw_ballot(t3);
        const int n0 = rsw_popcll(m0), n1 = n0 + rsw_popcll(m1), n2 = n1 + rsw_popcll(m2);
        nroots = n2 + rsw_popcll(m3);
        if (nroots < dL) ret = -1;
        else {
            const unsigned long long below = (1ull << lane) - 1ull;
            if (t0) rs223_root(cw, pos, val, scr, dL, dO, lx0, rsw_popcll(m0 & below), g);
            if (t1) rs223_root(cw, pos, val, scr, dL, dO, lx1, n0 + rsw_popcll(m1 & below), g);
            if (t2) rs223_root(cw, pos, val, scr, dL, dO, lx2, n1 + rsw_popcll(m2 & below), g);
            if (t3) rs223_root(cw, pos, val, scr, dL, dO, lx3, n2 + rsw_popcll(m3 & below), g);
            ret = nroots;
        }
    }
    if (ret <= 0) nroots = 0;
    if (lane >= nroots && lane < RS223_T) { pos[lane] = 0; val[lane] = 0; }
    rsw_wave_sync();
    return ret;
}

// frmsync_X (lms6Xmod.c:815-827) on block bytes: the position of 24 46 05 00 among 5 / 40 / 45, 0 when it is at none of them
static RSW_DEV bool lms6_rs_syncx_at(const uint8_t *p) { return p[0] == 0x24 && p[1] == 0x46 && p[2] == 0x05 && p[3] == 0x00; }
static RSW_DEV int lms6_rs_syncx(const uint8_t *bb) {
    if (lms6_rs_syncx_at(bb + LMS6_RS_SYNC)) return LMS6_RS_SYNC;
    if (lms6_rs_syncx_at(bb + LMS6_RS_SYNC + 35)) return LMS6_RS_SYNC + 35;
    if (lms6_rs_syncx_at(bb + LMS6_RS_SYNC + 40)) return LMS6_RS_SYNC + 40;
    return 0;
}

// head of a hypothesis by lane 0
static RSW_DEV void lms6_rs_head(sonde_lms6_rs_hyp_t *h, const int at, const int err, const int lane) { if (lane == 0) { h->at = at; h->err = err; } }
// a hypothesis whose decoder does not run
static RSW_DEV void lms6_rs_none(sonde_lms6_rs_hyp_t *h, const int at, const int lane) {
    lms6_rs_head(h, at, 0, lane);
    if (lane < RS223_T) { h->pos[lane] = 0; h->val[lane] = 0; }
}
// the decoder on bb[at .. at + 255), reversed into the codeword (lms6Xmod.c:885-889) -> *h; L->cw holds the word afterwards, repaired on success
static RSW_DEV int lms6_rs_run(Lms6RsLds *L, const int at, sonde_lms6_rs_hyp_t *h, const RsGf g, const int lane) {
    for (int j = lane; j < 256; j += 64) L->cw[j] = j < 255 ? L->bb[at + 254 - j] : 0;
    rsw_wave_sync();
    const int syn = rs223_wave_syndromes(L->cw, L->scr, g, lane);
    const int e = rs223_wave_decode(L->cw, syn, h->pos, h->val, L->scr, g, lane);
    lms6_rs_head(h, at, e, lane);
    return e;
}

// One block record: bytes[308] in device memory (read only; what lies behind blen counts as zero), blen, decoded -> *o, every byte written exactly once.
//   hX   the raw bytes at frmsync_X's position, when the sync is there and blen > 100 (proc_frame's type-10 branch :966-975); else at = 0 and nothing runs
//   h6   the raw bytes at 5 (the type-6 branch with --ecc :885-889), always
//   h6X  the type-10 branch on the bytes as h6 patched them (a type-6 block that falls through under auto detection); only when h6 repaired something,
//        else at = -1: the same as hX
static RSW_DEV void lms6_rs_wave_record(const uint8_t *bytes, const int blen, const int decoded, sonde_lms6_rs_t *o, Lms6RsLds *L, const int lane) {
    if (!decoded || blen <= 0) {
        lms6_rs_none(&o->h6, 0, lane); lms6_rs_none(&o->hX, 0, lane); lms6_rs_none(&o->h6X, 0, lane);
        return;
    }
    const RsGf g{L->exp, L->log};
    for (int k = lane; k < 320; k += 64) L->bb[k] = (k < blen && k < LMS6_RS_BB) ? bytes[k] : 0;
    rsw_wave_sync();
    const int atX = blen > 100 ? lms6_rs_syncx(L->bb) : 0;
    if (atX) lms6_rs_run(L, atX, &o->hX, g, lane); else lms6_rs_none(&o->hX, 0, lane);
    const int e6 = lms6_rs_run(L, LMS6_RS_SYNC, &o->h6, g, lane);
    if (e6 > 0) {
        for (int j = lane; j < 255; j += 64) L->bb[LMS6_RS_SYNC + j] = L->cw[254 - j];
        rsw_wave_sync();
        const int at6X = blen > 100 ? lms6_rs_syncx(L->bb) : 0;
        if (at6X) lms6_rs_run(L, at6X, &o->h6X, g, lane); else lms6_rs_none(&o->h6X, 0, lane);
    } else lms6_rs_none(&o->h6X, -1, lane);
}

// where the records lie: record of ring slot s at recs + s * stride, its bytes / blen / decoded at these offsets (off_decoded < 0: every record counts as decoded)
struct Lms6RsArgs {
    const uint8_t *recs; long long stride;
    int off_bytes, off_blen, off_decoded, max_frames;
    sonde_lms6_rs_t *out;                          // [max_frames]
};

// the tables into the wave's LDS: 768 bytes, tab = exp[512] | log[256]
static RSW_DEV void lms6_rs_wave_tables(Lms6RsLds *L, const uint8_t *tab, const int lane) {
    for (int k = lane; k < 512; k += 64) L->exp[k] = tab[k];
    for (int k = lane; k < 256; k += 64) L->log[k] = tab[512 + k];
    rsw_wave_sync();
}

// the loop of k_lms6_rs: records [start, end) of the ring, record i on workgroup i % grid, slot i % max_frames
static RSW_DEV void lms6_rs_wave_records(const Lms6RsArgs &a, unsigned start, const unsigned end, const int block, const int grid, Lms6RsLds *L, const int lane) {
    if ((int)(end - start) > a.max_frames) start = end - (unsigned)a.max_frames;                   // (what the ring no longer holds)
    for (unsigned i = start + (unsigned)block; (int)(end - i) > 0; i += (unsigned)grid) {
        const unsigned slot = i % (unsigned)a.max_frames;
        const uint8_t *r = a.recs + (size_t)slot * (size_t)a.stride;
        const int blen = *(const int *)(r + a.off_blen);
        const int decoded = a.off_decoded < 0 ? 1 : *(const int *)(r + a.off_decoded);
        lms6_rs_wave_record(r + a.off_bytes, blen, decoded, a.out + slot, L, lane);
        rsw_wave_sync();                                               // the LDS of this record is not touched by the next before every lane is through
    }
}
#endif
