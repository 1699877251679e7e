// sonde_softin_meisei_dev.h — `meisei100mod --softin [--ecc]` behind the modem on ONE wavefront per channel: header search on the half-symbol stream, biphase-S bits
// on a lane per bit, and at the end of a frame the 12 BCH(63,51) blocks with their padding and word-parity rules, one block at a time on the same wave.
// Behaviour reproduced (not code): demod/mod/meisei100mod.c main :654-776 (find_softbinhead on the 48 half symbols of :75 at 0.8 in EITHER polarity, 1152 half
// symbols behind the hit, the ring left as it is), biphi_s :213-229, the block loop :735-776; find_softbinhead / corr_softhdb are demod_mod.c:1692-1762,
// rs_decode_bch_gf2t2 is bch_ecc_mod.c:968-1043.  The host mirror is sonde_meisei_dec_push_soft (sonde_meisei_fields.cpp) with sonde_ecc_decode_bch_gf2t2.
//
//   search: a lane per stream position, softin_wave_score<48> (float first, the reference's double form wherever that is not safely below the threshold): that
//           value decides (fabs(mv) > 0.8f in either polarity; 0.8f itself and the NaN of an all-zero window are no hits) and is recorded with its sign.  There is
//           no polarity rule: every hit is accepted, the first of a round of 64 positions starts the frame.  The ring is NOT emptied on a hit and is advanced only
//           while searching: behind a frame the search resumes on the 48 half symbols of the header that frame was found by.
//   frame:  a lane per bit (bit j = 1 if half symbols 2 j and 2 j + 1 have the same hard value s >= 0, so -0.0 is a 1), 576 bits in nine rounds of 64, each round's
//           ballot ORed into the frame's bit words in LDS behind the 24 known header bits; an odd half symbol and the words so far survive a call in device memory.
//   end of frame (1152 half symbols behind the hit, --ecc): block k of subframe f is the 46 bits at 300 f + 24 + 46 k, cw[45 - j] = block bit j on lane 45 - j,
//           cw[46 .. 62] = 0.  bch63_wave_decode: every lane whose bit is set contributes alpha^p and alpha^3p (one word), the XOR over the wave is S1 and S3 (S2 =
//           S1^2, S4 = S2^2 hold for a binary word); S1 times the locator, S1 + S1^2 x + (S3 + S1^3) x^2, is evaluated at alpha^-p on lane p < 63 and ONE ballot is
//           the error-position mask; its population count against the degree says uncorrectable, its bits 46 .. 62 are the padding check, and both word parities
//           are population counts of the masked ballot of the corrected bits.  GF(2^6) products are six shift-and-add steps: no table, no indexed array.
//
// Only COMPLETE frames are delivered: a consumer behind a live modem has no end of input.
//
// Compiled twice, like sonde_softin_imet54_dev.h: by hipcc into k_softin_meisei (sonde_softin_dev.hip) and by g++ under tests/emu/wave_emu.h
// (tests/emu/softin_meisei_emu.cpp).  Control flow around every cross-lane primitive is wave-uniform.
#ifndef SONDE_SOFTIN_MEISEI_DEV_H
#define SONDE_SOFTIN_MEISEI_DEV_H
#include "sonde_softin_wave_dev.h"                                     // the staged call, softin_wave_score<HL>, the ring refresh, softin_wave_xor
// (no contraction: the reference is plain C on x86-64 — every product and sum rounded on its own)
#pragma clang fp contract(off)

#define MEISEI_HEADLEN  48                                            // half symbols of the header
#define MEISEI_NSYM     1152                                          // half symbols behind the header: 576 bits
#define MEISEI_HDRBITS  24
#define MEISEI_NBITS    600                                           // frame bits: subframe 0 at 0, subframe 1 at 300
#define MEISEI_WORDS    19                                            // 32-bit words of the frame's bits, bit i in bit i & 31 of word i >> 5
#define MEISEI_NBYTES   75
#define MEISEI_BLOCKS   12
#define MEISEI_BLKBITS  46
// the header meisei100mod hands to find_softbinhead (meisei100mod.c:75: 0x049DCE as biphase-S half symbols), half symbol i in bit i
static RSW_DEV unsigned long long meisei_header_mask() {
    const char h[MEISEI_HEADLEN + 1] = "101010101011010100101011001101001100101011001101";
    unsigned long long m = 0;
    for (int i = 0; i < MEISEI_HEADLEN; i++) m |= (unsigned long long)(h[i] & 1) << i;
    return m;
}
// the 24 bits that header stands for (000001001001110111001110), bit i in bit i
#define MEISEI_HDR24 0x73B920u

// a completed frame as the kernel leaves it (104 bytes)
struct SoftinMeiseiRec {
    int32_t  channel;
    float    mv;                   // score of the header in front of the frame (the double form, rounded), with its sign
    unsigned long long hdr_bit;    // half symbols read when the header matched
    uint8_t  block_err[MEISEI_BLOCKS];   // 0 / 1 / 2 corrected bits, 0xF padding or word parity, 0xE uncorrectable; subframe 0 first; all 0 without --ecc
    uint8_t  bits[MEISEI_NBYTES];  // the 600 frame bits, MSB first
    uint8_t  pad[1];
};
// a channel between calls (global memory)
struct SoftinMeiseiChan {
    int   mode;                    // 0 searching, 1 inside a frame
    int   done;                    // half symbols of the frame consumed (0 .. 1152), a pending odd one included
    float mv;                      // score of the header in front of the frame in progress
    float carry;                   // the pending odd half symbol (done & 1)
    unsigned long long bits_in, hdr_bit;
    float hist[MEISEI_HEADLEN];    // hdb.sbuf: the last 48 half symbols seen while searching, oldest first
    uint32_t w[MEISEI_WORDS];      // the bits of the frame in progress
    int   pad;
};
// LDS of a wave besides the staged soft decisions: 192 + 4 + 76 = 272 B
struct SoftinMeiseiLds {
    float hist[MEISEI_HEADLEN];
    float carry;
    uint32_t w[MEISEI_WORDS];
};

// ---- BCH(63,51) over GF(2^6) / 0x43, t = 2, b = 1, on a wave: what a later consumer of the same code (MRZ) can reuse
static RSW_DEV uint32_t gf64_mul(uint32_t a, const uint32_t b) {
    uint32_t r = 0;
    for (int i = 0; i < 6; i++) {
        if ((b >> i) & 1u) r ^= a;
        a <<= 1;
        if (a & 64u) a ^= 0x43u;
    }
    return r;
}
// what lane p holds for every block: alpha^p | alpha^3p << 8 for the syndromes, alpha^-p and alpha^-2p for the root search
struct Bch63Lane { uint32_t a13, b1, b2; };
static RSW_DEV Bch63Lane bch63_lane(const int lane) {
    const int p = lane % 63, m = (63 - p) % 63;
    uint32_t a = 1, b = 1;
    for (int i = 0; i < 62; i++) {
        if (i < p) { a <<= 1; if (a & 64u) a ^= 0x43u; }
        if (i < m) { b <<= 1; if (b & 64u) b ^= 0x43u; }
    }
    Bch63Lane c;
    c.a13 = a | gf64_mul(gf64_mul(a, a), a) << 8; c.b1 = b; c.b2 = gf64_mul(b, b);
    return c;
}
// One codeword on the wave: lane p < 63 holds cw[p] in `bit` (lane 63: 0).  Returns rs_decode_bch_gf2t2's result — 0, 1, 2 corrected bits, -1 fewer roots than the
// locator's degree, -2 S1 = 0 with S3 != 0 — and for a result >= 0 leaves the corrected bit in `bit` and the error positions in *errmask; the same on every lane.
static RSW_DEV int bch63_wave_decode(int &bit, unsigned long long *errmask, const Bch63Lane c, const int lane) {
    *errmask = 0;
    const uint32_t s = softin_wave_xor(bit ? c.a13 : 0u, lane), S1 = s & 63u, S3 = (s >> 8) & 63u;
    if (!s) return 0;
    if (!S1) return -2;
    // S1 L(x) = S1 + S1^2 x + (S3 + S1^3) x^2 has the roots of L(x) = 1 + S1 x + (S3 + S1^3) / S1 x^2: a root at alpha^-p is an error at p
    const uint32_t S1q = gf64_mul(S1, S1), q2 = S3 ^ gf64_mul(S1q, S1);
    const uint32_t val = S1 ^ gf64_mul(S1q, c.b1) ^ gf64_mul(q2, c.b2);
    const unsigned long long mask = rsw_ballot(lane < 63 && val == 0);
    const int n = rsw_popcll(mask);
    if (n != (q2 ? 2 : 1)) return -1;
    bit ^= (int)((mask >> lane) & 1ull);
    *errmask = mask;
    return n;
}

// The block loop of meisei100mod.c:735-776 on the 600 bits in L->w with --ecc: every block decoded, demoted to -3 where a correction landed in the padding or a word
// parity fails (cw[12] = 1 ^ XOR cw[13 .. 28], cw[29] = 1 ^ XOR cw[30 .. 45]), corrected bits written back only for a result >= 0.  Returns the 12 verdicts, block k
// in bits 4 k .. 4 k + 3 (0, 1, 2, 0xF for -3, 0xE for -1 / -2), the same on every lane.
static RSW_DEV unsigned long long meisei_wave_end(SoftinMeiseiLds *L, const int lane) {
    const Bch63Lane c = bch63_lane(lane);
    const unsigned long long m46 = (1ull << MEISEI_BLKBITS) - 1, par1 = ((1ull << 29) - 1) & ~((1ull << 12) - 1), par2 = m46 & ~((1ull << 29) - 1);
    unsigned long long be = 0;
    for (int blk = 0; blk < MEISEI_BLOCKS; blk++) {
        const int base = (blk / 6) * (MEISEI_NBITS / 2) + MEISEI_HDRBITS + MEISEI_BLKBITS * (blk % 6);
        int bit = 0;
        if (lane < MEISEI_BLKBITS) { const int i = base + (MEISEI_BLKBITS - 1) - lane; bit = (int)((L->w[i >> 5] >> (i & 31)) & 1u); }
        unsigned long long err;
        int e = bch63_wave_decode(bit, &err, c, lane);
        const unsigned long long cwm = rsw_ballot(lane < MEISEI_BLKBITS && bit);
        if (e >= 0 && ((err & ~m46) || !(rsw_popcll(cwm & par1) & 1) || !(rsw_popcll(cwm & par2) & 1))) e = -3;
        if (e > 0) {
            rsw_wave_sync();
            while (err) {                                             // (at most two, one after the other: they may share a word)
                const int p = __builtin_ctzll(err), i = base + (MEISEI_BLKBITS - 1) - p;
                err &= err - 1;
                if (lane == 0) L->w[i >> 5] ^= 1u << (i & 31);
            }
            rsw_wave_sync();
        }
        be |= (unsigned long long)(e >= 0 ? e : e == -3 ? 0xF : 0xE) << (4 * blk);
    }
    return be;
}

// One channel, one call: nb half symbols at x (sgn = -1: --softinv), ecc = --ecc.  s_x: room for stage_cap staged symbols (LDS); a call of more reads x where it
// lies.  Completed frames go to out[slot], slot from *count; a slot at or beyond cap is decoded and counted, not written.
static RSW_DEV void meisei_wave_channel(SoftinMeiseiChan *st, const float *x, const int nb, const float sgn, const int ecc, const float ths, SoftinMeiseiLds *L,
                                        float *s_x, const int stage_cap, SoftinMeiseiRec *out, unsigned *count, const int cap, const int ch, const int lane) {
    int mode = st->mode, done = st->done;
    float mv_hdr = st->mv; unsigned long long hdr_bit = st->hdr_bit; const unsigned long long bits0 = st->bits_in;
    if (mode < 0 || mode > 1 || done < 0 || done >= MEISEI_NSYM || (mode == 0 && done != 0) || nb < 0) return;                 // (never: the host zeroes the state)
    if (lane < MEISEI_HEADLEN) L->hist[lane] = st->hist[lane];
    if (lane < MEISEI_WORDS) L->w[lane] = st->w[lane];
    if (lane == 0) L->carry = st->carry;
    const SoftinX X = softin_wave_stage(s_x, x, sgn, nb, stage_cap, lane);                        // half symbol p of this call, --softinv applied
    rsw_wave_sync();
    const unsigned long long hbits = meisei_header_mask();
    int cur = 0;
    while (cur < nb) {
        if (mode == 0) {
            // element k of hist ++ the call's symbols from `cur`
            const int cur0 = cur;
            auto W = [&](const int k) -> float { return k < MEISEI_HEADLEN ? L->hist[k] : X(cur0 + (k - MEISEI_HEADLEN)); };
            bool stop = false;
            for (int base = cur0; base < nb && !stop; base += 64) {
                const int q = base + lane;
                float mv = 0.f;
                if (q < nb) mv = softin_wave_score<MEISEI_HEADLEN>(W, q - cur0 + 1, hbits, ths);   // the window of position q ends with the symbol at q
                const unsigned long long hits = rsw_ballot(q < nb && fabsf(mv) > ths);
                if (hits) {
                    // every hit counts, in either polarity: the first one starts the frame, the positions behind it are frame symbols
                    const int l = __builtin_ctzll(hits), qs = base + l;
                    const float mvl = mxxw_bcast_f(mv, l);
                    // the ring as the header leaves it: the 48 elements up to the hit (softin_wave_ring with the frame's first words in the same step)
                    const float v = W(qs - cur0 + 1 + (lane < MEISEI_HEADLEN ? lane : 0));
                    rsw_wave_sync();
                    if (lane < MEISEI_HEADLEN) L->hist[lane] = v;
                    if (lane < MEISEI_WORDS) L->w[lane] = lane == 0 ? MEISEI_HDR24 : 0u;
                    rsw_wave_sync();
                    stop = true;
                    mode = 1; done = 0; mv_hdr = mvl; hdr_bit = bits0 + (unsigned long long)qs + 1ull;
                    cur = qs + 1;
                }
            }
            if (!stop) {
                softin_wave_ring<MEISEI_HEADLEN>(L->hist, W, nb - cur0, lane);                     // the 48 elements up to the call's last symbol
                cur = nb;
            }
        } else {
            // bits from the pending half symbol of the last call and the new ones; frame symbols never enter the ring
            const int left = MEISEI_NSYM - done, take = nb - cur < left ? nb - cur : left;
            const int cn = done & 1, tot = cn + take, nbits = tot / 2, bit0 = MEISEI_HDRBITS + (done - cn) / 2;
            const int cur0 = cur;
            auto S = [&](const int k) -> float { return k < cn ? L->carry : X(cur0 + (k - cn)); };
            for (int r0 = 0; r0 < nbits; r0 += 64) {
                const int j = r0 + lane;
                bool b = false;
                if (j < nbits) b = (S(2 * j) >= 0.0f) == (S(2 * j + 1) >= 0.0f);                    // biphase-S: equal halves are a 1
                const unsigned long long m = rsw_ballot(j < nbits && b);
                // frame bit f0 + l from lane l: up to three words
                const int f0 = bit0 + r0, sh = f0 & 31, idx = (f0 >> 5) + lane;
                if (lane < 3 && idx < MEISEI_WORDS) {
                    const uint32_t v = lane == 0 ? (uint32_t)(m << sh) : lane == 1 ? (uint32_t)(m >> (32 - sh)) : sh ? (uint32_t)(m >> (64 - sh)) : 0u;
                    L->w[idx] |= v;
                }
                rsw_wave_sync();
            }
            float cv = 0.f;
            if (lane == 0 && (tot & 1)) cv = S(tot - 1);
            rsw_wave_sync();
            if (lane == 0) L->carry = cv;
            rsw_wave_sync();
            done += take; cur += take;
            if (done == MEISEI_NSYM) {
                const unsigned long long be = ecc ? meisei_wave_end(L, lane) : 0ull;
                rsw_wave_sync();
                const unsigned slot = softin_wave_slot(count, lane);
                if ((int)slot < cap && (int)slot >= 0) {
                    SoftinMeiseiRec *o = out + slot;
                    for (int k = lane; k < MEISEI_NBYTES; k += 64) {
                        const uint32_t by = (L->w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
                        uint32_t rv = 0;
                        for (int i = 0; i < 8; i++) rv |= ((by >> i) & 1u) << (7 - i);             // MSB first
                        o->bits[k] = (uint8_t)rv;
                    }
                    if (lane < MEISEI_BLOCKS) o->block_err[lane] = (uint8_t)((be >> (4 * lane)) & 0xF);
                    if (lane == 0) { o->channel = ch; o->mv = mv_hdr; o->hdr_bit = hdr_bit; o->pad[0] = 0; }
                }
                rsw_wave_sync();
                mode = 0; done = 0;                                       // the ring is still the header's 48 half symbols: the search resumes on it
            }
        }
    }
    rsw_wave_sync();
    if (lane < MEISEI_HEADLEN) st->hist[lane] = L->hist[lane];
    if (mode == 1 && lane < MEISEI_WORDS) st->w[lane] = L->w[lane];
    if (lane == 0) { st->mode = mode; st->done = done; st->mv = mv_hdr; st->carry = L->carry; st->hdr_bit = hdr_bit; st->bits_in = bits0 + (unsigned long long)nb; }
}
#endif
