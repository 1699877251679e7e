// sonde_softin_mrz_dev.h — `mp3h1mod --softin [-i] [--auto] [--ofs n]` behind the modem on ONE wavefront per channel: header search on the half-symbol stream,
// Manchester bits on a lane per bit, and at the end of a frame the bytes, the frame type and the CRC-16 on the same wave — the verdict decides how long the NEXT
// frame of the channel is, in the same call or a later one.
// Behaviour reproduced (not code): demod/mod/mp3h1mod.c main :1151-1242 (find_softbinhead on the 44 half symbols of :75 at 0.82, the polarity rule :1188-1191 with
// --auto, two half symbols per bit behind the hit, the ring left as it is), bits2bytes :157-183, crc16rev / check_CRC :280-310, the frame type and the length
// switch of print_frame :805-815; find_softbinhead / corr_softhdb are demod_mod.c:1692-1762.  The host mirror is sonde_mrz_dec_push_soft (sonde_mrz_fields.cpp).
//
//   search: a lane per stream position, softin_wave_score<44> (float first, the reference's double form wherever that is not safely below the threshold): that
//           value decides (fabs(mv) > 0.82f; 0.82f itself and the NaN of an all-zero window are no hits) and is recorded with its sign.  A hit of the other
//           polarity is dropped — the ring stays as it stands, the search goes on at the next half symbol and the later hits of the same 64 positions stay valid —
//           or with --auto flips the polarity for good and counts.  The ring is NOT emptied on a hit and is advanced only while searching.
//   frame:  a lane per bit (s = s2 - s1 of its two half symbols in one float subtraction, bit = (s >= 0), inverted unless `inv`: equal halves give +0 and a 1
//           before the polarity step), rounds of 64 bits, each round's ballot ORed into the frame's bit words in LDS behind the 22 known header bits; an odd half
//           symbol and the words so far survive a call in device memory.  The frame ends at bitfrm_len bits (408 ECEF, 384 lat / lon) from the header's first.
//   end of frame (not with -R, where the reference never looks at the bytes): byte k < (bitfrm_len - bits_ofs) / 8 on lane k from bit bits_ofs + 8 k, MSB
//           first, the bytes behind them 0; crclen = 42 if bytes 30 / 31 are FF FF, else 45.  mrz_wave_crc: CRC-16 (0xA001 reflected) is linear over GF(2), so
//           lane j < crclen carries its byte alone through the 8 (crclen - j) shifts that byte and the ones behind it take, the start value 0xFFFF folded into
//           bytes 0 and 1, and the XOR over the wave is the register: no table, no indexed array.  A good CRC sets bitfrm_len = (crclen + 6) * 8.
//
// Only COMPLETE frames are delivered: a consumer behind a live modem has no end of input.
//
// Compiled twice, like sonde_softin_meisei_dev.h: by hipcc into k_softin_mrz (sonde_softin_dev.hip) and by g++ under tests/emu/wave_emu.h
// (tests/emu/softin_mrz_emu.cpp).  Control flow around every cross-lane primitive is wave-uniform.
#ifndef SONDE_SOFTIN_MRZ_DEV_H
#define SONDE_SOFTIN_MRZ_DEV_H
#include "sonde_softin_wave_dev.h"                                     // the staged call, softin_wave_score<HL>, the ring refresh, softin_wave_xor
// (no contraction: the reference is plain C on x86-64 — every product and sum rounded on its own)
#pragma clang fp contract(off)

#define MRZ_HEADLEN   44                                              // half symbols of the header
#define MRZ_HDRBITS   22
#define MRZ_MAXBITS   408                                             // (45 + 6) * 8: the ECEF frame; the lat / lon frame has 384
#define MRZ_WORDS     13                                              // 32-bit words of the frame's bits, bit i in bit i & 31 of word i >> 5
#define MRZ_FRAME     51                                              // frame bytes (FRAME_LEN)
#define MRZ_NBYTES    52                                              // bytes of the record's bits
#define MRZ_CRCLEN_ECEF   45
#define MRZ_CRCLEN_LATLON 42
// the header mp3h1mod hands to find_softbinhead (mp3h1mod.c:75: AA AA and 101111 in Manchester), half symbol i in bit i
static RSW_DEV unsigned long long mrz_header_mask() {
    const char h[MRZ_HEADLEN + 1] = "1001" "1001" "1001" "1001" "1001" "1001" "1001" "1001" "1001" "10101010";
    unsigned long long m = 0;
    for (int i = 0; i < MRZ_HEADLEN; i++) m |= (unsigned long long)(h[i] & 1) << i;
    return m;
}
// manchester1 of that header: 10 nine times and 1111, bit i in bit i
#define MRZ_HDR22 0x3D5555u

// a completed frame as the kernel leaves it (80 bytes)
struct SoftinMrzRec {
    int32_t  channel;
    float    mv;                   // score of the header in front of the frame (the double form, rounded), with its sign
    unsigned long long hdr_bit;    // half symbols read when the header matched
    int32_t  nbits;                // 408 / 384: the frame length in effect for this frame
    uint8_t  inv;                  // polarity in effect for the frame's bits (-i, or what --auto made of it)
    uint8_t  crc_ok;               // the CRC verdict (0 with -R: never looked at)
    uint8_t  crclen;               // 42 / 45 (0 with -R)
    uint8_t  pad;
    uint16_t crcval, crcdat;       // computed and stored CRC (0 with -R)
    uint8_t  bits[MRZ_NBYTES];     // the frame bits from the header's first, MSB first; 0 behind nbits
};
// a channel between calls (global memory)
struct SoftinMrzChan {
    int   mode;                    // 0 searching, 1 inside a frame
    int   done;                    // half symbols of the frame consumed, a pending odd one included
    int   inv;                     // gpx.option.inv as it stands (--auto may flip it)
    int   bitfrm_len;              // bits of the frame in progress or the next one: 408 until a lat / lon frame passes its CRC, 384 until an ECEF one does
    float mv;                      // score of the header in front of the frame in progress
    float carry;                   // the pending odd half symbol (done & 1)
    unsigned long long bits_in, hdr_bit;
    float hist[MRZ_HEADLEN];       // hdb.sbuf: the last 44 half symbols seen while searching, oldest first
    uint32_t w[MRZ_WORDS];         // the bits of the frame in progress
    int   pad;
};
// LDS of a wave besides the staged soft decisions: 176 + 4 + 52 + 52 = 284 B
struct SoftinMrzLds {
    float hist[MRZ_HEADLEN];
    float carry;
    uint32_t w[MRZ_WORDS];
    uint8_t by[MRZ_NBYTES];
};
// what the end of a frame derives from its bits
struct MrzVerdict { int crclen, crc_ok; uint32_t crcval, crcdat; };

// CRC-16, 0xA001 reflected, start value 0xFFFF, over by[0 .. len - 1] (2 <= len <= 64) on the wave; the same on every lane.  The register is linear in (start
// value, message): the start value is the message's first two bytes XORed with FF FF, and byte j alone, stepped through its own 8 shifts and the 8 of every byte
// behind it, is its share of the register.
static RSW_DEV uint32_t mrz_wave_crc(const uint8_t *by, const int len, const int lane) {
    uint32_t rem = 0;
    if (lane < len) {
        rem = (uint32_t)by[lane] ^ (lane < 2 ? 0xFFu : 0u);
        for (int i = 0; i < 8 * (len - lane); i++) rem = (rem & 1u) ? (rem >> 1) ^ 0xA001u : rem >> 1;
    }
    return softin_wave_xor(rem, lane);
}

// print_frame's look at the nbits bits in L->w (mp3h1mod.c:799-815): L->by gets the frame bytes; the return value is the same on every lane
static RSW_DEV MrzVerdict mrz_wave_end(SoftinMrzLds *L, const int nbits, const int bits_ofs, const int lane) {
    const int frmlen = (nbits - bits_ofs) / 8;
    if (lane < MRZ_NBYTES) {
        uint32_t v = 0;
        if (lane < frmlen) for (int i = 0; i < 8; i++) { const int p = bits_ofs + 8 * lane + i; v |= ((L->w[p >> 5] >> (p & 31)) & 1u) << (7 - i); }
        L->by[lane] = (uint8_t)v;
    }
    rsw_wave_sync();
    MrzVerdict v;
    v.crclen = (L->by[30] == 0xFF && L->by[31] == 0xFF) ? MRZ_CRCLEN_LATLON : MRZ_CRCLEN_ECEF;
    v.crcval = mrz_wave_crc(L->by + 3, v.crclen, lane);
    v.crcdat = (uint32_t)L->by[v.crclen + 3] | (uint32_t)L->by[v.crclen + 4] << 8;
    v.crc_ok = v.crcval == v.crcdat ? 1 : 0;
    return v;
}

// One channel, one call: nb half symbols at x (sgn = -1: --softinv); aut = --auto, classify = 0 with -R, bits_ofs = --ofs (default 8); the polarity -i set is in
// st->inv from create on.  s_x: room for stage_cap staged symbols (LDS); a call of more reads x where it lies.  Completed frames go to out[slot], slot from
// *count; a slot at or beyond cap is decoded — its verdict still sets the next frame's length — and counted, not written.
static RSW_DEV void mrz_wave_channel(SoftinMrzChan *st, const float *x, const int nb, const float sgn, const int aut, const int classify, const int bits_ofs,
                                     const float ths, SoftinMrzLds *L, float *s_x, const int stage_cap, SoftinMrzRec *out, unsigned *count, const int cap,
                                     const int ch, const int lane) {
    int mode = st->mode, done = st->done, inv = st->inv, bitfrm_len = st->bitfrm_len;
    float mv_hdr = st->mv; unsigned long long hdr_bit = st->hdr_bit; const unsigned long long bits0 = st->bits_in;
    if (mode < 0 || mode > 1 || inv < 0 || inv > 1 || (bitfrm_len != MRZ_MAXBITS && bitfrm_len != (MRZ_CRCLEN_LATLON + 6) * 8) || done < 0
        || done >= 2 * (bitfrm_len - MRZ_HDRBITS) || (mode == 0 && done != 0) || bits_ofs < 0 || bits_ofs > 64 || nb < 0) return;       // (never: the host sets the state)
    if (lane < MRZ_HEADLEN) L->hist[lane] = st->hist[lane];
    if (lane < MRZ_WORDS) L->w[lane] = st->w[lane];
    if (lane == 0) L->carry = st->carry;
    const SoftinX X = softin_wave_stage(s_x, x, sgn, nb, stage_cap, lane);                        // half symbol p of this call, --softinv applied
    rsw_wave_sync();
    const unsigned long long hbits = mrz_header_mask();
    int cur = 0;
    while (cur < nb) {
        if (mode == 0) {
            // element k of hist ++ the call's symbols from `cur`
            const int cur0 = cur;
            auto W = [&](const int k) -> float { return k < MRZ_HEADLEN ? L->hist[k] : X(cur0 + (k - MRZ_HEADLEN)); };
            bool stop = false;
            for (int base = cur0; base < nb && !stop; base += 64) {
                const int q = base + lane;
                float mv = 0.f;
                if (q < nb) mv = softin_wave_score<MRZ_HEADLEN>(W, q - cur0 + 1, hbits, ths);      // the window of position q ends with the symbol at q
                unsigned long long hits = rsw_ballot(q < nb && fabsf(mv) > ths);
                while (hits && !stop) {
                    const int l = __builtin_ctzll(hits), qs = base + l;
                    hits &= hits - 1;
                    const float mvl = mxxw_bcast_f(mv, l);
                    // a header of the other polarity (:1188-1191): dropped — the ring stays, so the hits behind it in this round are what the reference sees —
                    // or with --auto the option flips and the hit counts
                    if ((double)mvl * (0.5 - inv) < 0) { if (!aut) continue; inv ^= 1; }
                    // the ring as the header leaves it: the 44 elements up to the hit (softin_wave_ring with the frame's first words in the same step)
                    const float v = W(qs - cur0 + 1 + (lane < MRZ_HEADLEN ? lane : 0));
                    rsw_wave_sync();
                    if (lane < MRZ_HEADLEN) L->hist[lane] = v;
                    if (lane < MRZ_WORDS) L->w[lane] = lane == 0 ? MRZ_HDR22 : 0u;
                    rsw_wave_sync();
                    stop = true;
                    mode = 1; done = 0; mv_hdr = mvl; hdr_bit = bits0 + (unsigned long long)qs + 1ull;
                    cur = qs + 1;
                }
            }
            if (!stop) {
                softin_wave_ring<MRZ_HEADLEN>(L->hist, W, nb - cur0, lane);                        // the 44 elements up to the call's last symbol
                cur = nb;
            }
        } else {
            // bits from the pending half symbol of the last call and the new ones; frame symbols never enter the ring
            const int nsym = 2 * (bitfrm_len - MRZ_HDRBITS);
            const int left = nsym - done, take = nb - cur < left ? nb - cur : left;
            const int cn = done & 1, tot = cn + take, nbits = tot / 2, bit0 = MRZ_HDRBITS + (done - cn) / 2;
            const int cur0 = cur;
            auto S = [&](const int k) -> float { return k < cn ? L->carry : X(cur0 + (k - cn)); };
            for (int r0 = 0; r0 < nbits; r0 += 64) {
                const int j = r0 + lane;
                bool b = false;
                if (j < nbits) {
                    const float s = S(2 * j + 1) - S(2 * j);                                     // both half symbols of a bit (:1205-1211)
                    b = (s >= 0.0f) != (inv == 0);                                               // Manchester1 unless inverted (:1227-1233)
                }
                const unsigned long long m = rsw_ballot(j < nbits && b);
                // frame bit f0 + l from lane l: up to three words
                const int f0 = bit0 + r0, sh = f0 & 31, idx = (f0 >> 5) + lane;
                if (lane < 3 && idx < MRZ_WORDS) {
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
            if (done == nsym) {
                MrzVerdict v; v.crclen = 0; v.crc_ok = 0; v.crcval = 0; v.crcdat = 0;
                if (classify) v = mrz_wave_end(L, bitfrm_len, bits_ofs, lane);
                rsw_wave_sync();
                const unsigned slot = softin_wave_slot(count, lane);
                if ((int)slot < cap && (int)slot >= 0) {
                    SoftinMrzRec *o = out + slot;
                    if (lane < MRZ_NBYTES) {
                        const uint32_t by = (L->w[lane >> 2] >> (8 * (lane & 3))) & 0xFFu;
                        uint32_t rv = 0;
                        for (int i = 0; i < 8; i++) rv |= ((by >> i) & 1u) << (7 - i);             // MSB first
                        o->bits[lane] = (uint8_t)rv;
                    }
                    if (lane == 0) {
                        o->channel = ch; o->mv = mv_hdr; o->hdr_bit = hdr_bit; o->nbits = bitfrm_len; o->inv = (uint8_t)inv; o->crc_ok = (uint8_t)v.crc_ok;
                        o->crclen = (uint8_t)v.crclen; o->pad = 0; o->crcval = (uint16_t)v.crcval; o->crcdat = (uint16_t)v.crcdat;
                    }
                }
                rsw_wave_sync();
                if (v.crc_ok) bitfrm_len = (v.crclen + 6) * 8;                // the next frame's length (:812-814), delivered or not
                mode = 0; done = 0;                                           // the ring is still the header's 44 half symbols: the search resumes on it
            }
        }
    }
    rsw_wave_sync();
    if (lane < MRZ_HEADLEN) st->hist[lane] = L->hist[lane];
    if (mode == 1 && lane < MRZ_WORDS) st->w[lane] = L->w[lane];
    if (lane == 0) {
        st->mode = mode; st->done = done; st->inv = inv; st->bitfrm_len = bitfrm_len; st->mv = mv_hdr; st->carry = L->carry; st->hdr_bit = hdr_bit;
        st->bits_in = bits0 + (unsigned long long)nb;
    }
}
#endif
