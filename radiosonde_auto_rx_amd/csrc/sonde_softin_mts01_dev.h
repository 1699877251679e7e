// sonde_softin_mts01_dev.h — `mts01mod --softin` behind the modem on ONE wavefront per channel: header search on the symbol stream, bits on a lane per bit, and at
// the end of a frame the 131 bytes and the CRC-16 on the same wave.
// Behaviour reproduced (not code): demod/mod/mts01mod.c main :543-618 (find_softbinhead on the 32 header symbols AA AA B4 2B at 0.8 in EITHER polarity, 1048
// symbols behind the hit read raw, the ring left as it is), crc16_re :76-99, bits2bytes :101-127, the CRC compare of print_frame :151-162; find_softbinhead /
// corr_softhdb are demod_mod.c:1692-1762.  The host mirror is sonde_mts01_dec_push_soft (sonde_mts01_fields.cpp).
//
//   search: a lane per stream position, softin_wave_score<32> (float first, the reference's double form wherever that is not safely below the threshold): that
//           value decides (fabs(mv) > 0.8f in either polarity; 0.8f itself and the NaN of an all-zero window are no hits) and is recorded with its sign.  Every
//           hit counts; the reference flips an option nothing reads, so the bits of an inverted stream come out inverted and the CRC fails (--softinv puts it
//           right).  The ring is NOT emptied on a hit and is advanced only while searching.
//   frame:  a lane per bit (bit = (s >= 0), so -0.0 is a 1), 1048 bits in rounds of 64, each round's ballot ORed into the frame's bit words in LDS.
//   end of frame: byte k of 131 on lane k (three rounds), MSB first.  mts01_wave_crc: CRC-16 (0x8005, MSB first) is linear over GF(2), so lane j carries bytes
//           1 + 2 j and 2 + 2 j alone through their own 16 shifts and the 16 of every pair behind them, the start value 0xFFFF folded into bytes 1 and 2, and the
//           XOR over the wave is the register; bit-reversed it is compared with bytes[130] << 8 | bytes[129].  No table, no indexed array.
//
// Only COMPLETE frames are delivered: a consumer behind a live modem has no end of input.
//
// Compiled twice, like sonde_softin_meisei_dev.h: by hipcc into k_softin_mts01 (sonde_softin_dev.hip) and by g++ under tests/emu/wave_emu.h
// (tests/emu/softin_mts01_emu.cpp).  Control flow around every cross-lane primitive is wave-uniform.
#ifndef SONDE_SOFTIN_MTS01_DEV_H
#define SONDE_SOFTIN_MTS01_DEV_H
#include "sonde_softin_wave_dev.h"                                     // the staged call, softin_wave_score<HL>, the ring refresh, softin_wave_xor
// (no contraction: the reference is plain C on x86-64 — every product and sum rounded on its own)
#pragma clang fp contract(off)

#define MTS01_HEADLEN  32                                             // symbols of the header
#define MTS01_NBITS    1048                                           // symbols = bits behind the header: 8 * (130 + 1)
#define MTS01_WORDS    33                                             // 32-bit words of the frame's bits, bit i in bit i & 31 of word i >> 5
#define MTS01_NBYTES   131
#define MTS01_DATLEN   128                                            // bytes under the CRC, from byte 1
// the header mts01mod hands to find_softbinhead (mts01mod.c:60: AA AA B4 2B), symbol i in bit i
static RSW_DEV unsigned long long mts01_header_mask() {
    const char h[MTS01_HEADLEN + 1] = "10101010" "10101010" "10110100" "00101011";
    unsigned long long m = 0;
    for (int i = 0; i < MTS01_HEADLEN; i++) m |= (unsigned long long)(h[i] & 1) << i;
    return m;
}

// a completed frame as the kernel leaves it (152 bytes)
struct SoftinMts01Rec {
    int32_t  channel;
    float    mv;                   // score of the header in front of the frame (the double form, rounded), with its sign
    unsigned long long hdr_bit;    // symbols read when the header matched
    uint16_t crcval, crcdat;       // computed (bit-reversed) and stored CRC
    uint8_t  crc_ok;
    uint8_t  bytes[MTS01_NBYTES];  // the 1048 frame bits, MSB first
};
// a channel between calls (global memory)
struct SoftinMts01Chan {
    int   mode;                    // 0 searching, 1 inside a frame
    int   done;                    // symbols of the frame consumed (0 .. 1047)
    float mv;                      // score of the header in front of the frame in progress
    int   pad;
    unsigned long long bits_in, hdr_bit;
    float hist[MTS01_HEADLEN];     // hdb.sbuf: the last 32 symbols seen while searching, oldest first
    uint32_t w[MTS01_WORDS];       // the bits of the frame in progress
    int   pad2;
};
// LDS of a wave besides the staged soft decisions: 128 + 132 + 132 = 392 B
struct SoftinMts01Lds {
    float hist[MTS01_HEADLEN];
    uint32_t w[MTS01_WORDS];
    uint8_t by[MTS01_NBYTES + 1];
};
struct Mts01Verdict { uint32_t crcval, crcdat; int crc_ok; };

// crc16_re over by[0 .. 127] on the wave: CRC-16, 0x8005, MSB first, start value 0xFFFF, the result bit-reversed; the same on every lane.  The register is linear in
// (start value, message): the start value is the message's first two bytes XORed with FF FF, and a byte pair alone, stepped through its own 16 shifts and the 16 of
// every pair behind it, is its share of the register.
static RSW_DEV uint32_t mts01_wave_crc(const uint8_t *by, const int lane) {
    const uint32_t fold = lane == 0 ? 0xFFu : 0u;
    uint32_t rem = ((uint32_t)by[2 * lane] ^ fold) << 8;
    for (int i = 0; i < 8; i++) rem = ((rem & 0x8000u) ? (rem << 1) ^ 0x8005u : rem << 1) & 0xFFFFu;
    rem ^= ((uint32_t)by[2 * lane + 1] ^ fold) << 8;
    for (int i = 0; i < 8 + 16 * (63 - lane); i++) rem = ((rem & 0x8000u) ? (rem << 1) ^ 0x8005u : rem << 1) & 0xFFFFu;
    rem = softin_wave_xor(rem, lane);
    uint32_t re = 0;
    for (int j = 0; j < 16; j++) re |= ((rem >> (15 - j)) & 1u) << j;
    return re;
}

// print_frame's look at the 1048 bits in L->w (mts01mod.c:151-162): L->by gets the 131 bytes; the return value is the same on every lane
static RSW_DEV Mts01Verdict mts01_wave_end(SoftinMts01Lds *L, const int lane) {
    for (int k = lane; k < MTS01_NBYTES + 1; k += 64) {
        uint32_t rv = 0;
        if (k < MTS01_NBYTES) {
            const uint32_t by = (L->w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
            for (int i = 0; i < 8; i++) rv |= ((by >> i) & 1u) << (7 - i);                         // MSB first
        }
        L->by[k] = (uint8_t)rv;
    }
    rsw_wave_sync();
    Mts01Verdict v;
    v.crcval = mts01_wave_crc(L->by + 1, lane);
    v.crcdat = (uint32_t)L->by[1 + MTS01_DATLEN + 1] << 8 | (uint32_t)L->by[1 + MTS01_DATLEN];
    v.crc_ok = v.crcval == v.crcdat ? 1 : 0;
    return v;
}

// One channel, one call: nb symbols at x (sgn = -1: --softinv).  s_x: room for stage_cap staged symbols (LDS); a call of more reads x where it lies.  Completed
// frames go to out[slot], slot from *count; a slot at or beyond cap is decoded and counted, not written.
static RSW_DEV void mts01_wave_channel(SoftinMts01Chan *st, const float *x, const int nb, const float sgn, const float ths, SoftinMts01Lds *L, float *s_x,
                                       const int stage_cap, SoftinMts01Rec *out, unsigned *count, const int cap, const int ch, const int lane) {
    int mode = st->mode, done = st->done;
    float mv_hdr = st->mv; unsigned long long hdr_bit = st->hdr_bit; const unsigned long long bits0 = st->bits_in;
    if (mode < 0 || mode > 1 || done < 0 || done >= MTS01_NBITS || (mode == 0 && done != 0) || nb < 0) return;                 // (never: the host zeroes the state)
    if (lane < MTS01_HEADLEN) L->hist[lane] = st->hist[lane];
    if (lane < MTS01_WORDS) L->w[lane] = st->w[lane];
    const SoftinX X = softin_wave_stage(s_x, x, sgn, nb, stage_cap, lane);                        // symbol p of this call, --softinv applied
    rsw_wave_sync();
    const unsigned long long hbits = mts01_header_mask();
    int cur = 0;
    while (cur < nb) {
        if (mode == 0) {
            // element k of hist ++ the call's symbols from `cur`
            const int cur0 = cur;
            auto W = [&](const int k) -> float { return k < MTS01_HEADLEN ? L->hist[k] : X(cur0 + (k - MTS01_HEADLEN)); };
            bool stop = false;
            for (int base = cur0; base < nb && !stop; base += 64) {
                const int q = base + lane;
                float mv = 0.f;
                if (q < nb) mv = softin_wave_score<MTS01_HEADLEN>(W, q - cur0 + 1, hbits, ths);    // the window of position q ends with the symbol at q
                const unsigned long long hits = rsw_ballot(q < nb && fabsf(mv) > ths);
                if (hits) {
                    // every hit counts, in either polarity: the first one starts the frame, the positions behind it are frame symbols
                    const int l = __builtin_ctzll(hits), qs = base + l;
                    const float mvl = mxxw_bcast_f(mv, l);
                    // the ring as the header leaves it: the 32 elements up to the hit (softin_wave_ring with the frame's words in the same step)
                    const float v = W(qs - cur0 + 1 + (lane < MTS01_HEADLEN ? lane : 0));
                    rsw_wave_sync();
                    if (lane < MTS01_HEADLEN) L->hist[lane] = v;
                    if (lane < MTS01_WORDS) L->w[lane] = 0u;
                    rsw_wave_sync();
                    stop = true;
                    mode = 1; done = 0; mv_hdr = mvl; hdr_bit = bits0 + (unsigned long long)qs + 1ull;
                    cur = qs + 1;
                }
            }
            if (!stop) {
                softin_wave_ring<MTS01_HEADLEN>(L->hist, W, nb - cur0, lane);                      // the 32 elements up to the call's last symbol
                cur = nb;
            }
        } else {
            // a bit per symbol, read raw (:604); frame symbols never enter the ring
            const int left = MTS01_NBITS - done, take = nb - cur < left ? nb - cur : left;
            const int cur0 = cur;
            for (int r0 = 0; r0 < take; r0 += 64) {
                const int j = r0 + lane;
                const unsigned long long m = rsw_ballot(j < take && X(cur0 + (j < take ? j : 0)) >= 0.0f);
                // frame bit f0 + l from lane l: up to three words
                const int f0 = done + r0, sh = f0 & 31, idx = (f0 >> 5) + lane;
                if (lane < 3 && idx < MTS01_WORDS) {
                    const uint32_t v = lane == 0 ? (uint32_t)(m << sh) : lane == 1 ? (uint32_t)(m >> (32 - sh)) : sh ? (uint32_t)(m >> (64 - sh)) : 0u;
                    L->w[idx] |= v;
                }
                rsw_wave_sync();
            }
            done += take; cur += take;
            if (done == MTS01_NBITS) {
                const Mts01Verdict v = mts01_wave_end(L, lane);
                const unsigned slot = softin_wave_slot(count, lane);
                if ((int)slot < cap && (int)slot >= 0) {
                    SoftinMts01Rec *o = out + slot;
                    for (int k = lane; k < MTS01_NBYTES; k += 64) o->bytes[k] = L->by[k];
                    if (lane == 0) { o->channel = ch; o->mv = mv_hdr; o->hdr_bit = hdr_bit; o->crcval = (uint16_t)v.crcval; o->crcdat = (uint16_t)v.crcdat; o->crc_ok = (uint8_t)v.crc_ok; }
                }
                rsw_wave_sync();
                mode = 0; done = 0;                                       // the ring is still the header's 32 symbols: the search resumes on it
            }
        }
    }
    rsw_wave_sync();
    if (lane < MTS01_HEADLEN) st->hist[lane] = L->hist[lane];
    if (mode == 1 && lane < MTS01_WORDS) st->w[lane] = L->w[lane];
    if (lane == 0) { st->mode = mode; st->done = done; st->mv = mv_hdr; st->hdr_bit = hdr_bit; st->bits_in = bits0 + (unsigned long long)nb; }
}
#endif
