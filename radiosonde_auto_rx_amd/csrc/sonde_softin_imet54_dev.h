// sonde_softin_imet54_dev.h — `imet54mod --softin [-i] [--auto] [--ecc]` behind the modem on ONE wavefront per channel: header search on the symbol stream, 8N1
// characters on a lane per character, and at the end of a frame the de-interleave, Hamming(8,4) on a lane per codeword and both check sums on the same wave.
// Behaviour reproduced (not code): demod/mod/imet54mod.c main :1007-1063 (find_softbinhead on the 40 header symbols of :95 at 0.8, the polarity rule :1018-1022 with
// --auto, 2200 symbols behind the hit, the ring left as it is), de8n1 :107-118, deinter64 :120-133, check / hamming :162-227, crc32ok :229-284, crc32_802 :286-303,
// crc32ok_cont :350-360, the ecc sums of print_frame :618-660; find_softbinhead / corr_softhdb are demod_mod.c:1692-1762.  The host mirror is
// sonde_imet54_dec_push_soft (sonde_imet54_fields.cpp).
//
//   search: a lane per stream position; the normalised correlation in float first, and every position that is not safely below the threshold again the
//           reference's way (float products, double sums in order, sum / sqrt(normx * 40.0), rounded to float): that value decides (fabs(mv) > 0.8f; 0.8f itself
//           and the NaN of an all-zero window are no hits) and is recorded.  The ring is NOT emptied on a hit and is advanced only while searching: behind a frame
//           the search resumes on the 40 symbols the accepted header left, behind a dropped hit (the other polarity without --auto) on the ring as it stands, and
//           the later hits of the same 64 positions stay valid.
//   frame:  a lane per character (10 symbols, bit = (s >= 0) ^ inv, data bit k in bit k, start and stop bit not looked at); the symbols of an unfinished
//           character and the characters of the frame in progress survive a call in device memory.
//   end of frame (220 characters = 2200 symbols behind the hit): codeword j = 8 b + r takes bit i from data bit r of character 3 + 8 b + i (de8n1, the 24-bit
//           offset and the 8 x 8 transpose in one gather; the 220th character belongs to no block), four rounds of 64 codewords; frame byte j from nibbles 2 j and
//           2 j + 1; ecc_frm / ecc_tlm / ecc_std from two ballots; both check sums as XOR sums of per-(byte, bit) contribution words (imet54_crc_table, built by
//           the host from the serial recurrences) reduced over the wave.
//
// Only COMPLETE frames are delivered: the reference prints a partial frame only at end of input (:1065), and a consumer behind a live modem has no end of input.
//
// Compiled twice, like sonde_softin_mxx_dev.h: by hipcc into k_softin_imet54 (sonde_softin_dev.hip) and by g++ under tests/emu/wave_emu.h
// (tests/emu/softin_imet54_emu.cpp).  Control flow around every cross-lane primitive is wave-uniform.
#ifndef SONDE_SOFTIN_IMET54_DEV_H
#define SONDE_SOFTIN_IMET54_DEV_H
#include "sonde_softin_wave_dev.h"                                     // the staged call, softin_wave_score<HL>, the ring refresh, softin_wave_8n1 / _xor
// (no contraction: the reference is plain C on x86-64 — every product and sum rounded on its own)
#pragma clang fp contract(off)

#define IMET54_HEADLEN  40
#define IMET54_CHARS    220
#define IMET54_CHARSYM  10                                            // symbols of an 8N1 character
#define IMET54_NSYM     (IMET54_CHARS * IMET54_CHARSYM)               // 2200 symbols behind the header
#define IMET54_NCW      216                                           // Hamming codewords of a frame: 27 blocks of 8
#define IMET54_FRAME    108
#define IMET54_TAB_N    (IMET54_FRAME * 8 * 3)                        // contribution words: (byte, bit) -> crc0, crc1 of the standard check, the CRC-32 of the continuous one
// the header imet54mod hands to find_softbinhead (imet54mod.c:95: 00 AA 24 24 as 8N1 characters), symbol i in bit i
static RSW_DEV unsigned long long imet54_header_mask() {
    const char h[IMET54_HEADLEN + 1] = "0000000001" "0101010101" "0001001001" "0001001001";
    unsigned long long m = 0;
    for (int i = 0; i < IMET54_HEADLEN; i++) m |= (unsigned long long)(h[i] & 1) << i;
    return m;
}

// a completed frame as the kernel leaves it
struct SoftinImet54Rec {
    int32_t  channel;
    float    mv;                   // score of the header in front of the frame (the double form, rounded)
    unsigned long long hdr_bit;    // symbols read when the header matched
    int32_t  inv;                  // polarity in effect for the frame's bits (-i, or what --auto made of it)
    int32_t  ecc_frm, ecc_tlm, ecc_std;
    int32_t  crc_std, crc_cont;    // crc32ok over the 108 bytes, crc32ok_cont over the first 52 + 4
    uint8_t  frame[IMET54_FRAME];
    uint8_t  pad[4];
};
// a channel between calls (global memory)
struct SoftinImet54Chan {
    int   mode;                    // 0 searching, 1 inside a frame
    int   inv;                     // gpx.option.inv as it stands (--auto may flip it)
    int   done;                    // symbols of the frame consumed (0 .. 2200), the pending ones included
    int   carry_n;                 // symbols of an unfinished character
    float mv;                      // score of the header in front of the frame in progress
    int   pad;
    unsigned long long bits_in, hdr_bit;
    float carry[IMET54_CHARSYM];
    float hist[IMET54_HEADLEN];    // hdb.sbuf: the last 40 symbols seen while searching, oldest first
    uint8_t chr[IMET54_CHARS];     // the characters of the frame in progress
};
// LDS of a wave besides the staged soft decisions: 160 + 40 + 224 + 216 + 108 = 748 B
struct SoftinImet54Lds {
    float hist[IMET54_HEADLEN];
    float carry[IMET54_CHARSYM];
    uint8_t chr[IMET54_CHARS + 4];
    uint8_t nib[IMET54_NCW];
    uint8_t fr[IMET54_FRAME];
};
// what the end of a frame derives from its characters
struct Imet54Verdict { int ecc_frm, ecc_tlm, ecc_std, crc_std, crc_cont; };

// ---- host side (plain C++: hipcc compiles it for the host, g++ for the emulator): the contribution words of both check sums.
// crc32ok (imet54mod.c:229-284) steps two registers through a sequence that does not depend on the data and XORs them into the sums wherever a data bit is set; the
// stored words at 100 / 101 and 106 / 107 are XORed in afterwards: every bit of the 108 bytes has a fixed word pair.  crc32ok_cont (:350-360) is CRC-32 with a zero
// start value over bytes 0 .. 51 in groups of four taken backwards, compared with the big-endian word at 52: linear as well, the stored word's bits standing for
// themselves.  t[3 * (8 * n + b) + 0 / 1 / 2] = crc0 / crc1 / CRC-32 word of bit b of byte n.  The verdicts (imet54_wave_end): (crc1 sum ^ 0x1DAD) == 0 and
// ((crc0 sum ^ 0x5000) & 0xF000) == 0; CRC-32 sum == 0x63D60875.
static inline void imet54_crc_table(uint32_t *t) {
    for (int i = 0; i < IMET54_TAB_N; i++) t[i] = 0;
    int n = 104, b = 0;
    uint32_t c0 = 0x48EB, c1 = 0x1ACA, nx_c0 = c0, nx_c1 = c1;
    while (n >= 0) {
        if (n < 100 || (n > 101 && n < 106)) { t[3 * (8 * n + b)] = c0; t[3 * (8 * n + b) + 1] = c1; }
        if (c1 & 0x8000) { nx_c0 ^= 0x0EDB; nx_c1 ^= 0x8260; }
        nx_c0 <<= 1; nx_c1 <<= 1;
        if (c1 & 0x8000) nx_c0 |= 1;
        if ((c1 ^ c0) & 0x8000) nx_c1 |= 1;
        nx_c0 &= 0xFFFF;
        c0 = nx_c0; c1 = nx_c1;
        if (b < 7) b += 1;
        else { b = 0; if (n % 4 == 3) n -= 7; else n += 1; }
    }
    for (int k = 0; k < 8; k++) {                                     // the stored words, big endian
        t[3 * (8 * 100 + k)] = 1u << (8 + k); t[3 * (8 * 101 + k)] = 1u << k;
        t[3 * (8 * 106 + k) + 1] = 1u << (8 + k); t[3 * (8 * 107 + k) + 1] = 1u << k;
    }
    for (int p = 0; p < 52; p++) {                                    // message position p holds frame byte 4 (p / 4) + 3 - p % 4
        const int nb = 4 * (p / 4) + 3 - p % 4;
        for (int k = 0; k < 8; k++) {
            uint32_t rem = (uint32_t)(1u << k) << 24;
            for (int i = 0; i < 8 * (52 - p); i++) rem = (rem & 0x80000000u) ? (rem << 1) ^ 0x04C11DB7u : rem << 1;
            t[3 * (8 * nb + k) + 2] = rem;
        }
    }
    for (int k = 0; k < 8; k++) for (int j = 0; j < 4; j++) t[3 * (8 * (52 + j) + k) + 2] = 1u << (8 * (3 - j) + k);
}

// print_frame's work on the 220 characters in L->chr (imet54mod.c:626-660): L->fr gets the 108 frame bytes, the return value is the same on every lane.
// tab: imet54_crc_table's words (global memory).
static RSW_DEV Imet54Verdict imet54_wave_end(SoftinImet54Lds *L, const int ecc, const uint32_t *tab, const int lane) {
    // ham_lut (:196-197), nibble n in byte n
    const unsigned long long lut_lo = 0xB4332DAA1E998700ull, lut_hi = 0xFF7866E155D2CC4Bull;
    unsigned long long bad0 = 0, bad1 = 0, fix0 = 0, fix1 = 0;
    for (int round = 0; round < 4; round++) {
        const int j = 64 * round + lane;
        int ec = 0;
        if (j < IMET54_NCW) {
            const int b = j >> 3, r = j & 7;
            unsigned cw = 0;
            for (int i = 0; i < 8; i++) cw |= (unsigned)((L->chr[3 + 8 * b + i] >> r) & 1) << i;
            int e = 0;
            if (ecc) {
                // the four parity rows H (:166-169) as masks over the codeword's bits
                const unsigned syn = (unsigned)(__builtin_popcount(cw & 0x55) & 1) | (unsigned)(__builtin_popcount(cw & 0x66) & 1) << 1
                                   | (unsigned)(__builtin_popcount(cw & 0x78) & 1) << 2 | (unsigned)(__builtin_popcount(cw & 0xFF) & 1) << 3;
                // He (:170-171): 0x9 .. 0xF name bits 0 .. 6, 0x8 bit 7; 1 .. 7 name none
                if (syn) { e = syn >= 9 ? (int)syn - 8 : syn == 8 ? 8 : -1; if (e > 0) cw ^= 1u << (e - 1); }
            }
            int nib = 16;
            for (int n = 0; n < 16; n++) if (((n < 8 ? lut_lo >> (8 * n) : lut_hi >> (8 * (n - 8))) & 0xFF) == cw) nib = n;
            ec = (e < 0 || nib >= 16) ? 0xF0 : e > 0 ? 1 : 0;
            L->nib[j] = (uint8_t)nib;
        }
        const unsigned long long bad = rsw_ballot(j < IMET54_NCW && ec == 0xF0), fix = rsw_ballot(j < IMET54_NCW && ec == 1);
        if (round == 0) { bad0 = bad; fix0 = fix; }
        if (round == 1) { bad1 = bad; fix1 = fix; }
    }
    rsw_wave_sync();
    // frame byte j from nibbles 2 j and 2 j + 1; a nibble of 16 (no table entry) leaves its half 0, as (16 << 4) | (16 & 0xF) truncates
    for (int j = lane; j < IMET54_FRAME; j += 64) L->fr[j] = (uint8_t)((L->nib[2 * j] << 4) | (L->nib[2 * j + 1] & 0xF));
    rsw_wave_sync();
    Imet54Verdict v;
    // the sums over the first 104 codewords (:651-659): ecc_tlm stops at 88 = 2 * (0x2A + 2), -1 and stop at the first 0xF0, ecc_std = -1 after a stop
    const unsigned long long m88 = (1ull << (88 - 64)) - 1, m104 = (1ull << (104 - 64)) - 1;
    const int tlm = rsw_popcll(fix0) + rsw_popcll(fix1 & m88);
    if (bad0 | (bad1 & m104)) {
        const int first = bad0 ? __builtin_ctzll(bad0) : 64 + __builtin_ctzll(bad1 & m104);
        v.ecc_frm = -1; v.ecc_std = -1; v.ecc_tlm = first < 88 ? -1 : tlm;
    } else {
        v.ecc_frm = rsw_popcll(fix0) + rsw_popcll(fix1 & m104); v.ecc_tlm = tlm; v.ecc_std = v.ecc_frm;
    }
    // both check sums: every lane the words of its bytes' set bits, then the XOR over the wave
    uint32_t w0 = 0, w1 = 0, w2 = 0;
    for (int j = lane; j < IMET54_FRAME; j += 64) {
        const unsigned by = L->fr[j];
        for (int k = 0; k < 8; k++) if ((by >> k) & 1u) { const uint32_t *t = tab + 3 * (8 * j + k); w0 ^= t[0]; w1 ^= t[1]; w2 ^= t[2]; }
    }
    w0 = softin_wave_xor(w0, lane); w1 = softin_wave_xor(w1, lane); w2 = softin_wave_xor(w2, lane);
    v.crc_std = ((w1 ^ 0x1DADu) == 0 && ((w0 ^ 0x5000u) & 0xF000u) == 0) ? 1 : 0;
    v.crc_cont = w2 == 0x63D60875u ? 1 : 0;
    return v;
}

// One channel, one call: nb symbols at x (sgn = -1: --softinv); aut = --auto, ecc = --ecc; the polarity -i set is in st->inv from create on.  s_x: room for
// stage_cap staged symbols (LDS); a call of more reads x where it lies.  Completed frames go to out[slot], slot from *count; a slot at or beyond cap is decoded and
// counted, not written.
static RSW_DEV void imet54_wave_channel(SoftinImet54Chan *st, const float *x, const int nb, const float sgn, const int aut, const int ecc, const float ths,
                                        const uint32_t *tab, SoftinImet54Lds *L, float *s_x, const int stage_cap, SoftinImet54Rec *out, unsigned *count, const int cap,
                                        const int ch, const int lane) {
    int mode = st->mode, inv = st->inv, done = st->done, carry_n = st->carry_n;
    float mv_hdr = st->mv; unsigned long long hdr_bit = st->hdr_bit; const unsigned long long bits0 = st->bits_in;
    if (mode < 0 || mode > 1 || inv < 0 || inv > 1 || done < 0 || done > IMET54_NSYM || carry_n < 0 || carry_n >= IMET54_CHARSYM || carry_n > done
        || (done - carry_n) % IMET54_CHARSYM != 0 || nb < 0) return;                                                       // (never: the host zeroes the state)
    if (lane < IMET54_HEADLEN) L->hist[lane] = st->hist[lane];
    if (lane < IMET54_CHARSYM) L->carry[lane] = st->carry[lane];
    for (int i = lane; i < IMET54_CHARS; i += 64) L->chr[i] = st->chr[i];
    const SoftinX X = softin_wave_stage(s_x, x, sgn, nb, stage_cap, lane);                        // symbol p of this call, --softinv applied
    rsw_wave_sync();
    const unsigned long long hbits = imet54_header_mask();
    int cur = 0;
    while (cur < nb) {
        if (mode == 0) {
            // element k of hist ++ the call's symbols from `cur`
            const int cur0 = cur;
            auto W = [&](const int k) -> float { return k < IMET54_HEADLEN ? L->hist[k] : X(cur0 + (k - IMET54_HEADLEN)); };
            bool stop = false;
            for (int base = cur0; base < nb && !stop; base += 64) {
                const int q = base + lane;
                float mv = 0.f;
                if (q < nb) mv = softin_wave_score<IMET54_HEADLEN>(W, q - cur0 + 1, hbits, ths);   // the window of position q ends with the symbol at q
                unsigned long long hits = rsw_ballot(q < nb && fabsf(mv) > ths);
                while (hits && !stop) {
                    const int l = __builtin_ctzll(hits), qs = base + l;
                    hits &= hits - 1;
                    const float mvl = mxxw_bcast_f(mv, l);
                    // a header of the other polarity (:1018-1022): dropped — the ring stays, so the hits behind it in this round are what the reference sees —
                    // or with --auto the option flips and the hit counts
                    if ((double)mvl * (0.5 - inv) < 0) { if (!aut) continue; inv ^= 1; }
                    softin_wave_ring<IMET54_HEADLEN>(L->hist, W, qs - cur0 + 1, lane);             // the ring as the header leaves it: the 40 elements up to the hit
                    stop = true;
                    mode = 1; done = 0; carry_n = 0; mv_hdr = mvl; hdr_bit = bits0 + (unsigned long long)qs + 1ull;
                    cur = qs + 1;
                }
            }
            if (!stop) {
                softin_wave_ring<IMET54_HEADLEN>(L->hist, W, nb - cur0, lane);                     // the 40 elements up to the call's last symbol
                cur = nb;
            }
        } else {
            // characters from the pending symbols of the last call and the new ones; frame symbols never enter the ring
            const int left = IMET54_NSYM - done, take = nb - cur < left ? nb - cur : left;
            const int tot = carry_n + take, nchars = tot / IMET54_CHARSYM, chr0 = (done - carry_n) / IMET54_CHARSYM;
            const int cur0 = cur, cn = carry_n;
            auto S = [&](const int k) -> float { return k < cn ? L->carry[k] : X(cur0 + (k - cn)); };
            softin_wave_8n1(S, nchars, inv, L->chr + chr0, lane);
            const int rest = tot - IMET54_CHARSYM * nchars;
            float cv = 0.f;
            if (lane < rest) cv = S(IMET54_CHARSYM * nchars + lane);
            rsw_wave_sync();
            if (lane < IMET54_CHARSYM) L->carry[lane] = cv;
            rsw_wave_sync();
            carry_n = rest; done += take; cur += take;
            if (done == IMET54_NSYM) {
                const Imet54Verdict v = imet54_wave_end(L, ecc, tab, lane);
                const unsigned slot = softin_wave_slot(count, lane);
                if ((int)slot < cap && (int)slot >= 0) {
                    SoftinImet54Rec *o = out + slot;
                    for (int i = lane; i < IMET54_FRAME; i += 64) o->frame[i] = L->fr[i];
                    if (lane < 4) o->pad[lane] = 0;
                    if (lane == 0) {
                        o->channel = ch; o->mv = mv_hdr; o->hdr_bit = hdr_bit; o->inv = inv; o->ecc_frm = v.ecc_frm; o->ecc_tlm = v.ecc_tlm; o->ecc_std = v.ecc_std;
                        o->crc_std = v.crc_std; o->crc_cont = v.crc_cont;
                    }
                }
                rsw_wave_sync();
                mode = 0; done = 0; carry_n = 0;                          // the ring is still the header's 40 symbols: the search resumes on it
            }
        }
    }
    rsw_wave_sync();
    if (lane < IMET54_HEADLEN) st->hist[lane] = L->hist[lane];
    if (lane < IMET54_CHARSYM) st->carry[lane] = L->carry[lane];
    if (mode == 1) for (int i = lane; i < IMET54_CHARS; i += 64) st->chr[i] = L->chr[i];
    if (lane == 0) { st->mode = mode; st->inv = inv; st->done = done; st->carry_n = carry_n; st->mv = mv_hdr; st->hdr_bit = hdr_bit; st->bits_in = bits0 + (unsigned long long)nb; }
}
#endif
