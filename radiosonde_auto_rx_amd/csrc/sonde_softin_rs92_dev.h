// sonde_softin_rs92_dev.h — `rs92mod --softin [-i] --ecc` behind the modem on ONE wavefront per channel: header search on the symbol stream, 8N1 bytes from two
// soft symbols per bit on a lane per byte, and RS(255,231) of the finished frame on the same wave (rs255_wave_decode, sonde_rs_dev.h: RS92 uses the RS41 code).
// Behaviour reproduced (not code): demod/mod/rs92mod.c main :1959-2050 (find_softbinhead on the 60 raw header symbols of :88-92 at 0.8, the ring zeroed on every hit
// :1988, a hit of the other polarity dropped — rs92mod has no --auto —, 234 bytes of 10 bits behind the hit), bits2byte :183-196 (bits 1..8, LSB first; start and
// stop bit not looked at), rs92_ecc :1360-1385 (cw = 24 parity bytes, 210 message bytes, 21 zeros; repaired bytes written back on success, the frame left alone on
// failure); find_softbinhead / corr_softhdb are demod_mod.c:1692-1762.  The host mirror is sonde_rs92_dec_push_soft (sonde_rs92_fields.cpp).
//
//   search: a lane per stream position; the normalised correlation in float first, and every position that is not safely below the threshold again the
//           reference's way (float products, double sums in order, sum / sqrt(normx * 60.0), rounded to float): that value decides (fabs(mv) > 0.8f; 0.8f itself
//           and the NaN of an all-zero window are no hits) and is recorded.  Every hit, accepted or dropped, leaves an empty ring; the ring is advanced only
//           while searching, so the search behind a frame starts on the empty ring its header left.
//   frame:  a lane per byte (20 symbols); the symbols of an unfinished byte and the bytes of the frame in progress survive a call in device memory.
//   end of frame (240 bytes = 4680 symbols behind the hit): the codeword in LDS, its 24 syndromes S_j = cw(alpha^j) on 48 lanes (two halves of the Horner sum, as
//           rs41_syndrome_partials splits it), rs255_wave_decode, write-back, one record.  ECC is always on: the reference's --json path and the host tier force it.
//
// Only COMPLETE frames are delivered: the reference prints a partial frame only at end of input (:2045), and a consumer behind a live modem has no end of input.
//
// Compiled twice, like sonde_softin_mxx_dev.h: by hipcc into k_softin_rs92 (sonde_softin_dev.hip) and by g++ under tests/emu/wave_emu.h (tests/emu/softin_rs92_emu.cpp).
// Control flow around every cross-lane primitive is wave-uniform.
#ifndef SONDE_SOFTIN_RS92_DEV_H
#define SONDE_SOFTIN_RS92_DEV_H
#include "sonde_softin_wave_dev.h"                                     // the staged call, softin_wave_score<HL>, the ring refresh, the slot of a record
// (no contraction: the reference is plain C on x86-64 — every product and sum rounded on its own)
#pragma clang fp contract(off)

#define RS92_HEADLEN    60
#define RS92_FRAME_LEN  240
#define RS92_FRAMESTART 6
#define RS92_BYTESYM    20                                            // symbols of a byte: 10 bits, two symbols each
#define RS92_NSYM       ((RS92_FRAME_LEN - RS92_FRAMESTART) * RS92_BYTESYM)   // 4680 symbols behind the header
#define RS92_RS_R       24
#define RS92_MSGLEN     (RS92_FRAME_LEN - RS92_FRAMESTART - RS92_RS_R) // 210
// the raw header rs92mod hands to find_softbinhead (rs92mod.c:88-92: 2A 2A 10 as 8N1 Manchester), symbol i in bit i
static RSW_DEV unsigned long long rs92_header_mask() {
    const char h[RS92_HEADLEN + 1] = "10100110011001101001" "1010011001100110100110101010100110101001";
    unsigned long long m = 0;
    for (int i = 0; i < RS92_HEADLEN; i++) m |= (unsigned long long)(h[i] & 1) << i;
    return m;
}

// a completed frame as the kernel leaves it
struct SoftinRs92Rec {
    int32_t  channel;
    int32_t  ec;                   // rs_decode's value: 0, the repaired count, -1 / -2 / -3
    float    mv;                   // score of the header in front of the frame (the double form, rounded)
    int32_t  pad;
    unsigned long long hdr_bit;    // symbols read when the header matched
    uint8_t  frame[RS92_FRAME_LEN];
};
// a channel between calls (global memory)
struct SoftinRs92Chan {
    int   mode;                    // 0 searching, 1 inside a frame
    int   done;                    // symbols of the frame consumed (0 .. 4680), the pending ones included
    int   carry_n;                 // symbols of an unfinished byte
    float mv;                      // score of the header in front of the frame in progress
    unsigned long long bits_in, hdr_bit;
    float carry[RS92_BYTESYM];
    float hist[RS92_HEADLEN];      // hdb.sbuf: the last 60 symbols seen while searching, oldest first; zeros behind a hit
    uint8_t frame[RS92_FRAME_LEN];
};
// LDS of a wave besides the staged soft decisions: 240 + 80 + 240 + 256 + 64 + 768 = 1648 B
struct SoftinRs92Lds {
    float hist[RS92_HEADLEN];
    float carry[RS92_BYTESYM];
    uint8_t frame[RS92_FRAME_LEN];
    uint8_t cw[256];
    uint8_t scr[64];
    uint8_t gexp[512], glog[256];
};

// rs92_ecc() on the 240 frame bytes in L->frame (rs92mod.c:1360-1385); L->gexp / L->glog hold the GF tables.  Returns rs_decode's value on every lane.
static RSW_DEV int rs92_wave_ecc(SoftinRs92Lds *L, const int lane) {
    const RsGf g{L->gexp, L->glog};
    for (int i = lane; i < 256; i += 64)
        L->cw[i] = i < RS92_RS_R ? L->frame[RS92_FRAME_LEN - RS92_RS_R + i] : i < RS92_RS_R + RS92_MSGLEN ? L->frame[RS92_FRAMESTART + (i - RS92_RS_R)] : 0;
    rsw_wave_sync();
    // S_j = cw(alpha^j), j < 24: lanes 0..23 the coefficients 0..127, lanes 24..47 the coefficients 128..255 scaled by alpha^(128 j)
    if (lane < 48) {
        const int half = lane / RS92_RS_R, jx = lane % RS92_RS_R;
        int h = 0;
        for (int i = 127; i >= 0; i--) {
            const int n = 128 * half + i;
            h = rs_gf_mul_l(g, h, jx) ^ (n < 255 ? L->cw[n] : 0);
        }
        L->scr[lane] = (uint8_t)(h ? g.exp[(g.log[h] + (jx * 128 * half) % 255) % 255] : 0);
    }
    rsw_wave_sync();
    const int syn = lane < RS92_RS_R ? L->scr[lane] ^ L->scr[RS92_RS_R + lane] : 0;
    rsw_wave_sync();
    const int ec = rs255_wave_decode(L->cw, syn, L->scr, g, lane);
    rsw_wave_sync();
    // (a failed decode leaves cw as it was: the frame keeps its bytes, as rs92_ecc leaves gpx->frame)
    for (int i = lane; i < RS92_RS_R + RS92_MSGLEN; i += 64) {
        if (i < RS92_RS_R) L->frame[RS92_FRAME_LEN - RS92_RS_R + i] = L->cw[i]; else L->frame[RS92_FRAMESTART + (i - RS92_RS_R)] = L->cw[i];
    }
    rsw_wave_sync();
    return ec;
}

// One channel, one call: nb symbols at x (sgn = -1: --softinv), inv = -i.  gf: exp[512] ++ log[256] in global memory.  s_x: room for stage_cap staged symbols
// (LDS); a call of more reads x where it lies.  Completed frames go to out[slot], slot from *count; a slot at or beyond cap is decoded and counted, not written.
static RSW_DEV void rs92_wave_channel(SoftinRs92Chan *st, const float *x, const int nb, const float sgn, const int inv, const float ths, const uint8_t *gf,
                                      SoftinRs92Lds *L, float *s_x, const int stage_cap, SoftinRs92Rec *out, unsigned *count, const int cap, const int ch, const int lane) {
    int mode = st->mode, done = st->done, carry_n = st->carry_n;
    float mv_hdr = st->mv; unsigned long long hdr_bit = st->hdr_bit; const unsigned long long bits0 = st->bits_in;
    if (done < 0 || done > RS92_NSYM || carry_n < 0 || carry_n >= RS92_BYTESYM || carry_n > done || nb < 0) return;       // (never: the host zeroes the state)
    if (lane < RS92_HEADLEN) L->hist[lane] = st->hist[lane];
    if (lane < RS92_BYTESYM) L->carry[lane] = st->carry[lane];
    for (int i = lane; i < RS92_FRAME_LEN; i += 64) L->frame[i] = st->frame[i];
    for (int i = lane; i < 512; i += 64) L->gexp[i] = gf[i];
    for (int i = lane; i < 256; i += 64) L->glog[i] = gf[512 + i];
    const SoftinX X = softin_wave_stage(s_x, x, sgn, nb, stage_cap, lane);                        // symbol p of this call, --softinv applied
    rsw_wave_sync();
    const unsigned long long hbits = rs92_header_mask();
    int cur = 0;
    while (cur < nb) {
        if (mode == 0) {
            // element k of hist ++ the call's symbols from `cur`
            const int cur0 = cur;
            auto W = [&](const int k) -> float { return k < RS92_HEADLEN ? L->hist[k] : X(cur0 + (k - RS92_HEADLEN)); };
            bool stop = false;
            for (int base = cur0; base < nb && !stop; base += 64) {
                const int q = base + lane;
                float mv = 0.f;
                if (q < nb) mv = softin_wave_score<RS92_HEADLEN>(W, q - cur0 + 1, hbits, ths);     // the window of position q ends with the symbol at q
                const unsigned long long hits = rsw_ballot(q < nb && fabsf(mv) > ths);
                if (hits) {
                    // the first hit counts; whatever the lanes behind it saw, they saw over a ring this hit empties: the search goes on from the next symbol
                    const int l = __builtin_ctzll(hits), qs = base + l;
                    const float mvl = mxxw_bcast_f(mv, l);
                    rsw_wave_sync();
                    if (lane < RS92_HEADLEN) L->hist[lane] = 0.f;         // (:1988) on every hit, of either polarity
                    rsw_wave_sync();
                    stop = true;
                    cur = qs + 1;
                    if (!((double)mvl * (0.5 - inv) < 0)) {               // a header of the other polarity is not this decoder's (:1999-2002)
                        mode = 1; done = 0; carry_n = 0; mv_hdr = mvl; hdr_bit = bits0 + (unsigned long long)qs + 1ull;
                        if (lane < RS92_FRAMESTART) L->frame[lane] = lane < 5 ? 0x2A : 0x10;
                    }
                }
            }
            if (!stop) {
                softin_wave_ring<RS92_HEADLEN>(L->hist, W, nb - cur0, lane);                       // the 60 elements up to the call's last symbol
                cur = nb;
            }
        } else {
            // bytes from the pending symbols of the last call and the new ones: bit = (s2 - s1 >= 0) ^ inv, the byte = bits 1..8, LSB first
            const int left = RS92_NSYM - done, take = nb - cur < left ? nb - cur : left;
            const int tot = carry_n + take, nbytes = tot / RS92_BYTESYM, byte0 = RS92_FRAMESTART + (done - carry_n) / RS92_BYTESYM;
            auto S = [&](const int k) -> float { return k < carry_n ? L->carry[k] : X(cur + (k - carry_n)); };
            for (int j = lane; j < nbytes; j += 64) {
                unsigned byte = 0;
                for (int b = 1; b <= 8; b++) {
                    const float s1 = S(RS92_BYTESYM * j + 2 * b), s2 = S(RS92_BYTESYM * j + 2 * b + 1);
                    const int bit = ((s2 - s1) >= 0.0f ? 1 : 0) ^ inv;
                    byte |= (unsigned)bit << (b - 1);
                }
                L->frame[byte0 + j] = (uint8_t)byte;
            }
            const int rest = tot - RS92_BYTESYM * nbytes;
            float cv = 0.f;
            if (lane < rest) cv = S(RS92_BYTESYM * nbytes + lane);
            rsw_wave_sync();
            if (lane < RS92_BYTESYM) L->carry[lane] = cv;
            rsw_wave_sync();
            carry_n = rest; done += take; cur += take;
            if (done == RS92_NSYM) {
                const int ec = rs92_wave_ecc(L, lane);
                const unsigned slot = softin_wave_slot(count, lane);
                if ((int)slot < cap && (int)slot >= 0) {
                    SoftinRs92Rec *o = out + slot;
                    for (int i = lane; i < RS92_FRAME_LEN; i += 64) o->frame[i] = L->frame[i];
                    if (lane == 0) { o->channel = ch; o->ec = ec; o->mv = mv_hdr; o->pad = 0; o->hdr_bit = hdr_bit; }
                }
                rsw_wave_sync();
                mode = 0; done = 0; carry_n = 0;                          // the ring is still the empty one the header left: the search resumes on it
            }
        }
    }
    rsw_wave_sync();
    if (lane < RS92_HEADLEN) st->hist[lane] = L->hist[lane];
    if (lane < RS92_BYTESYM) st->carry[lane] = L->carry[lane];
    if (mode == 1) for (int i = lane; i < RS92_FRAME_LEN; i += 64) st->frame[i] = L->frame[i];
    if (lane == 0) { st->mode = mode; st->done = done; st->carry_n = carry_n; st->mv = mv_hdr; st->hdr_bit = hdr_bit; st->bits_in = bits0 + (unsigned long long)nb; }
}
#endif
