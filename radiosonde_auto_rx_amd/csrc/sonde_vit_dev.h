// sonde_vit_dev.h — `lms6Xmod --softin --vit / --vit2` behind the modem on ONE wavefront per channel: header search, block assembly and the K = 7 rate-1/2
// Viterbi decoder whose trellis has as many states as the wave has lanes.  Behaviour reproduced (not code): demod/mod/lms6Xmod.c main :1352-1433 (header in
// either polarity, bc, the sign flip of every second raw bit, the 80 sync positions), viterbi :232-341 (vit_start's warm-up, `<=` keeps the first candidate,
// first minimum at the end), deconv :343-374, bits2bytes :415-441.  The host mirror is sonde_lms6_fields.cpp; what follows block_bytes (RS(255,223), frame
// sync, CRC, text) stays there (sonde_lms6_dec_block_bytes).
//
//   step t, lane s:  wA = w[s >> 1] + d(code[s], rc[2t..]),  wB = w[(s >> 1) + 32] + d(code[s + 64], rc[2t..]);  the first is kept when wA <= wB (always for
//   t < 6, where only 2^t states exist).  The 64 decisions of a step are one ballot; the words go to LDS, 64 steps at a time.  Lane 0 then walks back from the
//   first minimum, re-encodes the path into hard bits and runs deconv over them exactly as the reference does (a path whose first six input bits are not zero
//   makes deconv stop early: that too is reproduced); bytes are cut on a lane each.
//
// Compiled twice, like sonde_rs_dev.h: by hipcc into k_softin_lms6 (sonde_softin_dev.hip) and by g++ under tests/emu/wave_emu.h (tests/emu/softin_lms6_emu.cpp).
// Control flow around every cross-lane primitive is wave-uniform.
#ifndef SONDE_VIT_DEV_H
#define SONDE_VIT_DEV_H
#include <stdint.h>
#include <string.h>
#include "sonde_rs_dev.h"
#include "sonde_softhdr_dev.h"
#pragma clang fp contract(off)

// ---- the primitives sonde_rs_dev.h does not have: a float from a lane of each lane's own choosing, and a counter shared by the waves of a launch
#ifndef SONDE_RS_EMU
static RSW_DEV float vitw_shfl_f(float v, int src) { return __shfl(v, src); }
static RSW_DEV void vitw_shfl2_f(float v, int srcA, int srcB, float &a, float &b) { a = __shfl(v, srcA); b = __shfl(v, srcB); }
static RSW_DEV unsigned vitw_atomic_inc(unsigned *p) { return atomicAdd(p, 1u); }
#else
static inline void vitw_shfl2_f(float v, int srcA, int srcB, float &a, float &b) {
    emu::Wave &w = emu::my_wave(); int32_t u; memcpy(&u, &v, 4); w.buf[emu::tid() & 63] = u; emu::wave_rendezvous();
    int32_t ua = (int32_t)w.buf[srcA & 63], ub = (int32_t)w.buf[srcB & 63]; emu::wave_rendezvous();
    memcpy(&a, &ua, 4); memcpy(&b, &ub, 4);
}
static inline float vitw_shfl_f(float v, int src) { float a, b; vitw_shfl2_f(v, src, src, a, b); return a; }
static inline unsigned vitw_atomic_inc(unsigned *p) { return (*p)++; }
#endif

#define LMS6_BLOCKSTART 80                      // sync positions in front of a block's raw bits (:1208-1213)
#define LMS6_RAWBLK6    (261 * 16)              // rawbitblock_len: 4096 + 80 (LMS6)
#define LMS6_RAWBLKX    (300 * 16)              //                  4720 + 80 (LMS-X)
#define LMS6_BB_LEN     308                     // block_bytes[FRAME_LEN + 8]

// a channel between calls (global memory)
struct Lms6Chan {
    int   mode;                    // 0 searching, 1 inside a block
    int   pos;                     // positions of the block filled (80 .. rawblk_len)
    int   rawblk_len;              // of the type in effect; with auto detection the host moves it between blocks
    int   consumed;                // soft bits of the call in progress read so far (a channel that stopped at a block, see stop_at_block)
    unsigned bc;
    float mv;                      // score of the header in front of the block in progress
    unsigned long long bits_in, hdr_bit;
    float hist[64];                // hdb.sbuf: the last 64 soft bits seen while searching, oldest first
    float sb[LMS6_RAWBLKX];        // blk_rawbits[].sb of the block in progress
};
// a completed block
struct Lms6Block {
    int   channel, pos, err, blen; // raw positions read, deconv's error index, bytes cut
    int   more;                    // the channel stopped here with input of the call left (auto detection)
    float mv;
    unsigned long long hdr_bit;
    unsigned char bytes[LMS6_BB_LEN + 4];
};
// LDS of a wave: 19200 + 19200 + 256 = 38656 B
struct Lms6Lds {
    float sb[LMS6_RAWBLKX];                        // soft values of the block; after the forward pass: the path's hard bits and deconv's characters
    unsigned long long dec[LMS6_RAWBLKX / 2];      // survivor decisions, a word per step
    float hist[64];
};

static RSW_DEV int lms6_code(const int bits) {     // code word of (state, input) = 7 bits, newest lowest: polynomials 1001111 / 1101101 (:232-237)
    return (__builtin_popcount(bits & 0x4F) & 1) << 1 | (__builtin_popcount(bits & 0x6D) & 1);
}
static RSW_DEV float lms6_dist2(const int c, const float sb0, const float sb1) {
    const int c0 = 2 * ((c >> 1) & 1) - 1, c1 = 2 * (c & 1) - 1;
    return (c0 - sb0) * (c0 - sb0) + (c1 - sb1) * (c1 - sb1);
}
static RSW_DEV float lms6_sync_sb(const int k) {   // positions 0 .. 79: 00 00 | 03 5d 49 c2 4f f2 68 6b as +-1
    const unsigned char s[10] = { 0x00, 0x00, 0x03, 0x5D, 0x49, 0xC2, 0x4F, 0xF2, 0x68, 0x6B };
    return (float)(2 * ((s[k >> 3] >> (7 - (k & 7))) & 1) - 1);
}

// viterbi + deconv + bits2bytes of the block in L->sb[0 .. len): bytes[LMS6_BB_LEN] (zero filled), returns blen; *err_out = deconv's value
static RSW_DEV int lms6_wave_decode(Lms6Lds *L, const int len, unsigned char *bytes, int *err_out, const int lane) {
    const int tmax = len / 2;
    const int cA = lms6_code(lane), cB = lms6_code(lane + 64), srcA = lane >> 1, srcB = (lane >> 1) + 32;
    float w = 0.f;
    for (int t0 = 0; t0 < tmax; t0 += 64) {
        unsigned long long mine = 0;
        const int n = tmax - t0 < 64 ? tmax - t0 : 64;
        for (int k = 0; k < n; k++) {
            const int t = t0 + k;
            const float sb0 = L->sb[2 * t], sb1 = L->sb[2 * t + 1];
            float pa, pb;
            vitw_shfl2_f(w, srcA, srcB, pa, pb);
            const float wa = pa + lms6_dist2(cA, sb0, sb1), wb = pb + lms6_dist2(cB, sb0, sb1);
            const bool first = t < 6 || wa <= wb;                       // vit_start: one predecessor only while t < K - 1
            w = first ? wa : wb;
            const unsigned long long m = rsw_ballot(!first);
            if (lane == k) mine = m;
        }
        if (lane < n) L->dec[t0 + lane] = mine;
    }
    // the first minimum over the states in ascending order
    float mn = w;
    for (int d = 32; d > 0; d >>= 1) { const float o = vitw_shfl_f(mn, lane ^ d); mn = o < mn ? o : mn; }
    const unsigned long long at = rsw_ballot(w == mn);
    const int j_min = at ? __builtin_ctzll(at) : 0;
    rsw_wave_sync();
    unsigned char *vr = (unsigned char *)L->sb;                           // the path's code bits as '0' / '1', NUL behind them
    char *bits = (char *)L->sb + (LMS6_RAWBLKX + 16);                     // deconv's output
    int nstr = 0, err = 0;
    if (lane == 0) {
        int j = j_min;
        vr[2 * tmax] = 0;
        for (int t = tmax; t > 0; t--) {
            const int d = (int)((L->dec[t - 1] >> j) & 1ull), c = lms6_code(j + 64 * d);
            vr[2 * t - 2] = (unsigned char)(0x30 + ((c >> 1) & 1));
            vr[2 * t - 1] = (unsigned char)(0x30 + (c & 1));
            j = (j >> 1) + 32 * d;
        }
        // deconv (:343-374): six zero bits assumed in front; reg bit i = bits[n + i] & 1
        constexpr int m = 6;
        for (int i = 0; i < m; i++) bits[i] = '0';
        int n = 0; unsigned reg = 0;
        while (2 * (m + n) < 2 * tmax) {
            const unsigned char *p = vr + 2 * (m + n);
            const int a = (__builtin_popcount(reg & 0x39u) & 1) ^ (p[0] & 1), b = (__builtin_popcount(reg & 0x1Bu) & 1) ^ (p[1] & 1);
            int nb;
            if (a == 1 && b == 1) nb = 1;
            else if (a == 0 && b == 0) nb = 0;
            else { bits[n + m] = (a != 1 && b == 1) ? 0x39 : 0x38; err = n; break; }
            bits[n + m] = (char)('0' + nb);
            reg = (reg >> 1) | ((unsigned)nb << 5);
            n += 1;
        }
        bits[n + m] = 0;
        nstr = err ? err : n + m;                                         // proc_frame cuts the string at the error index (:874)
        if (err) bits[err] = 0;
    }
    rsw_wave_sync();
    nstr = rsw_bcast(nstr, 0); err = rsw_bcast(err, 0);
    const int blen = nstr / 8;
    for (int b = lane; b < LMS6_BB_LEN; b += 64) {                        // bits2bytes: LSB first, '1' and '9' count
        int v = 0;
        if (b < blen) for (int i = 0; i < 8; i++) { const char c = bits[8 * b + i]; if (c == '1' || c == '9') v += 1 << i; }
        bytes[b] = (unsigned char)v;
    }
    rsw_wave_sync();
    *err_out = err;
    return blen;
}

// One channel, one call: nb soft bits at x (sgn = -1: --softinv).  vit: 1 = hard values into the decoder, 2 = soft.  stop_at_block: return at the first
// completed block if input is left (the next block's length is the host decoder's to say).  hdr: the 64 raw header bits as characters.
static RSW_DEV void lms6_wave_channel(Lms6Chan *st, const float *x, const int nb, const float sgn, const int vit, const int stop_at_block, const unsigned char *hdr,
                                      Lms6Lds *L, Lms6Block *out, unsigned *count, const int cap, const int ch, const int lane) {
    int mode = st->mode, pos = st->pos, cur = st->consumed; const int rawblk = st->rawblk_len;
    unsigned bc = st->bc; float mv_hdr = st->mv; unsigned long long hdr_bit = st->hdr_bit; const unsigned long long bits0 = st->bits_in;
    if (rawblk < LMS6_BLOCKSTART || rawblk > LMS6_RAWBLKX || pos < LMS6_BLOCKSTART || pos > rawblk || cur < 0) return;      // (never: the host writes 4176 or 4800)
    L->hist[lane] = st->hist[lane];
    for (int i = lane; i < LMS6_BLOCKSTART; i += 64) L->sb[i] = lms6_sync_sb(i);
    if (mode == 1) for (int i = LMS6_BLOCKSTART + lane; i < pos; i += 64) L->sb[i] = st->sb[i];
    rsw_wave_sync();
    bool stopped = false;
    while (cur < nb && !stopped) {
        if (mode == 0) {
            bool found = false;
            for (int base = cur; base < nb && !found; base += 64) {
                const int q = base + lane;
                float mv = 0.f;
                if (q < nb) mv = softhdr_corr64(L->hist, x, sgn, cur, q, hdr);
                const unsigned long long hits = rsw_ballot(q < nb && fabsf(mv) > 0.7f);
                if (hits) {
                    const int l = __builtin_ctzll(hits), qs = base + l;
                    const float mvl = vitw_shfl_f(mv, l);
                    const float v = softhdr_ring64(L->hist, x, sgn, cur, qs, lane);
                    rsw_wave_sync();
                    L->hist[lane] = v;
                    rsw_wave_sync();
                    found = true;
                    mode = 1; pos = LMS6_BLOCKSTART; bc = mvl > 0 ? 0u : 1u; mv_hdr = mvl; hdr_bit = bits0 + (unsigned long long)qs + 1ull;
                    cur = qs + 1;
                }
            }
            if (!found) {
                const float v = softhdr_ring64(L->hist, x, sgn, cur, nb - 1, lane);
                rsw_wave_sync();
                L->hist[lane] = v;
                rsw_wave_sync();
                cur = nb;
            }
        } else {
            const int take = nb - cur < rawblk - pos ? nb - cur : rawblk - pos;
            for (int j = lane; j < take; j += 64) {
                const float s = sgn * x[cur + j];
                const unsigned odd = (bc + (unsigned)j) % 2;
                const int hb = (s >= 0.0f) ^ (int)odd;                    // (c0, inv(c1))
                const int sg = -2 * (int)odd + 1;
                float sb = sg * s;
                if (vit == 1) sb = (float)(2 * hb - 1);
                L->sb[pos + j] = sb;
            }
            pos += take; bc += (unsigned)take; cur += take;
            if (pos >= rawblk) {
                rsw_wave_sync();
                unsigned slot = 0;
                if (lane == 0) slot = vitw_atomic_inc(count);
                slot = (unsigned)rsw_bcast((int)slot, 0);
                const bool keep = (int)slot < cap && (int)slot >= 0;
                // (a record the buffer cannot take is decoded into the block's own LDS tail and dropped: the host counts it)
                unsigned char *by = keep ? out[slot].bytes : (unsigned char *)L->sb + 3 * LMS6_RAWBLKX;
                int err = 0;
                const int blen = lms6_wave_decode(L, rawblk, by, &err, lane);
                const bool more = stop_at_block && cur < nb;
                if (keep && lane == 0) {
                    Lms6Block *o = out + slot;
                    o->channel = ch; o->pos = pos; o->err = err; o->blen = blen; o->more = more ? 1 : 0; o->mv = mv_hdr; o->hdr_bit = hdr_bit;
                }
                for (int i = lane; i < LMS6_BLOCKSTART; i += 64) L->sb[i] = lms6_sync_sb(i);
                rsw_wave_sync();
                mode = 0; pos = LMS6_BLOCKSTART;
                stopped = more;
            }
        }
    }
    rsw_wave_sync();
    st->hist[lane] = L->hist[lane];
    if (mode == 1) for (int i = LMS6_BLOCKSTART + lane; i < pos; i += 64) st->sb[i] = L->sb[i];
    if (lane == 0) {
        st->mode = mode; st->pos = pos; st->bc = bc; st->mv = mv_hdr; st->hdr_bit = hdr_bit;
        if (stopped) st->consumed = cur;
        else { st->consumed = 0; st->bits_in = bits0 + (unsigned long long)(nb > 0 ? nb : 0); }
    }
}
#endif
