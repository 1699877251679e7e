// sonde_softin_wxr_dev.h — `weathex301d --softin [-i] [--pn9]` behind the modem on ONE wavefront per channel: the sign of every soft bit into the 40-bit header
// ring, 512 bits behind a ring that equals the header, and at the end of a frame the 69 bytes, the PN9 de-whitening and the xor8 / sum8 check on the same wave.
// Behaviour reproduced (not code): weathex/weathex301d.c main :607-648 (bit = (s >= 0), with -i (s <= 0), so +-0.0 is a 1 and a NaN a 0 either way; EVERY bit
// enters the ring, frame bits included; the ring starts as 'x' / NUL characters, so nothing matches before 40 bits have been read; outside a frame a ring equal
// to AA AA AA 2D D4 — with --pn9 AA AA AA C1 94 — opens one, whose first 40 bits are the header; inside a frame the header is not searched for), compare :250-256,
// bits2bytes :272-294 and print_frame up to the verdict :359-375.  The host mirror is sonde_wxr_softin_push + sonde_wxr_print_frame (sonde_wxr_fields.cpp).
//
//   search: 64 soft bits a pass.  Signs by ballot; the ring is two 40-bit masks (values, "holds a bit"), newest bit lowest, and every lane tests the ring as it
//           stands behind its own bit of the pass; the first hit is taken by ballot (the scheme of k_softin_drop).  hdr_bit = soft bits read before the matching one.
//   frame:  up to 64 bits a pass, each pass's ballot ORed into the frame's bit words in LDS.  The ring is not kept while a frame is open — nothing reads it — and
//           behind the 552nd bit it is the frame's last 40 bits, so a header that ends right behind a frame is found.
//   end of frame (wxr_wave_end): byte k of 69 on lane k (two rounds), MSB first; with --pn9 bytes 6 .. 68 XORed with the PN9 sequence; xor8 and sum8 over the 53
//           bytes from ofs (6, with --pn9 8) as reductions over the wave; the verdict, frame id, serial and counter are the same on every lane.
//
// Only COMPLETE frames are delivered: a consumer behind a live modem has no end of input.  The soft decisions are read once, so nothing is staged.
//
// Compiled twice, like sonde_softin_mts01_dev.h: by hipcc into k_softin_wxr (sonde_softin_dev.hip) and by g++ under tests/emu/wave_emu.h
// (tests/emu/softin_wxr_emu.cpp).  Control flow around every cross-lane primitive is wave-uniform; no indexed local array, so nothing goes to scratch.
#ifndef SONDE_SOFTIN_WXR_DEV_H
#define SONDE_SOFTIN_WXR_DEV_H
#include "sonde_softin_wave_dev.h"                                     // the slot of a record, softin_wave_xor, the rsw_* primitives

#define WXR_HEADLEN  40                                               // bits of the header ring
#define WXR_NBITS    552                                              // bits of a frame, header included: 8 * 69
#define WXR_WORDS    18                                               // 32-bit words of the frame's bits, bit i in bit i & 31 of word i >> 5
#define WXR_NBYTES   69
#define WXR_CHKLEN   53                                               // bytes under the check, from byte ofs
#define WXR_M40      ((1ULL << WXR_HEADLEN) - 1)

// the format's whitening sequence from frame byte 6 on (TI SWRA322)
#ifndef SONDE_RS_EMU
#define WXR_CONST __constant__
static RSW_DEV unsigned long long wxr_brev64(unsigned long long v) { return __brevll(v); }
#else
#define WXR_CONST
static inline unsigned long long wxr_brev64(unsigned long long v) {
    unsigned long long r = 0;
    for (int i = 0; i < 64; i++) r |= ((v >> i) & 1ULL) << (63 - i);
    return r;
}
#endif
static WXR_CONST const uint8_t kWxrPn9[64] = { 0xFF, 0x87, 0xB8, 0x59, 0xB7, 0xA1, 0xCC, 0x24, 0x57, 0x5E, 0x4B, 0x9C, 0x0E, 0xE9, 0xEA, 0x50,
                                               0x2A, 0xBE, 0xB4, 0x1B, 0xB6, 0xB0, 0x5D, 0xF1, 0xE6, 0x9A, 0xE3, 0x45, 0xFD, 0x2C, 0x53, 0x18,
                                               0x0C, 0xCA, 0xC9, 0xFB, 0x49, 0x37, 0xE5, 0xA8, 0x51, 0x3B, 0x2F, 0x61, 0xAA, 0x72, 0x18, 0x84,
                                               0x02, 0x23, 0x23, 0xAB, 0x63, 0x89, 0x51, 0xB3, 0xE7, 0x8B, 0x72, 0x90, 0x4C, 0xE8, 0xFB, 0xC1 };

// the header as the ring holds it when it matches: the first bit on the air highest, the newest lowest (weathex301d.c header[] / header_pn9[])
static RSW_DEV unsigned long long wxr_header40(const int pn9) { return pn9 ? 0xAAAAAAC194ULL : 0xAAAAAA2DD4ULL; }

// a completed frame as the kernel leaves it (176 bytes; sonde_wxr_softin_rec_t of include/sonde_fsk.h)
struct SoftinWxrRec {
    int32_t  channel;
    int32_t  pad;
    unsigned long long hdr_bit;    // soft bits read before the one that completed the header
    uint8_t  raw[WXR_NBYTES];      // the 552 frame bits, MSB first, before PN9 (what -R prints)
    uint8_t  x[WXR_NBYTES];        // behind PN9 (without --pn9 the same bytes)
    uint8_t  pad2[2];
    uint32_t chkval, chkdat;       // computed (xor8 << 8 | sum8) and stored check
    uint8_t  chk_ok, frid;
    uint8_t  pad3[2];
    uint32_t sn, cnt;
};
// a channel between calls (global memory)
struct SoftinWxrChan {
    int mode;                      // 0 searching, 1 inside a frame
    int pos;                       // bits of the frame so far (40 .. 551 inside a frame, else 0)
    unsigned long long hist, valid;// the ring: values and "holds a bit", newest bit lowest; as the header left it while a frame is open
    unsigned long long bits_in, hdr_bit;
    uint32_t w[WXR_WORDS];         // the bits of the frame in progress
};
// LDS of a wave: 72 + 72 + 72 = 216 B
struct SoftinWxrLds {
    uint32_t w[WXR_WORDS];
    uint8_t raw[WXR_NBYTES + 3];
    uint8_t x[WXR_NBYTES + 3];
};
struct WxrVerdict { uint32_t chkval, chkdat, sn, cnt; int chk_ok, frid; };

// the ring after bits 0 .. k of a pass (bm: bit i = soft bit i of the pass)
static RSW_DEV void wxr_ring_after(const unsigned long long hist, const unsigned long long valid, const unsigned long long bm, const int k,
                                   unsigned long long &h, unsigned long long &v) {
    const unsigned long long fresh = wxr_brev64(bm) >> (63 - k), ones = (2ULL << k) - 1;          // bits 0 .. k, bit 0 highest
    h = ((k + 1 >= WXR_HEADLEN ? 0 : hist << (k + 1)) | fresh) & WXR_M40;
    v = ((k + 1 >= WXR_HEADLEN ? 0 : valid << (k + 1)) | ones) & WXR_M40;
}
// sum of v over the 64 lanes, on every lane
static RSW_DEV uint32_t wxr_wave_sum(uint32_t v, const int lane) {
    for (int d = 1; d < 64; d <<= 1) v += (uint32_t)rsw_shfl_up((int)v, d, lane);
    return (uint32_t)rsw_bcast((int)v, 63);
}

// print_frame's look at the 552 bits in L->w (weathex301d.c:359-375): L->raw / L->x get the 69 bytes before / behind PN9; the return value is the same on every lane
static RSW_DEV WxrVerdict wxr_wave_end(SoftinWxrLds *L, const int pn9, const int lane) {
    for (int k = lane; k < WXR_NBYTES + 3; k += 64) {
        uint32_t rv = 0, xv = 0;
        if (k < WXR_NBYTES) {
            const uint32_t by = (L->w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
            for (int i = 0; i < 8; i++) rv |= ((by >> i) & 1u) << (7 - i);                         // MSB first
            xv = (pn9 && k >= 6) ? rv ^ kWxrPn9[k - 6] : rv;
        }
        L->raw[k] = (uint8_t)rv; L->x[k] = (uint8_t)xv;
    }
    rsw_wave_sync();
    const int ofs = pn9 ? 8 : 6;
    const uint32_t b = lane < WXR_CHKLEN ? (uint32_t)L->x[ofs + lane] : 0u;
    const uint32_t x8 = softin_wave_xor(b, lane) & 0xFFu, s8 = wxr_wave_sum(b, lane) & 0xFFu;
    WxrVerdict v;
    v.chkval = x8 << 8 | s8;
    v.chkdat = (uint32_t)L->x[ofs + WXR_CHKLEN] << 8 | (uint32_t)L->x[ofs + WXR_CHKLEN + 1];
    v.chk_ok = v.chkval == v.chkdat ? 1 : 0;
    v.sn = (uint32_t)L->x[ofs] | (uint32_t)L->x[ofs + 1] << 8 | (uint32_t)L->x[ofs + 2] << 16 | (uint32_t)L->x[ofs + 3] << 24;
    v.cnt = (uint32_t)L->x[ofs + 4] | (uint32_t)L->x[ofs + 5] << 8;
    v.frid = L->x[ofs + 6];
    return v;
}

// One channel, one call: nb soft bits at x.  inv = -i XOR the stream's own inversion (bit = inv ? s <= 0 : s >= 0).  Completed frames go to out[slot], slot from
// *count; a slot at or beyond cap is decoded and counted, not written.
static RSW_DEV void wxr_wave_channel(SoftinWxrChan *st, const float *x, const int nb, const int inv, const int pn9, SoftinWxrLds *L, SoftinWxrRec *out,
                                     unsigned *count, const int cap, const int ch, const int lane) {
    int mode = st->mode, pos = st->pos;
    unsigned long long hist = st->hist, valid = st->valid, hdr_bit = st->hdr_bit; const unsigned long long bits0 = st->bits_in;
    if (mode < 0 || mode > 1 || (mode == 1 ? (pos < WXR_HEADLEN || pos >= WXR_NBITS) : pos != 0) || nb < 0) return;       // (never: the host zeroes the state)
    if (lane < WXR_WORDS) L->w[lane] = mode == 1 ? st->w[lane] : 0u;
    rsw_wave_sync();
    const unsigned long long hdr40 = wxr_header40(pn9);
    int cur = 0;
    while (cur < nb) {
        if (mode == 0) {
            const int q = cur + lane, nv = nb - cur < 64 ? nb - cur : 64;
            const float s = x[q < nb ? q : cur];
            const unsigned long long bm = rsw_ballot(q < nb && (inv ? s <= 0.0f : s >= 0.0f));
            unsigned long long h, v;
            wxr_ring_after(hist, valid, bm, lane, h, v);
            const unsigned long long hm = rsw_ballot(lane < nv && h == hdr40 && v == WXR_M40);
            const int used = hm ? __builtin_ctzll(hm) + 1 : nv;
            wxr_ring_after(hist, valid, bm, used - 1, h, v);
            hist = h; valid = v;
            if (hm) {
                // the frame's first 40 bits are the header (strncpy(frame_bits, hdr, HEADLEN)): frame bit i = header bit i, the first on the air
                const unsigned long long hw = wxr_brev64(hdr40) >> (64 - WXR_HEADLEN);
                if (lane < WXR_WORDS) L->w[lane] = lane == 0 ? (uint32_t)hw : lane == 1 ? (uint32_t)(hw >> 32) : 0u;
                rsw_wave_sync();
                mode = 1; pos = WXR_HEADLEN; hdr_bit = bits0 + (unsigned long long)(cur + used - 1);
            }
            cur += used;
        } else {
            const int left = WXR_NBITS - pos, take = nb - cur < left ? nb - cur : left;
            const int cur0 = cur;
            for (int r0 = 0; r0 < take; r0 += 64) {
                const int j = r0 + lane;
                const float s = x[cur0 + (j < take ? j : 0)];
                const unsigned long long m = rsw_ballot(j < take && (inv ? s <= 0.0f : s >= 0.0f));
                // frame bit f0 + l from lane l: up to three words
                const int f0 = pos + r0, sh = f0 & 31, idx = (f0 >> 5) + lane;
                if (lane < 3 && idx < WXR_WORDS) {
                    const uint32_t v = lane == 0 ? (uint32_t)(m << sh) : lane == 1 ? (uint32_t)(m >> (32 - sh)) : sh ? (uint32_t)(m >> (64 - sh)) : 0u;
                    L->w[idx] |= v;
                }
                rsw_wave_sync();
            }
            pos += take; cur += take;
            if (pos == WXR_NBITS) {
                const WxrVerdict v = wxr_wave_end(L, pn9, lane);
                const unsigned slot = softin_wave_slot(count, lane);
                if ((int)slot < cap && (int)slot >= 0) {
                    SoftinWxrRec *o = out + slot;
                    for (int k = lane; k < WXR_NBYTES; k += 64) { o->raw[k] = L->raw[k]; o->x[k] = L->x[k]; }
                    if (lane == 0) {
                        o->channel = ch; o->pad = 0; o->hdr_bit = hdr_bit; o->pad2[0] = o->pad2[1] = 0; o->chkval = v.chkval; o->chkdat = v.chkdat;
                        o->chk_ok = (uint8_t)v.chk_ok; o->frid = (uint8_t)v.frid; o->pad3[0] = o->pad3[1] = 0; o->sn = v.sn; o->cnt = v.cnt;
                    }
                }
                // the search resumes on a ring that holds the frame's last 40 bits: frame bits 512 .. 551, the last one lowest
                const unsigned long long tail = (unsigned long long)L->w[16] | (unsigned long long)(L->w[17] & 0xFFu) << 32;
                hist = wxr_brev64(tail) >> (64 - WXR_HEADLEN); valid = WXR_M40;
                rsw_wave_sync();
                mode = 0; pos = 0;
            }
        }
    }
    rsw_wave_sync();
    if (mode == 1 && lane < WXR_WORDS) st->w[lane] = L->w[lane];
    if (lane == 0) { st->mode = mode; st->pos = pos; st->hist = hist; st->valid = valid; st->hdr_bit = hdr_bit; st->bits_in = bits0 + (unsigned long long)nb; }
}
#endif
