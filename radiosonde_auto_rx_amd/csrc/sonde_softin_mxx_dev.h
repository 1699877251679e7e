// sonde_softin_mxx_dev.h — `m20mod --softin` behind the modem on ONE wavefront per channel: header search on the symbol stream, two soft symbols per bit,
// differential decoding, bits2bytes on a lane per byte and what print_frame() derives from the bytes (length, firmware byte, frame checksum, block checksum).
// Behaviour reproduced (not code): demod/mod/m20mod.c main :1276-1377 (find_softbinhead on the 32 raw header symbols of :81 at 0.8 in either polarity, bit0 = '0'
// at the frame's first bit, (101 + 64) * 8 bits, one symbol per counted bit dropped up to 5 * 808 below -vvv), print_frame :875-907, blk_checkM10 :548-560,
// checkM10 :562-596; find_softbinhead / corr_softhdb are demod_mod.c:1692-1762.  The host mirror is sonde_softin.cpp (SONDE_M20) + sonde_m20_frame_finish.
//
//   search: a lane per stream position; the normalised correlation in float first, and every position that is not safely below the threshold again the
//           reference's way (float products, double sums in order, sum / sqrt(normx * 32.0)): that value decides and is recorded.  The ring (hdb.sbuf) is
//           advanced only while searching.
//   frame:  a lane per bit, the previous bit from the lane below; the characters of the frame in progress survive a call in device memory.
//   end of frame: a lane per byte, then the frame checksum on lane 0 and the block checksum on lane 1.
//
// Compiled twice, like sonde_vit_dev.h: by hipcc into k_softin_m20 (sonde_softin_dev.hip) and by g++ under tests/emu/wave_emu.h (tests/emu/softin_m20_emu.cpp).
// Control flow around every cross-lane primitive is wave-uniform.  k_softin_m10 (sonde_softin_dev.hip) is the same scheme with 968 bits and M10's verdicts, a body of
// its own.  What both share with the other consumers — the staged call, the header score, the ring refresh, the slot of a record — is sonde_softin_wave_dev.h.
#ifndef SONDE_SOFTIN_MXX_DEV_H
#define SONDE_SOFTIN_MXX_DEV_H
#include "sonde_softin_wave_dev.h"                                     // the staged call, softin_wave_score<HL>, the ring refresh, the slot of a record
#include "../../include/sonde_hip.h"
// (no contraction: the reference is plain C on x86-64 — every product and sum rounded on its own)
#pragma clang fp contract(off)

#define M20_HEADLEN   32
#define M20_NBYTES    (101 + 64)                // FRAME_LEN + AUX_LEN (m20mod.c:83-87)
#define M20_NBITS     (M20_NBYTES * 8)          // 1320 bits = 2640 symbols
#define M20_SKIP_END  (5 * 808)                 // bitpos up to which the rest of the second is dropped (m20mod.c:1362)
#define M20_AUX_MAX   64
// the raw header m20mod hands to find_softbinhead (m20mod.c:81), one character per symbol
static RSW_DEV unsigned long long m20_header_mask() {
    const char h[M20_HEADLEN + 1] = "10011001100110010100110010011001";
    unsigned long long m = 0;
    for (int i = 0; i < M20_HEADLEN; i++) m |= (unsigned long long)(h[i] & 1) << i;
    return m;
}

// a channel between calls (global memory)
struct SoftinM20Chan {
    int   mode;                    // 0 searching, 1 inside a frame, 2 dropping the rest of the second
    int   inv;                     // gpx.option.inv as the last header left it (irrelevant for the differential code, m20mod.c:1312-1314)
    int   mpos;                    // frame bits decided so far
    int   mhalf;                   // the first symbol of a pair is pending in ms1
    int   mbit0;                   // previous bit ('0' = 0x30 in front of the frame's first bit: the reference's quirk)
    int   mskip;                   // bitpos of the skip loop
    float ms1;
    float mv;                      // score of the header in front of the frame in progress
    unsigned long long bits_in, hdr_bit;
    float hist[M20_HEADLEN];       // hdb.sbuf: the last 32 symbols seen while searching, oldest first
    char  mbits[M20_NBITS + 8];    // gpx.frame_bits of the frame in progress
};
// LDS of a wave besides the staged soft decisions: 128 + 1328 + 172 = 1628 B
struct SoftinM20Lds {
    float hist[M20_HEADLEN];
    char  mb[M20_NBITS + 8];
    unsigned char fr[172];
};

static RSW_DEV int mxx_cs_step(int c, unsigned char b) {          // one byte of checkM10 (m20mod.c:562-596)
    b = (unsigned char)((b >> 1) | ((b & 1) << 7));
    b ^= (b >> 2) & 0xFF;
    const int t6 = (c & 1) ^ ((c >> 2) & 1) ^ ((c >> 4) & 1), t7 = ((c >> 1) & 1) ^ ((c >> 3) & 1) ^ ((c >> 5) & 1);
    const int t = (c & 0x3F) | (t6 << 6) | (t7 << 7);
    int sreg = (c >> 7) & 0xFF;
    sreg ^= (sreg >> 2) & 0xFF;
    return (((c & 0xFF) << 8) | ((b ^ t ^ sreg) & 0xFF)) & 0xFFFF;
}

// what print_frame() derives from the 165 bytes in fr (m20mod.c:875-907) -> *o; lane 0: length, firmware byte, frame checksum; lane 1: block checksum.
// A length byte of 0 follows the host rule (sonde_frame.cpp sonde_m20_frame_finish): nothing summed, cs_calc 0, cs_ok 1.
static RSW_DEV void m20_wave_verdicts(const unsigned char *fr, sonde_m20_frame_t *o, const int lane) {
    if (lane == 0) {
        int flen = fr[0], pos_fw = 0x43;
        if (flen < 0x45) pos_fw = flen - 2;
        else if (flen - 0x45 > M20_AUX_MAX) flen = 0x45 + M20_AUX_MAX;
        const int pc = flen - 1;
        int fw = pos_fw >= 0 ? fr[pos_fw] : 0;
        if (fw > 0x20) fw = 0;
        int c = 0;
        for (int i = 0; i < pc; i++) c = mxx_cs_step(c, fr[i]);
        o->len = flen + 1; o->fw = fw; o->cs_calc = (uint32_t)c;
        o->cs_ok = pc >= 0 ? ((uint32_t)((fr[pc] << 8) | fr[pc + 1]) == (uint32_t)c) : 1;
    }
    if (lane == 1) {
        int c = mxx_cs_step(0, 0x16);                                 // blk_checkM10(0x16, frame + 2): the length byte, then 0x14 bytes of the block
        for (int i = 0; i < 0x14; i++) c = mxx_cs_step(c, fr[2 + i]);
        const int bc1 = (fr[0x16] << 8) | fr[0x17];
        o->blk_ok = bc1 == c ? 1 : bc1 == 0 ? -1 : 0;
    }
}

// One channel, one call: nb symbols at x (sgn = -1: --softinv).  doskip: verbosity below 3 (m20mod.c:1361).  s_x: room for stage_cap staged symbols (LDS);
// a call of more reads x where it lies.  Completed frames go to out[slot], slot from *count; a slot at or beyond cap is counted, not written.
static RSW_DEV void m20_wave_channel(SoftinM20Chan *st, const float *x, const int nb, const float sgn, const float ths, const int doskip, SoftinM20Lds *L,
                                     float *s_x, const int stage_cap, sonde_m20_frame_t *out, unsigned *count, const int cap, const int ch, const int lane) {
    int mode = st->mode, inv = st->inv, mpos = st->mpos, mhalf = st->mhalf, mbit0 = st->mbit0, mskip = st->mskip;
    float ms1 = st->ms1, mv_hdr = st->mv; unsigned long long hdr_bit = st->hdr_bit; const unsigned long long bits0 = st->bits_in;
    if (mpos < 0 || mpos > M20_NBITS || nb < 0) return;                          // (never: the host zeroes the state)
    if (lane < M20_HEADLEN) L->hist[lane] = st->hist[lane];
    if (mode == 1) for (int i = lane; i < mpos; i += 64) L->mb[i] = st->mbits[i];
    const SoftinX X = softin_wave_stage(s_x, x, sgn, nb, stage_cap, lane);                        // symbol p of this call, --softinv applied
    rsw_wave_sync();
    const unsigned long long hbits = m20_header_mask();
    int cur = 0;
    while (cur < nb) {
        if (mode == 0) {
            // element k of hist ++ the call's symbols from `cur`
            const int cur0 = cur;
            auto W = [&](const int k) -> float { return k < M20_HEADLEN ? L->hist[k] : X(cur0 + (k - M20_HEADLEN)); };
            bool found = false;
            for (int base = cur0; base < nb && !found; base += 64) {
                const int q = base + lane;
                float mv = 0.f;
                if (q < nb) mv = softin_wave_score<M20_HEADLEN>(W, q - cur0 + 1, hbits, ths);      // the window of position q ends with the symbol at q
                const unsigned long long hits = rsw_ballot(q < nb && fabsf(mv) > ths);
                if (hits) {
                    const int l = __builtin_ctzll(hits), qs = base + l;
                    const float mvl = mxxw_bcast_f(mv, l);
                    if ((double)mvl * (0.5 - inv) < 0) inv ^= 1;
                    softin_wave_ring<M20_HEADLEN>(L->hist, W, qs - cur0 + 1, lane);                // the ring as the header leaves it: the 32 elements up to the hit
                    found = true;
                    mode = 1; mpos = 0; mhalf = 0; mbit0 = '0'; mv_hdr = mvl; hdr_bit = bits0 + (unsigned long long)qs + 1ull;
                    cur = qs + 1;
                }
            }
            if (!found) {
                softin_wave_ring<M20_HEADLEN>(L->hist, W, nb - cur0, lane);                        // the 32 elements up to the call's last symbol
                cur = nb;
            }
        } else if (mode == 1) {
            // two symbols a bit (the first of a pair may be left over from the last call): bit = (s2 - s1) >= 0, out = 0x31 ^ (previous ^ bit)
            const int need = M20_NBITS - mpos, left = 2 * need - mhalf, take = nb - cur < left ? nb - cur : left, nbits = (mhalf + take) / 2;
            int last_bit = mbit0;
            for (int j0 = 0; j0 < nbits; j0 += 64) {
                const int j = j0 + lane;
                int bit = 0;
                if (j < nbits) {
                    const int p1 = cur + 2 * j - mhalf, p2 = p1 + 1;
                    const float s1 = (j == 0 && mhalf) ? ms1 : X(p1), s2 = X(p2);
                    bit = (s2 - s1) >= 0.0f;
                }
                int prev = rsw_shfl_up(bit, 1, lane);
                if (lane == 0) prev = last_bit;
                if (j < nbits) L->mb[mpos + j] = (char)(0x31 ^ (prev ^ bit));
                const int cnt = nbits - j0 < 64 ? nbits - j0 : 64;
                last_bit = rsw_bcast(bit, cnt - 1);
            }
            if (nbits > 0) mbit0 = last_bit;
            if ((mhalf + take) & 1) { ms1 = X(cur + take - 1); mhalf = 1; } else mhalf = 0;
            mpos += nbits; cur += take;
            if (mpos == M20_NBITS) {
                rsw_wave_sync();
                const unsigned slot = softin_wave_slot(count, lane);
                for (int i = lane; i < 172; i += 64) {                    // bits2bytes (m20mod.c:192-220): big endian, anything but '1' counts as 0
                    unsigned v = 0;
                    if (i < M20_NBYTES) for (int k = 0; k < 8; k++) if (L->mb[8 * i + 7 - k] == '1') v |= 1u << k;
                    L->fr[i] = (unsigned char)v;
                }
                rsw_wave_sync();
                if ((int)slot < cap && (int)slot >= 0) {
                    sonde_m20_frame_t *o = out + slot;
                    for (int i = lane; i < 172; i += 64) o->frame[i] = L->fr[i];
                    m20_wave_verdicts(L->fr, o, lane);
                    if (lane == 2) { o->channel = ch; o->nbits = M20_NBITS; o->mv = mv_hdr; o->mv_pos = (uint32_t)hdr_bit; }
                }
                rsw_wave_sync();
                mskip = M20_NBITS;
                mode = doskip ? 2 : 0;
            }
        } else {
            // the rest of the second: one symbol per counted bit (m20mod.c:1361-1373)
            const int left = M20_SKIP_END - mskip, take = nb - cur < left ? nb - cur : left;
            mskip += take; cur += take;
            if (mskip >= M20_SKIP_END) mode = 0;
        }
    }
    rsw_wave_sync();
    if (lane < M20_HEADLEN) st->hist[lane] = L->hist[lane];
    if (mode == 1) for (int i = lane; i < mpos; i += 64) st->mbits[i] = L->mb[i];
    if (lane == 0) {
        st->mode = mode; st->inv = inv; st->mpos = mpos; st->mhalf = mhalf; st->mbit0 = mbit0; st->mskip = mskip; st->ms1 = ms1; st->mv = mv_hdr;
        st->hdr_bit = hdr_bit; st->bits_in = bits0 + (unsigned long long)nb;
    }
}
#endif
