// sonde_lms6_hits_dev.h — the LMS6-403 / LMS-X (lms6Xmod) hits of a GENERIC engine on the device, ONE wavefront per hit record: what FamilyDecoder.hit ->
// sonde_lms6_dec_block does per hit on one host thread up to block_bytes (the raw-bit sign alternation, the K = 7 Viterbi decoder, deconv, bits2bytes), without
// the channel's state.  What follows block_bytes — RS(255,223), frame sync, CRC, auto detection, text — stays with the channel's host decoder
// (sonde_lms6_dec_block_bytes), which sees the records in order.
//
//   bits:    an engine has one description, so one block length: nb = 4096 (LMS6) or 4720 (LMS-X) soft bits behind the header.  The engine stores them in the
//            polarity in effect; the decoder wants them raw, so they are flipped back when the header score is negative (FamilyDecoder.hit, pol = "raw").  Then
//            put_bit (lms6Xmod.c:1393-1421): s = mv < 0 ? -x[j] : x[j], bc = mv > 0 ? 0 : 1, odd = (bc + j) & 1, hb = (s >= 0) ^ odd, sb = odd ? -s : s, with
//            --vit (vit = 1) sb = 2 hb - 1, into Lms6Lds::sb[80 + j] behind the 80 sync positions.  The negations are negations: -0.0 stays a 1 under >= 0.
//   decode:  lms6_wave_decode of the soft-bit consumer (sonde_vit_dev.h), unchanged, over 80 + nb positions, its bytes straight into the record.
//   record:  sonde_lms6_hit_t, every byte written exactly once, by one lane: len = 80 + nb, blen, err = deconv's error index, vit, bytes[308] zero behind blen.
// A record with fewer than nb valid bits (end of input) is not decoded: decoded = 0, everything behind mv zero; its soft bits stay in the ring for the host.
//
// lms6_wave_records is the loop of k_lms6_hits (sonde_lms6_hits.hip), with the slot, ring and ticket rules of family_wave_records (sonde_family_hits_dev.h): records
// [start, end) of the ring, record i on workgroup i % grid, slot i % max_frames; family_wave_ticket hands over.
//
// Compiled twice, like sonde_mrz_hits_dev.h: by hipcc into k_lms6_hits and by g++ under tests/emu/wave_emu.h (tests/emu/lms6_hits_emu.cpp).  Control flow around
// every cross-lane primitive is wave-uniform.
#ifndef SONDE_LMS6_HITS_DEV_H
#define SONDE_LMS6_HITS_DEV_H
#include "sonde_vit_dev.h"                                             // Lms6Lds, lms6_sync_sb, lms6_wave_decode
#include "sonde_family_hits_dev.h"                                     // FamilyHitIn, family_wave_ticket
// (no contraction: the reference is plain C on x86-64 — every product and sum rounded on its own)
#pragma clang fp contract(off)

#define LMS6_HIT_BITS6 (LMS6_RAWBLK6 - LMS6_BLOCKSTART)                // 4096: soft bits of a complete hit, family.FAMILY["LMS6"]'s nbits
#define LMS6_HIT_BITSX (LMS6_RAWBLKX - LMS6_BLOCKSTART)                // 4720: family.FAMILY["LMSX"]'s

// what does not change from record to record
struct Lms6HitsArgs {
    const float *soft; long long stride;           // soft bits of ring slot s at soft + s * stride
    int vit, nb, max_frames;                       // 1 = --vit, 2 = --vit2; nb = LMS6_HIT_BITS6 or LMS6_HIT_BITSX (the callers have checked both)
    sonde_lms6_hit_t *out;                         // [max_frames]
};

// the head of a record, by lane 0
static RSW_DEV void lms6_wave_head(sonde_lms6_hit_t *o, const FamilyHitIn &h, const int decoded, const int len, const int blen, const int err, const int vit,
                                   const int lane) {
    if (lane == 0) {
        o->channel = h.channel; o->kind = SONDE_LMS6; o->nbits = h.nv; o->decoded = decoded; o->mv_pos = h.mv_pos; o->mv = h.mv;
        o->len = len; o->blen = blen; o->err = err; o->vit = vit;
    }
}
// a hit shorter than a block: marked, nothing else
static RSW_DEV void lms6_wave_short(sonde_lms6_hit_t *o, const FamilyHitIn &h, const int lane) {
    lms6_wave_head(o, h, 0, 0, 0, 0, 0, lane);
    for (int k = lane; k < LMS6_BB_LEN; k += 64) o->bytes[k] = 0;
}

// one complete hit: h, x[0 .. nb) -> *o
static RSW_DEV void lms6_wave_hit(const int vit, const int nb, const FamilyHitIn &h, const float *x, Lms6Lds *L, sonde_lms6_hit_t *o, const int lane) {
    const bool flip = h.mv < 0.f;
    const unsigned bc = h.mv > 0.f ? 0u : 1u;
    for (int i = lane; i < LMS6_BLOCKSTART; i += 64) L->sb[i] = lms6_sync_sb(i);
    for (int j = lane; j < nb; j += 64) {
        const float s = flip ? -x[j] : x[j];
        const unsigned odd = (bc + (unsigned)j) & 1u;
        const int hb = (s >= 0.0f) ^ (int)odd;                         // (c0, inv(c1))
        float sb = odd ? -s : s;
        if (vit == 1) sb = (float)(2 * hb - 1);
        L->sb[LMS6_BLOCKSTART + j] = sb;
    }
    rsw_wave_sync();
    int err = 0;
    const int blen = lms6_wave_decode(L, LMS6_BLOCKSTART + nb, o->bytes, &err, lane);
    lms6_wave_head(o, h, 1, LMS6_BLOCKSTART + nb, blen, err, vit, lane);
}

// the loop of k_lms6_hits; rec(slot) -> FamilyHitIn
template <class RF>
static RSW_DEV void lms6_wave_records(const Lms6HitsArgs &a, const RF &rec, unsigned start, const unsigned end, const int block, const int grid, Lms6Lds *L,
                                      const int lane) {
    if ((int)(end - start) > a.max_frames) start = end - (unsigned)a.max_frames;                   // (what the ring no longer holds)
    for (unsigned i = start + (unsigned)block; (int)(end - i) > 0; i += (unsigned)grid) {
        const unsigned slot = i % (unsigned)a.max_frames;
        const FamilyHitIn h = rec(slot);
        sonde_lms6_hit_t *o = a.out + slot;
        if (h.nv >= a.nb) lms6_wave_hit(a.vit, a.nb, h, a.soft + (size_t)slot * a.stride, L, o, lane);
        else lms6_wave_short(o, h, lane);
        rsw_wave_sync();                                               // the LDS of this record is not touched by the next before every lane is through
    }
}
#endif
