// sonde_family_hits_dev.h — the block codes of a GENERIC engine's header hits on the device, ONE wavefront per hit record: what FamilyDecoder.hit ->
// sonde_<kind>_dec_frame does per frame on one host thread (BCH(63,51), Hamming(8,4) + check sums, CRC-16, RS(255,231)) for the four kinds whose hit is decoded
// without per-channel state.  The hit is complete in memory — nbits soft bits behind the header, in the polarity the engine stores — so there is no header search,
// no mode and no carry: per kind the bit stage of the SAMPLE form (sonde_<kind>_dec_frame) into the LDS struct of the kind's soft-bit consumer, then that consumer's
// end-of-frame routine unchanged.
//   Meisei  1152 half symbols: bit j = 1 if half symbols 2 j and 2 j + 1 have the same hard value (biphase-S), 576 bits in nine rounds of 64, each round's ballot
//           ORed into SoftinMeiseiLds::w behind MEISEI_HDR24 -> meisei_wave_end (--ecc) -> 75 bytes MSB first, 12 block verdicts, err_frm, err_blks
//   iMet-54 2200 symbols: softin_wave_8n1 into chr[220], polarity already applied by the engine -> imet54_wave_end -> 108 bytes, three ecc sums, both check sums
//   MTS01   1048 bits read raw: the engine flipped them when the header score is negative, so they are flipped back (FamilyDecoder.hit, pol = "raw"); ballots into
//           SoftinMts01Lds::w -> mts01_wave_end -> 131 bytes MSB first, crcval, crcdat, crc_ok
//   RS92    2340 bits, one per Manchester pair, 10 per byte: bits 1 .. 8 LSB first on a lane per byte into frame[240] behind 2A 2A 2A 2A 2A 10 -> rs92_wave_ecc
//           (GF tables in LDS) -> 240 bytes, rs_decode's value
// The bit rule is the reference's everywhere: s >= 0 is a 1, so -0.0 is a 1.  A record with fewer valid bits than the kind's frame (end of input) is not decoded:
// decoded = 0, everything behind the head of the record zero; its soft bits stay in the ring for the host.
//
// family_wave_records is the loop of k_family_hits: records [start, end) of the ring, record i on workgroup i % grid, slot i % max_frames; every byte of a record
// is written exactly once, by one lane.  family_wave_ticket is the {done, ticket} hand-over of k_dfm_hits.
//
// Compiled twice, like the sonde_softin_*_dev.h headers: by hipcc into k_family_hits<kind> (sonde_family_hits.hip) and by g++ under tests/emu/wave_emu.h
// (tests/emu/family_hits_emu.cpp).  Control flow around every cross-lane primitive is wave-uniform.
#ifndef SONDE_FAMILY_HITS_DEV_H
#define SONDE_FAMILY_HITS_DEV_H
#include "sonde_softin_wave_dev.h"
#include "sonde_softin_meisei_dev.h"
#include "sonde_softin_imet54_dev.h"
#include "sonde_softin_mts01_dev.h"
#include "sonde_softin_rs92_dev.h"
// (no contraction: the reference is plain C on x86-64 — every product and sum rounded on its own)
#pragma clang fp contract(off)

#define FAMILY_RS92_BITS   2340                                        // one soft bit per Manchester pair: 234 bytes of 10
#define FAMILY_RS92_BYTEBITS 10
#define FAMILY_DATA        240                                         // sonde_family_hit_t.data
#define FAMILY_AUX         12
#define FAMILY_V           6

// soft bits a complete hit of `kind` holds (family.FAMILY's nbits); 0: not a kind of this decoder
static inline int family_kind_bits(const int kind) {
    return kind == SONDE_MEISEI ? MEISEI_NSYM : kind == SONDE_IMET54 ? IMET54_NSYM : kind == SONDE_MTS01 ? MTS01_NBITS : kind == SONDE_RS92 ? FAMILY_RS92_BITS : 0;
}
static inline int family_kind_symlen(const int kind) { return kind == SONDE_RS92 ? 2 : 1; }

// what a record says about its hit before anything is decoded
struct FamilyHitIn { int32_t channel, nv; uint32_t mv_pos; float mv; };      // nv: valid soft bits of the hit
// what does not change from record to record
struct FamilyArgs {
    const float *soft; long long stride;           // soft bits of ring slot s at soft + s * stride
    int ecc, max_frames;
    const uint32_t *tab;                           // iMet-54: imet54_crc_table's words
    const uint8_t *gf;                             // RS92: exp[512] ++ log[256]
    sonde_family_hit_t *out;                       // [max_frames]
};

// the head of a record and its v[]: lane 0 .. 5 hold v[lane] in `val`
static RSW_DEV void family_wave_head(sonde_family_hit_t *o, const FamilyHitIn &h, const int kind, const int decoded, const int val, const int lane) {
    if (lane < FAMILY_V) o->v[lane] = val;
    if (lane == 0) { o->channel = h.channel; o->kind = kind; o->nbits = h.nv; o->decoded = decoded; o->mv_pos = h.mv_pos; o->mv = h.mv; }
}
// a hit shorter than a frame: marked, nothing else
static RSW_DEV void family_wave_short(sonde_family_hit_t *o, const FamilyHitIn &h, const int kind, const int lane) {
    family_wave_head(o, h, kind, 0, 0, lane);
    if (lane < FAMILY_AUX) o->aux[lane] = 0;
    for (int k = lane; k < FAMILY_DATA; k += 64) o->data[k] = 0;
}
// 64 bits of a round, bit l from lane l, ORed into the bit words at frame bit f0 (up to three words; nwords of them exist)
static RSW_DEV void family_wave_or64(uint32_t *w, const int nwords, const unsigned long long m, const int f0, const int lane) {
    const int sh = f0 & 31, idx = (f0 >> 5) + lane;
    if (lane < 3 && idx < nwords) {
        const uint32_t v = lane == 0 ? (uint32_t)(m << sh) : lane == 1 ? (uint32_t)(m >> (32 - sh)) : sh ? (uint32_t)(m >> (64 - sh)) : 0u;
        w[idx] |= v;
    }
    rsw_wave_sync();
}

// ---- Meisei: sonde_meisei_dec_frame's bit stage (frame(): the 24 header bits, then biphase-S), meisei_wave_end
struct FamilyMeisei {
    typedef SoftinMeiseiLds Lds;
    static constexpr int KIND = SONDE_MEISEI, NB = MEISEI_NSYM;
    static RSW_DEV void stage(const FamilyArgs &, Lds *, const int) {}
    static RSW_DEV void hit(const FamilyArgs &a, const FamilyHitIn &h, const float *sb, Lds *L, sonde_family_hit_t *o, const int lane) {
        if (lane < MEISEI_WORDS) L->w[lane] = lane == 0 ? MEISEI_HDR24 : 0u;
        rsw_wave_sync();
        for (int r0 = 0; r0 < MEISEI_NSYM / 2; r0 += 64) {             // 576 = 9 x 64: every lane has a bit in every round
            const int j = r0 + lane;
            const bool b = (sb[2 * j] >= 0.0f) == (sb[2 * j + 1] >= 0.0f);                         // biphase-S: equal halves are a 1
            family_wave_or64(L->w, MEISEI_WORDS, rsw_ballot(b), MEISEI_HDRBITS + r0, lane);
        }
        const unsigned long long be = a.ecc ? meisei_wave_end(L, lane) : 0ull;
        rsw_wave_sync();
        int err_frm = 0, err_blks = 0;                                 // what the frame loop counts over both subframes (meisei100mod.c:735-776)
        for (int k = 0; k < MEISEI_BLOCKS; k++) { const int e = (int)((be >> (4 * k)) & 0xF); err_frm += e >= 0xE; err_blks += e != 0; }
        family_wave_head(o, h, KIND, 1, lane == 0 ? err_frm : lane == 1 ? err_blks : 0, lane);
        if (lane < FAMILY_AUX) o->aux[lane] = (uint8_t)((be >> (4 * lane)) & 0xF);
        for (int k = lane; k < FAMILY_DATA; k += 64) {
            uint32_t rv = 0;
            if (k < MEISEI_NBYTES) {
                const uint32_t by = (L->w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
                for (int i = 0; i < 8; i++) rv |= ((by >> i) & 1u) << (7 - i);                     // MSB first
            }
            o->data[k] = (uint8_t)rv;
        }
    }
};

// ---- iMet-54: sonde_imet54_dec_frame's bit stage (bit = s >= 0, de8n1), imet54_wave_end
struct FamilyImet54 {
    typedef SoftinImet54Lds Lds;
    static constexpr int KIND = SONDE_IMET54, NB = IMET54_NSYM;
    static RSW_DEV void stage(const FamilyArgs &, Lds *, const int) {}
    static RSW_DEV void hit(const FamilyArgs &a, const FamilyHitIn &h, const float *sb, Lds *L, sonde_family_hit_t *o, const int lane) {
        auto S = [&](const int k) -> float { return sb[k]; };
        softin_wave_8n1(S, IMET54_CHARS, 0, L->chr, lane);
        rsw_wave_sync();
        const Imet54Verdict v = imet54_wave_end(L, a.ecc, a.tab, lane);
        rsw_wave_sync();
        family_wave_head(o, h, KIND, 1, lane == 0 ? v.ecc_frm : lane == 1 ? v.ecc_tlm : lane == 2 ? v.ecc_std : lane == 3 ? v.crc_std : lane == 4 ? v.crc_cont : 0, lane);
        if (lane < FAMILY_AUX) o->aux[lane] = 0;
        for (int k = lane; k < FAMILY_DATA; k += 64) o->data[k] = k < IMET54_FRAME ? L->fr[k] : (uint8_t)0;
    }
};

// ---- MTS01: FamilyDecoder.hit's un-flip for pol = "raw", sonde_mts01_dec_frame's bit stage (bit = s >= 0, bytes MSB first), mts01_wave_end
struct FamilyMts01 {
    typedef SoftinMts01Lds Lds;
    static constexpr int KIND = SONDE_MTS01, NB = MTS01_NBITS;
    static RSW_DEV void stage(const FamilyArgs &, Lds *, const int) {}
    static RSW_DEV void hit(const FamilyArgs &a, const FamilyHitIn &h, const float *sb, Lds *L, sonde_family_hit_t *o, const int lane) {
        (void)a;
        const bool flip = h.mv < 0.f;
        if (lane < MTS01_WORDS) L->w[lane] = 0u;
        rsw_wave_sync();
        for (int r0 = 0; r0 < MTS01_NBITS; r0 += 64) {
            const int j = r0 + lane;
            bool b = false;
            if (j < MTS01_NBITS) { const float s = flip ? -sb[j] : sb[j]; b = s >= 0.0f; }
            family_wave_or64(L->w, MTS01_WORDS, rsw_ballot(b), r0, lane);
        }
        const Mts01Verdict v = mts01_wave_end(L, lane);
        rsw_wave_sync();
        family_wave_head(o, h, KIND, 1, lane == 0 ? (int)v.crcval : lane == 1 ? (int)v.crcdat : lane == 2 ? v.crc_ok : 0, lane);
        if (lane < FAMILY_AUX) o->aux[lane] = 0;
        for (int k = lane; k < FAMILY_DATA; k += 64) o->data[k] = k < MTS01_NBYTES ? L->by[k] : (uint8_t)0;
    }
};

// ---- RS92: sonde_rs92_dec_frame's bit stage (10 bits a byte, bits 1 .. 8 LSB first, the header bytes in front), rs92_wave_ecc
struct FamilyRs92 {
    typedef SoftinRs92Lds Lds;
    static constexpr int KIND = SONDE_RS92, NB = FAMILY_RS92_BITS;
    // the GF tables, once per workgroup: they do not change from record to record
    static RSW_DEV void stage(const FamilyArgs &a, Lds *L, const int lane) {
        for (int i = lane; i < 512; i += 64) L->gexp[i] = a.gf[i];
        for (int i = lane; i < 256; i += 64) L->glog[i] = a.gf[512 + i];
        rsw_wave_sync();
    }
    static RSW_DEV void hit(const FamilyArgs &a, const FamilyHitIn &h, const float *sb, Lds *L, sonde_family_hit_t *o, const int lane) {
        (void)a;
        if (lane < RS92_FRAMESTART) L->frame[lane] = lane < 5 ? 0x2A : 0x10;
        for (int j = lane; j < RS92_FRAME_LEN - RS92_FRAMESTART; j += 64) {
            unsigned byte = 0;
            for (int b = 1; b <= 8; b++) byte |= (unsigned)(sb[FAMILY_RS92_BYTEBITS * j + b] >= 0.0f ? 1 : 0) << (b - 1);
            L->frame[RS92_FRAMESTART + j] = (uint8_t)byte;
        }
        rsw_wave_sync();
        const int ec = rs92_wave_ecc(L, lane);
        family_wave_head(o, h, KIND, 1, lane == 0 ? ec : 0, lane);
        if (lane < FAMILY_AUX) o->aux[lane] = 0;
        for (int k = lane; k < FAMILY_DATA; k += 64) o->data[k] = L->frame[k];
    }
};

// records [start, end) of the ring on workgroup `block` of `grid`: record i by workgroup i % grid into slot i % max_frames.  rec(slot) -> FamilyHitIn.
template <class K, class RF>
static RSW_DEV void family_wave_records(const FamilyArgs &a, const RF &rec, unsigned start, const unsigned end, const int block, const int grid, typename K::Lds *L,
                                        const int lane) {
    if ((int)(end - start) > a.max_frames) start = end - (unsigned)a.max_frames;                   // (what the ring no longer holds)
    if ((int)(end - (start + (unsigned)block)) > 0) K::stage(a, L, lane);                          // (tables that do not change from record to record)
    for (unsigned i = start + (unsigned)block; (int)(end - i) > 0; i += (unsigned)grid) {
        const unsigned slot = i % (unsigned)a.max_frames;
        const FamilyHitIn h = rec(slot);
        sonde_family_hit_t *o = a.out + slot;
        if (h.nv >= K::NB) K::hit(a, h, a.soft + (size_t)slot * a.stride, L, o, lane);
        else family_wave_short(o, h, K::KIND, lane);
        rsw_wave_sync();                                               // the LDS of this record is not touched by the next before every lane is through
    }
}
// the last workgroup to finish moves *done up to `end` (done[1] is its ticket counter); the caller has made its records visible
static RSW_DEV void family_wave_ticket(unsigned *done, const unsigned end, const int grid, const int lane) {
    if (lane == 0 && mxxw_atomic_inc(&done[1]) == (unsigned)grid - 1u) { done[1] = 0; done[0] = end; }
}
#endif
