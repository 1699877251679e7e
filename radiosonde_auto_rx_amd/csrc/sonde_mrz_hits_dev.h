// sonde_mrz_hits_dev.h — the MRZ (Meteo-Radiy MP3-H1, mp3h1mod) hits of a GENERIC engine on the device, ONE wavefront per hit record: what FamilyDecoder.hit ->
// sonde_mrz_dec_frame does per hit on one host thread (bits, bytes from bit --ofs on, the frame type, CRC-16), without the channel's state.
// The host decoder reads min(386, frame length in effect - 22) soft bits of a hit: 386 for the ECEF frame (408 bits with the 22 header bits), 362 for the lat / lon
// frame (384 bits), and which of the two depends on the CRC verdict of the channel's previous frames.  bits2bytes zero-fills the frame bytes behind the length in
// effect, so the verdict is a function of (bits, length, bits_ofs) alone: the device computes it under BOTH lengths and the channel's host decoder, which sees the
// records in order anyway, takes the one that matches its state when it prints (sonde_mrz_dec_decoded with 408 / v[0] or 384 / v[1]).
//
//   bits:    the engine always slices 386 soft bits behind the header.  Bit j = !(s >= 0) on a lane per bit — the engine's bits carry the polarity and Manchester1
//            is the other sense (sonde_mrz_dec_frame), so -0.0 gives a 0 and a NaN a 1 — in rounds of 64, each round's ballot ORed into SoftinMrzLds::w behind
//            MRZ_HDR22.
//   verdict: mrz_wave_end of the soft-bit consumer (sonde_softin_mrz_dev.h), unchanged, with 384 bits and then with 408: it never reads a bit at or behind the
//            length it is given, so the 24 bits behind a lat / lon frame do not enter its verdict.  crclen comes from bytes 30 / 31, which lie inside both lengths
//            for every --ofs (0 .. 64).
//   record:  sonde_family_hit_t, every byte written exactly once, by one lane: v = {crc_ok at 408, crc_ok at 384, crclen, crcval408 | crcval384 << 16,
//            crcdat408 | crcdat384 << 16, bits_ofs}, aux zero, data[0 .. 50] the 408 frame bits from the header's first, MSB first, the rest zero.
// A record with fewer than 386 valid bits (end of input; 362 .. 385 included) is family_wave_short: decoded = 0, its soft bits stay in the ring for the host.
//
// mrz_wave_records is the loop of k_mrz_hits (sonde_mrz_hits.hip), with the slot, ring and ticket rules of family_wave_records (sonde_family_hits_dev.h): records
// [start, end) of the ring, record i on workgroup i % grid, slot i % max_frames; family_wave_ticket hands over.
//
// Compiled twice, like sonde_family_hits_dev.h: by hipcc into k_mrz_hits and by g++ under tests/emu/wave_emu.h (tests/emu/mrz_hits_emu.cpp).  Control flow around
// every cross-lane primitive is wave-uniform.
#ifndef SONDE_MRZ_HITS_DEV_H
#define SONDE_MRZ_HITS_DEV_H
#include "sonde_softin_mrz_dev.h"                                      // SoftinMrzLds, MRZ_HDR22, mrz_wave_end
#include "sonde_family_hits_dev.h"                                     // FamilyHitIn, family_wave_head / _short / _or64 / _ticket

#define MRZ_HIT_BITS    (MRZ_MAXBITS - MRZ_HDRBITS)                    // 386: soft bits of a complete hit (family.FAMILY["MRZ"]'s nbits)
#define MRZ_LATLON_BITS ((MRZ_CRCLEN_LATLON + 6) * 8)                  // 384: the lat / lon frame from the header's first bit

// what does not change from record to record
struct MrzHitsArgs {
    const float *soft; long long stride;           // soft bits of ring slot s at soft + s * stride
    int bits_ofs, max_frames;                      // --ofs: 0 .. 64 (the callers have checked)
    sonde_family_hit_t *out;                       // [max_frames]
};

// one complete hit: h, sb[0 .. 385] -> *o
static RSW_DEV void mrz_wave_hit(const int bits_ofs, const FamilyHitIn &h, const float *sb, SoftinMrzLds *L, sonde_family_hit_t *o, const int lane) {
    if (lane < MRZ_WORDS) L->w[lane] = lane == 0 ? MRZ_HDR22 : 0u;
    rsw_wave_sync();
    for (int r0 = 0; r0 < MRZ_HIT_BITS; r0 += 64) {                    // 386 = 6 x 64 + 2
        const int j = r0 + lane;
        bool b = false;
        if (j < MRZ_HIT_BITS) b = !(sb[j] >= 0.0f);
        family_wave_or64(L->w, MRZ_WORDS, rsw_ballot(b), MRZ_HDRBITS + r0, lane);
    }
    const MrzVerdict s = mrz_wave_end(L, MRZ_LATLON_BITS, bits_ofs, lane);
    rsw_wave_sync();                                                   // (the second look rewrites L->by: every lane is through with the first)
    const MrzVerdict e = mrz_wave_end(L, MRZ_MAXBITS, bits_ofs, lane);
    rsw_wave_sync();
    const int val = lane == 0 ? e.crc_ok : lane == 1 ? s.crc_ok : lane == 2 ? e.crclen : lane == 3 ? (int)(e.crcval | s.crcval << 16)
                  : lane == 4 ? (int)(e.crcdat | s.crcdat << 16) : bits_ofs;
    family_wave_head(o, h, SONDE_MRZ, 1, val, lane);
    if (lane < FAMILY_AUX) o->aux[lane] = 0;
    for (int k = lane; k < FAMILY_DATA; k += 64) {
        uint32_t rv = 0;
        if (k < MRZ_FRAME) {
            const uint32_t by = (L->w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
            for (int i = 0; i < 8; i++) rv |= ((by >> i) & 1u) << (7 - i);                         // MSB first
        }
        o->data[k] = (uint8_t)rv;
    }
}

// the loop of k_mrz_hits; rec(slot) -> FamilyHitIn
template <class RF>
static RSW_DEV void mrz_wave_records(const MrzHitsArgs &a, const RF &rec, unsigned start, const unsigned end, const int block, const int grid, SoftinMrzLds *L,
                                     const int lane) {
    if ((int)(end - start) > a.max_frames) start = end - (unsigned)a.max_frames;                   // (what the ring no longer holds)
    for (unsigned i = start + (unsigned)block; (int)(end - i) > 0; i += (unsigned)grid) {
        const unsigned slot = i % (unsigned)a.max_frames;
        const FamilyHitIn h = rec(slot);
        sonde_family_hit_t *o = a.out + slot;
        if (h.nv >= MRZ_HIT_BITS) mrz_wave_hit(a.bits_ofs, h, a.soft + (size_t)slot * a.stride, L, o, lane);
        else family_wave_short(o, h, SONDE_MRZ, lane);
        rsw_wave_sync();                                               // the LDS of this record is not touched by the next before every lane is through
    }
}
#endif
