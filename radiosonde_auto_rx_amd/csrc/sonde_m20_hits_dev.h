// sonde_m20_hits_dev.h — the M20 hits of a base-rate (or mixed) engine on the device, ONE wavefront per hit record: what sonde_engine_fetch_m20 did per hit on one
// host thread (mxx_bytes(e, r, 101 + 64, ..) + sonde_m20_frame_finish, sonde_engine.cpp / sonde_frame.cpp), restated exactly.
// Behaviour reproduced (not code): demod/mod/m20mod.c main :1318-1354 (bit0 = '0' in front of the frame's first bit :1321, frame_bits[pos] = 0x31 ^ (bit0 ^ bit)
// :1348, the terminator :1353 behind the last bit, also of a frame the input cuts short), bits2bytes :192-220, print_frame :875-907, blk_checkM10 :548-560, checkM10 :562-596.
//
//   bits:       nv = min(valid bits of the hit, 1320) hard bits from the record, LSB first (M20 has no --chk3: the soft bits are not read)
//   characters: a lane per bit, the previous bit from the record itself; they go to the channel's PERSISTENT characters in device memory (gpx.frame_bits: zero at
//               create), then fb[nv] = 0 — a hit cut short by the end of input keeps the previous frame's characters behind the terminator
//   bytes:      all 165 of them from the characters, a lane per byte, big endian; anything but '1' counts as 0
//   verdicts:   m20_wave_verdicts of the soft-bit consumer (sonde_softin_mxx_dev.h), lane 0 the frame checksum, lane 1 the block checksum
//   record:     every byte of a sonde_m20_frame_t is written exactly once, by one lane (frame[165..171] = 0 included)
// m20_wave_records is the loop of k_m20_hits (sonde_m20_hits.hip): records [start, end) of the ring in order, a channel's by the ONE workgroup with
// channel % grid == block (the characters persist), slot i % max_frames.  m20_wave_ticket is the {done, ticket} hand-over of k_m10_hits.
//
// Compiled twice, like the sonde_softin_*_dev.h headers: by hipcc into k_m20_hits and by g++ under tests/emu/wave_emu.h (tests/emu/m20_hits_emu.cpp).  Control flow
// around every cross-lane primitive is wave-uniform.
#ifndef SONDE_M20_HITS_DEV_H
#define SONDE_M20_HITS_DEV_H
#include "sonde_softin_mxx_dev.h"                                      // M20_NBYTES, M20_NBITS, m20_wave_verdicts

#define M20_CHAN_CHARS (M20_NBITS + 8)                                 // characters of a channel: 165 * 8 and the terminator, a multiple of 8
#define M20_REC_BYTES  172                                             // sonde_m20_frame_t.frame

// what a record says about its hit: nv = valid bits (any value: clamped here), bits = the hard bits, 8 a byte, LSB first (165 bytes are readable)
struct M20HitIn { int32_t channel, nv; uint32_t mv_pos; float mv; const uint8_t *bits; };
// what does not change from record to record
struct M20HitsArgs {
    int n_channels, max_frames;
    char *chan_bits;                               // [n_channels][M20_CHAN_CHARS]
    sonde_m20_frame_t *out;                        // [max_frames]
};

// characters of a channel written by one lane of the wave, read by another one
#ifndef SONDE_RS_EMU
static RSW_DEV void m20h_chars_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); }
#else
static inline void m20h_chars_sync() { rsw_wave_sync(); }
#endif

// one hit: h -> *o; fb = the channel's characters, s_fr = M20_REC_BYTES bytes of LDS
static RSW_DEV void m20_wave_hit(const M20HitIn &h, char *fb, unsigned char *s_fr, sonde_m20_frame_t *o, const int lane) {
    const int nv = h.nv < 0 ? 0 : h.nv < M20_NBITS ? h.nv : M20_NBITS;
    for (int p = lane; p < nv; p += 64) {
        // differential decoding: 1 = same as the previous bit; the first against '0' = 0x30, which gives a character that is neither '0' nor '1' (m20mod.c:1321,1348)
        const int bit = (h.bits[p >> 3] >> (p & 7)) & 1, prev = p == 0 ? 0x30 : (h.bits[(p - 1) >> 3] >> ((p - 1) & 7)) & 1;
        fb[p] = (char)(0x31 ^ (prev ^ bit));
    }
    if (lane == 0) fb[nv] = 0;
    m20h_chars_sync();
    for (int k = lane; k < M20_REC_BYTES; k += 64) {
        unsigned v = 0;
        if (k < M20_NBYTES) for (int q = 0; q < 8; q++) if (fb[8 * k + 7 - q] == '1') v |= 1u << q;       // bits2bytes, big endian
        s_fr[k] = (unsigned char)v;
    }
    rsw_wave_sync();
    for (int k = lane; k < M20_REC_BYTES; k += 64) o->frame[k] = s_fr[k];
    m20_wave_verdicts(s_fr, o, lane);                                  // lane 0: len, fw, cs_calc, cs_ok; lane 1: blk_ok
    if (lane == 2) { o->channel = h.channel; o->nbits = nv; o->mv = h.mv; o->mv_pos = h.mv_pos; }      // (positions relative to the channel's start: the host, which knows it)
    m20h_chars_sync();                                                 // the next record of the channel reads these characters, and writes s_fr
}

// the loop of k_m20_hits; rec(i % max_frames) = the hit of counter value i
template <class RF>
static RSW_DEV void m20_wave_records(const M20HitsArgs &a, const RF &rec, unsigned start, const unsigned end, const int block, const int grid, unsigned char *s_fr,
                                     const int lane) {
    if ((int)(end - start) > a.max_frames) start = end - (unsigned)a.max_frames;                   // (what the ring no longer holds)
    for (unsigned i = start; (int)(end - i) > 0; i++) {
        const unsigned slot = i % (unsigned)a.max_frames;
        const M20HitIn h = rec(slot);
        if ((unsigned)h.channel >= (unsigned)a.n_channels) continue;                               // (never: the frame sync numbers its own channels)
        if (h.channel % grid != block) continue;                       // a channel's records in order, by one workgroup: its characters persist from frame to frame
        m20_wave_hit(h, a.chan_bits + (size_t)h.channel * M20_CHAN_CHARS, s_fr, a.out + slot, lane);
    }
}
// the last workgroup to finish moves *done up to `end` (done[1] is its ticket counter); the caller has made its records visible
static RSW_DEV void m20_wave_ticket(unsigned *done, const unsigned end, const int grid, const int lane) {
    if (lane == 0 && mxxw_atomic_inc(&done[1]) == (unsigned)grid - 1u) { done[1] = 0; done[0] = end; }
}
#endif
