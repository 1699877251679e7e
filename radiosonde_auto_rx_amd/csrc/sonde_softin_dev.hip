// sonde_softin_dev.hip — `rs41mod --softin [-i]` for MANY channels on the device, fed from the modem's soft decisions where they lie
// (include/sonde_fsk.h sonde_softin_dev_*): the consumer half of auto_rx's production pipe `fsk_demod ... | rs41mod --softin -i`
// (auto_rx/autorx/decode.py:901-909), so that BASELINE configs[3] ends at decoded, repaired frames without a device-to-host copy of the
// soft-decision stream.
//   find_softbinhead / corr_softhdb (demod/mod/demod_mod.c:1692-1762): the last 64 soft bits against the +-1 header, normalised, in double,
//     |mv| > 0.7 — one lane per bit position, 64 positions at a time; the polarity rule of rs41mod.c:2886-2890 (-i / --auto) on the first hit
//   the bit loop (rs41mod.c:2893-2962): 510 x 8 hard decisions, LSB first, de-whitened — one lane per byte
//   rs41_ecc (rs41mod.c:1703-1769): k_rs41_ecc_batch (sonde_kernels.hip), one workgroup per completed frame
// A wavefront per channel; the state that survives a call (search ring, frame in progress, pending bits of a byte, polarity) lives in
// device memory.  The ring is only advanced while SEARCHING — the reference's frame loop does not touch hdb.sbuf — so a search behind a
// frame starts from the ring as the header left it.  Arithmetic as the reference's (float products, double sums, in order): frames are
// bit-identical for identical soft bits (tests/test_gpu_softin_dev.py against oracle/_ref/fsk_demod | oracle/_ref/rs41mod --softin).
// (no contraction: the reference is plain C on x86-64 — every product and sum rounded on its own)
#pragma clang fp contract(off)
#include "../../include/sonde_fsk.h"
#include "sonde_fsk_dev.h"
#include "sonde_host.h"
#include "sonde_drop_dev.h"
#include "sonde_softhdr_dev.h"
#include "sonde_vit_dev.h"
#include "sonde_softin_wave_dev.h"
#include "sonde_softin_mxx_dev.h"
#include "sonde_softin_rs92_dev.h"
#include "sonde_softin_imet54_dev.h"
#include "sonde_softin_meisei_dev.h"
#include "sonde_softin_mrz_dev.h"
#include "sonde_softin_mts01_dev.h"
#include "sonde_softin_wxr_dev.h"
#include "../../include/sonde_drop.h"
#include "../../include/sonde_rs92.h"
#include "../../include/sonde_imet54.h"
#include "../../include/sonde_meisei.h"
#include "../../include/sonde_mrz.h"
#include "../../include/sonde_mts01.h"
#include "../../include/sonde_wxr.h"
#include "sonde_devmem.h"
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

struct SoftinChan {
    int   mode;                    // 0 searching, 1 inside a frame
    int   inv;                     // gpx.option.inv as it stands (--auto may flip it)
    int   body_done;               // frame bits consumed (0 .. 4080)
    int   carry_n;                 // soft bits of an unfinished byte
    float carry[8];
    float hist[64];                // the last 64 soft bits seen while searching, oldest first (hdb.sbuf)
    float mv;                      // score of the header in front of the frame in progress
    unsigned long long bits_in, hdr_bit;
    unsigned char frame[520];
};
struct SoftinMeta { int channel, len, nbytes; float mv; unsigned long long hdr_bit; };

struct SoftinArgs {
    const float *sd; long long ch_stride;          // soft decisions of channel c at sd + c * ch_stride
    const int *nbits_ch; int nbits;                // per channel (device) or one count for all
    const int *ch_list;                            // the channels of this launch (one workgroup each); null: all of them
    int n_ch, inv_in, opt_auto; float ths;
    SoftinChan *chan;
    unsigned char *frames; int *flen; SoftinMeta *meta; unsigned *count; int cap;
    const unsigned char *hdr;                      // 64 header bits ('0'/'1'), 8 header bytes, 64 mask bytes
};
// what every kernel begins with: the channel of this workgroup, its share of the call (nb symbols at x, wave-uniform) and the sign --softinv gives them;
// false = nothing to do (a channel the launch does not have; a count beyond the stride never comes from the host)
struct SoftinIn { int ch, nb; const float *x; float sgn; };
__device__ __forceinline__ bool softin_input(const SoftinArgs &a, SoftinIn &in) {
    in.ch = a.ch_list ? a.ch_list[blockIdx.x] : (int)blockIdx.x;
    if (in.ch >= a.n_ch || in.ch < 0) return false;
    in.nb = __builtin_amdgcn_readfirstlane(a.nbits_ch ? a.nbits_ch[in.ch] : a.nbits);
    in.x = a.sd + (size_t)in.ch * a.ch_stride; in.sgn = a.inv_in ? -1.f : 1.f;
    return (long long)in.nb <= a.ch_stride;
}

__global__ __launch_bounds__(64)
void k_softin_rs41(const SoftinArgs a) {
    __shared__ float s_hist[64];
    __shared__ unsigned char s_frame[520];
    __shared__ float s_carry[8];
    SoftinIn in;
    if (!softin_input(a, in)) return;
    const int ch = in.ch, nb = in.nb, lane = threadIdx.x;
    const float *x = in.x; const float sgn = in.sgn;
    SoftinChan *st = a.chan + ch;
    int mode = st->mode, inv = st->inv, body_done = st->body_done, carry_n = st->carry_n;
    float mv_hdr = st->mv; unsigned long long hdr_bit = st->hdr_bit; const unsigned long long bits0 = st->bits_in;
    s_hist[lane] = st->hist[lane];
    for (int i = lane; i < 520; i += 64) s_frame[i] = st->frame[i];
    if (lane < 8) s_carry[lane] = st->carry[lane];
    // the header as +-1, one element per lane (for the dot products every lane needs all 64: from LDS-free registers via the constant array)
    __builtin_amdgcn_wave_barrier();
    int cur = 0;
    while (cur < nb) {
        if (mode == 0) {
            // ---- find_softbinhead: position q of the call = stream element 64 + (q - cur) of hist ++ x[cur ..]
            bool found = false;
            int base = cur;
            for (; base < nb && !found; base += 64) {
                const int q = base + lane;
                float mv = 0.f;
                if (q < nb) mv = softhdr_corr64(s_hist, x, sgn, cur, q, a.hdr);
                unsigned long long hits = __ballot(q < nb && fabsf(mv) > a.ths);
                while (hits) {
                    const int l = __builtin_ctzll(hits);
                    hits &= hits - 1;
                    const float mvl = __shfl(mv, l);
                    // the polarity rule (rs41mod.c:2886-2890): a header of the other sign is skipped, or with --auto flips the option
                    if ((double)mvl * (0.5 - inv) < 0) { if (!a.opt_auto) continue; inv ^= 1; }
                    found = true;
                    const int qs = base + l;
                    // the ring as the header leaves it: the 64 elements up to the hit
                    const float v = softhdr_ring64(s_hist, x, sgn, cur, qs, lane);
                    __builtin_amdgcn_wave_barrier();
                    s_hist[lane] = v;
                    __builtin_amdgcn_wave_barrier();
                    mode = 1; body_done = 0; carry_n = 0; mv_hdr = mvl; hdr_bit = bits0 + (unsigned long long)qs + 1ull;
                    cur = qs + 1;
                    break;
                }
            }
            if (!found) {
                const float v = softhdr_ring64(s_hist, x, sgn, cur, nb - 1, lane);
                __builtin_amdgcn_wave_barrier();
                s_hist[lane] = v;
                __builtin_amdgcn_wave_barrier();
                cur = nb;
            }
        } else {
            // ---- the bit loop: bytes from the pending bits of the last call and the new ones
            const int take = min(nb - cur, 4080 - body_done);
            const int tot = carry_n + take, nbytes = tot / 8, byte0 = 8 + (body_done - carry_n) / 8;
            for (int j = lane; j < nbytes; j += 64) {
                unsigned byte = 0;
                for (int b = 0; b < 8; b++) {
                    const int k = 8 * j + b;
                    const float v = k < carry_n ? s_carry[k] : sgn * x[cur + (k - carry_n)];
                    int bit = v >= 0.0f;
                    if (inv) bit ^= 1;
                    byte |= (unsigned)bit << b;                         // bits2byte: LSB first (rs41mod.c:224)
                }
                const int bc = byte0 + j;
                s_frame[bc] = (unsigned char)(byte ^ a.hdr[72 + (bc & 63)]);
            }
            __builtin_amdgcn_wave_barrier();
            const int rest = tot - 8 * nbytes;
            float cv = 0.f;
            if (lane < rest) { const int k = 8 * nbytes + lane; cv = k < carry_n ? s_carry[k] : sgn * x[cur + (k - carry_n)]; }
            __builtin_amdgcn_wave_barrier();
            if (lane < 8) s_carry[lane] = cv;
            __builtin_amdgcn_wave_barrier();
            carry_n = rest; body_done += take; cur += take;
            if (body_done == 4080) {
                // print_frame(): the frame goes out (header bytes in front), rs41_ecc() follows in k_rs41_ecc_batch
                const unsigned slot = softin_wave_slot(a.count, lane);
                if ((int)slot < a.cap) {
                    unsigned char *o = a.frames + (size_t)slot * 518;
                    for (int i = lane; i < 518; i += 64) o[i] = i < 8 ? a.hdr[64 + i] : s_frame[i];
                    if (lane == 0) {
                        int ft = 0; const unsigned char b = s_frame[0x38];
                        for (int i = 0; i < 4; i++) ft += ((b >> i) & 1) - ((b >> (i + 4)) & 1);        // frametype (rs41mod.c:407-415)
                        a.flen[slot] = ft >= 0 ? 320 : 518;
                        SoftinMeta m; m.channel = ch; m.len = ft >= 0 ? 320 : 518; m.nbytes = 518; m.mv = mv_hdr; m.hdr_bit = hdr_bit;
                        a.meta[slot] = m;
                    }
                }
                mode = 0; body_done = 0; carry_n = 0;
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    st->hist[lane] = s_hist[lane];
    for (int i = lane; i < 520; i += 64) st->frame[i] = s_frame[i];
    if (lane < 8) st->carry[lane] = s_carry[lane];
    if (lane == 0) { st->mode = mode; st->inv = inv; st->body_done = body_done; st->carry_n = carry_n; st->mv = mv_hdr; st->hdr_bit = hdr_bit; st->bits_in = bits0 + (unsigned long long)nb; }
}


// ------------------------------------------------------------------------------------------------
// DFM09: dfm09mod --softin (dfm09mod.c:1604-1720) — 32 raw header symbols at 0.7, then two soft symbols per bit (s2 - s1), 8 frames of 280 bits per hit
// (the first one starts behind its 16 header bits), de-interleave + Hamming(8,4) with the soft 2-bit pass of --ecc2 (:231-345) on a lane per codeword
// ------------------------------------------------------------------------------------------------
struct SoftinDfmChan {
    int   mode, inv, dpos, dfrm, dhalf;
    float ds1;
    unsigned hdrcnt;
    float hist[32];
    float mv;
    unsigned long long bits_in, hdr_bit;
    unsigned char dhb[280];
    float dsf[280];
};
// one 8-bit codeword (dfm09mod.c:240-307): 0 clean, j + 1 = bit j fixed, -1 uncorrectable (level 2: the codeword at distance 2 that correlates best with the soft bits)
__device__ __forceinline__ void dfm_dev_codeword(int n, unsigned char *c) {
    const unsigned char d0 = (n >> 3) & 1, d1 = (n >> 2) & 1, d2 = (n >> 1) & 1, d3 = n & 1;
    c[0] = d0; c[1] = d1; c[2] = d2; c[3] = d3; c[4] = d1 ^ d2 ^ d3; c[5] = d0 ^ d2 ^ d3; c[6] = d0 ^ d1 ^ d3; c[7] = d0 ^ d1 ^ d2;
}
__device__ int dfm_dev_check(int level, unsigned char hb[8], const float sb[8]) {
    const unsigned char Hm[4][8] = { {0,1,1,1,1,0,0,0}, {1,0,1,1,0,1,0,0}, {1,1,0,1,0,0,1,0}, {1,1,1,0,0,0,0,1} };
    const unsigned char He[8] = { 0x7, 0xB, 0xD, 0xE, 0x8, 0x4, 0x2, 0x1 };
    unsigned syn = 0;
    for (int i = 0; i < 4; i++) { unsigned char s = 0; for (int j = 0; j < 8; j++) s ^= Hm[i][j] & hb[j]; syn = (syn << 1) | s; }
    if (!syn) return 0;
    for (int j = 0; j < 8; j++) if (syn == He[j]) { hb[j] ^= 1; return j + 1; }
    if (level == 2) {
        int best = -1; float bestsum = 0.0f;
        for (int n = 0; n < 16; n++) {
            unsigned char c[8]; int d = 0;
            dfm_dev_codeword(n, c);
            for (int i = 0; i < 8; i++) d += (hb[i] != c[i]);
            if (d != 2) continue;
            float sum = 0.0f;
            for (int i = 0; i < 8; i++) sum += (2 * c[i] - 1) * sb[i];
            if (sum >= bestsum) { bestsum = sum; best = n; }
        }
        if (best >= 0) dfm_dev_codeword(best, hb);
    }
    return -1;
}

struct SoftinDfmArgs {
    SoftinArgs base;                       // sd / counts / n_ch / inv_in / opt_auto / ths / count / cap / hdr (32 raw header symbols)
    SoftinDfmChan *chan;
    sonde_dfm_frame_t *out;
    int ecc_level;
};

__global__ __launch_bounds__(64)
void k_softin_dfm(const SoftinDfmArgs A) {
    const SoftinArgs &a = A.base;
    __shared__ float s_hist[32];
    __shared__ unsigned char s_hb[280];
    __shared__ float s_sf[280];
    SoftinIn in;
    if (!softin_input(a, in)) return;
    const int ch = in.ch, nb = in.nb, lane = threadIdx.x;
    const float *x = in.x; const float sgn = in.sgn;
    SoftinDfmChan *st = A.chan + ch;
    int mode = st->mode, inv = st->inv, dpos = st->dpos, dfrm = st->dfrm, dhalf = st->dhalf;
    float ds1 = st->ds1, mv_hdr = st->mv; unsigned hdrcnt = st->hdrcnt; unsigned long long hdr_bit = st->hdr_bit; const unsigned long long bits0 = st->bits_in;
    if (lane < 32) s_hist[lane] = st->hist[lane];
    for (int i = lane; i < 280; i += 64) { s_hb[i] = st->dhb[i]; s_sf[i] = st->dsf[i]; }
    __builtin_amdgcn_wave_barrier();
    int cur = 0;
    while (cur < nb) {
        if (mode == 0) {
            bool found = false;
            for (int base = cur; base < nb && !found; base += 64) {
                const int q = base + lane;
                float mv = 0.f;
                if (q < nb) {
                    double sum = 0.0, normx = 0.0;
                    const int e = 32 + (q - cur);
                    for (int i = 0; i < 32; i++) {
                        const int k = e - 31 + i;
                        const float v = k < 32 ? s_hist[k] : sgn * x[cur + (k - 32)];
                        const float y = (a.hdr[i] & 1) ? 1.f : -1.f;
                        sum += (double)(y * v);
                        normx += (double)(v * v);
                    }
                    sum /= sqrt(normx * 32.0);
                    mv = (float)sum;
                }
                unsigned long long hits = __ballot(q < nb && fabsf(mv) > a.ths);
                while (hits) {
                    const int l = __builtin_ctzll(hits);
                    hits &= hits - 1;
                    const float mvl = __shfl(mv, l);
                    hdrcnt += 8;                                        // every header seen counts (dfm09mod.c:1628,1632), accepted or not
                    if ((double)mvl * (0.5 - inv) < 0) { if (!a.opt_auto) continue; inv ^= 1; }
                    found = true;
                    const int qs = base + l, e = 32 + (qs - cur), k = e - 31 + (lane & 31);
                    const float v = k < 32 ? s_hist[k] : sgn * x[cur + (k - 32)];
                    __builtin_amdgcn_wave_barrier();
                    if (lane < 32) s_hist[lane] = v;
                    __builtin_amdgcn_wave_barrier();
                    mode = 1; dpos = 16; dfrm = 0; dhalf = 0; mv_hdr = mvl; hdr_bit = bits0 + (unsigned long long)qs + 1ull;
                    cur = qs + 1;
                    break;
                }
            }
            if (!found) {
                const int e = 32 + (nb - 1 - cur), k = e - 31 + (lane & 31);
                const float v = k < 32 ? s_hist[k] : sgn * x[cur + (k - 32)];
                __builtin_amdgcn_wave_barrier();
                if (lane < 32) s_hist[lane] = v;
                __builtin_amdgcn_wave_barrier();
                cur = nb;
            }
        } else {
            // ---- frame bits: two symbols each (the first of a pair may be left over from the last call)
            const int need = 280 - dpos, take = min(nb - cur, 2 * need - dhalf), nbits = (dhalf + take) / 2;
            for (int j = lane; j < nbits; j += 64) {
                const float s1 = (j == 0 && dhalf) ? ds1 : sgn * x[cur + 2 * j - dhalf], s2 = sgn * x[cur + 2 * j + 1 - dhalf];
                float v = s2 - s1;                                      // integrate both Manchester symbols (dfm09mod.c:1684)
                int hb = v >= 0.0f;
                if (inv) { hb ^= 1; v = -v; }
                s_hb[dpos + j] = (unsigned char)hb; s_sf[dpos + j] = v;
            }
            __builtin_amdgcn_wave_barrier();
            if ((dhalf + take) & 1) { ds1 = sgn * x[cur + take - 1]; dhalf = 1; } else dhalf = 0;
            dpos += nbits; cur += take;
            if (dpos == 280) {
                const unsigned slot = softin_wave_slot(a.count, lane);
                // de-interleave + Hamming: lanes 0..6 conf (block at bit 16, 7 codewords), 7..19 dat1 (72, 13), 20..32 dat2 (176, 13)
                int e = 0; unsigned char nib = 0;
                const int blk = lane < 7 ? 0 : lane < 20 ? 1 : 2, i = lane < 7 ? lane : lane < 20 ? lane - 7 : lane - 20;
                const int L = blk == 0 ? 7 : 13, off = blk == 0 ? 16 : blk == 1 ? 72 : 176;
                if (lane < 33) {
                    unsigned char c[8]; float sb[8];
                    for (int j = 0; j < 8; j++) { c[j] = s_hb[off + L * j + i]; sb[j] = s_sf[off + L * j + i]; }
                    if (A.ecc_level) e = dfm_dev_check(A.ecc_level, c, sb);
                    nib = (unsigned char)((c[0] << 3) | (c[1] << 2) | (c[2] << 1) | c[3]);
                }
                const unsigned long long fixed = __ballot(lane < 33 && e > 0), bad = __ballot(lane < 33 && e < 0);
                if ((int)slot < a.cap) {
                    sonde_dfm_frame_t *o = A.out + slot;
                    if (lane < 7) o->conf[i] = nib; else if (lane < 20) o->dat1[i] = nib; else if (lane < 33) o->dat2[i] = nib;
                    if (lane < 35) { unsigned char rb = 0; for (int b = 0; b < 8; b++) rb |= (unsigned char)((s_hb[8 * lane + b] & 1) << b); o->rawbits[lane] = rb; }
                    if (lane == 0) {
                        o->channel = ch; o->frame_in_hit = dfrm; o->mv = mv_hdr; o->mv_pos = (uint32_t)hdr_bit;
                        o->frm_count = (float)(hdrcnt + (unsigned)dfrm); o->inv = inv; o->pad[0] = o->pad[1] = o->pad[2] = 0; o->pad2 = 0;
                        // hamming()'s return per block: a bit per fixed codeword, or'ed with -1 for an uncorrectable one
                        o->ecc[0] = ((bad & 0x7Full) ? -1 : 0) | (int)(fixed & 0x7Full);
                        o->ecc[1] = (((bad >> 7) & 0x1FFFull) ? -1 : 0) | (int)((fixed >> 7) & 0x1FFFull);
                        o->ecc[2] = (((bad >> 20) & 0x1FFFull) ? -1 : 0) | (int)((fixed >> 20) & 0x1FFFull);
                    }
                }
                dpos = 0;
                if (++dfrm == 8) mode = 0;                              // nfrms frames per header hit, then search again (:1656,1718)
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 32) st->hist[lane] = s_hist[lane];
    for (int i = lane; i < 280; i += 64) { st->dhb[i] = s_hb[i]; st->dsf[i] = s_sf[i]; }
    if (lane == 0) { st->mode = mode; st->inv = inv; st->dpos = dpos; st->dfrm = dfrm; st->dhalf = dhalf; st->ds1 = ds1; st->hdrcnt = hdrcnt; st->mv = mv_hdr; st->hdr_bit = hdr_bit; st->bits_in = bits0 + (unsigned long long)nb; }
}

// ------------------------------------------------------------------------------------------------
// M10: m10mod --softin (m10mod.c:1405-1510) — 32 raw header symbols at 0.8 in either polarity, two soft symbols per bit (s2 - s1), differential decoding,
// 968 bits, then one symbol per counted bit dropped up to 5 x 808; the frame checksum (m10mod.c:594-628) on the device
// ------------------------------------------------------------------------------------------------
struct SoftinM10Chan {
    int   mode, inv, mpos, mhalf, mbit0, mskip;
    float ms1;
    float hist[32];
    float mv;
    unsigned long long bits_in, hdr_bit;
    char  mbits[976];
};
struct SoftinM10Args { SoftinArgs base; SoftinM10Chan *chan; sonde_m10_frame_t *out; int stage_cap; };
// (M10_STAGE_MAX, the soft decisions of a call the kernel keeps in LDS: sonde_softin_wave_dev.h)

// The header search (find_softbinhead / corr_softhdb, demod_mod.c:1692-1762) evaluates at EVERY symbol the normalised correlation of the last 32 with the header, in
// double.  Round 5 did exactly that on a lane per position — 64 dependent double adds and 32 global loads each, 0.37 ms for 341 channels.  Now the call's soft decisions
// are staged in LDS once and every position gets the same quantity in float first (error < 1e-5); only a position whose float value comes within 1e-3 of the
// threshold — a header, a few per second — is evaluated again the reference's way (same operands, same order, double), and that value decides and is recorded.
__global__ __launch_bounds__(64)
void k_softin_m10(const SoftinM10Args A) {
    const SoftinArgs &a = A.base;
    extern __shared__ float s_x[];                     // [stage_cap] sgn * x of this call (staged: nb <= stage_cap)
    __shared__ float s_hist[32];
    __shared__ char s_mb[976];
    __shared__ unsigned char s_fr[124];
    SoftinIn in;
    if (!softin_input(a, in)) return;
    const int ch = in.ch, nb = in.nb, lane = threadIdx.x;
    SoftinM10Chan *st = A.chan + ch;
    constexpr int NBITS = 121 * 8;
    int mode = st->mode, inv = st->inv, mpos = st->mpos, mhalf = st->mhalf, mbit0 = st->mbit0, mskip = st->mskip;
    float ms1 = st->ms1, mv_hdr = st->mv; unsigned long long hdr_bit = st->hdr_bit; const unsigned long long bits0 = st->bits_in;
    if (lane < 32) s_hist[lane] = st->hist[lane];
    for (int i = lane; i < 976; i += 64) s_mb[i] = st->mbits[i];
    const SoftinX X = softin_wave_stage(s_x, in.x, in.sgn, nb, A.stage_cap, lane);           // soft decision p of this call, in the polarity in effect
    rsw_wave_sync();
    unsigned hbits = 0;                                                          // the 32 header symbols as a bit mask
    for (int i = 0; i < 32; i++) hbits |= (unsigned)(a.hdr[i] & 1) << i;
    int cur = 0;
    while (cur < nb) {
        if (mode == 0) {
            // element k of the ring ++ the call's symbols from `cur`
            const int cur0 = cur;
            auto W = [&](const int k) -> float { return k < 32 ? s_hist[k] : X(cur0 + (k - 32)); };
            bool found = false;
            for (int base = cur0; base < nb && !found; base += 64) {
                const int q = base + lane;
                float mv = 0.f;
                if (q < nb) {
                    // softin_wave_score<32>, written out: with the header in a register (a.hdr, not a constant) the template's unrolled loops keep 32 condition
                    // masks in scalar registers — 85 of them spilled, 80 vector registers for 66 and a wave less per SIMD
                    const int k0 = q - cur0 + 1;                          // the window of position q ends with the symbol at q
                    float fs = 0.f, fn = 0.f;
                    for (int i = 0; i < 32; i++) {
                        const float v = W(k0 + i);
                        fs += ((hbits >> i) & 1u) ? v : -v;
                        fn = fmaf(v, v, fn);
                    }
                    mv = fs * mxxw_rsq(fn * 32.0f);
                    if (!(fabsf(mv) < a.ths - 1e-3f)) {                   // (also NaN: an all-zero window is the reference's 0 / 0)
                        double sum = 0.0, normx = 0.0;
                        for (int i = 0; i < 32; i++) {
                            const float v = W(k0 + i);
                            const float y = ((hbits >> i) & 1u) ? 1.f : -1.f;
                            sum += (double)(y * v);
                            normx += (double)(v * v);
                        }
                        sum /= sqrt(normx * 32.0);
                        mv = (float)sum;
                    }
                }
                const unsigned long long hits = __ballot(q < nb && fabsf(mv) > a.ths);
                if (hits) {
                    const int l = __builtin_ctzll(hits), qs = base + l;
                    const float mvl = mxxw_bcast_f(mv, l);
                    if ((double)mvl * (0.5 - inv) < 0) inv ^= 1;            // irrelevant for the differential code (m10mod.c:1447)
                    found = true;
                    softin_wave_ring<32>(s_hist, W, qs - cur0 + 1, lane);  // the ring as the header leaves it: the 32 elements up to the hit
                    mode = 1; mpos = 0; mhalf = 0; mbit0 = '0'; mv_hdr = mvl; hdr_bit = bits0 + (unsigned long long)qs + 1ull;
                    cur = qs + 1;
                }
            }
            if (!found) {
                softin_wave_ring<32>(s_hist, W, nb - cur0, lane);          // the 32 elements up to the call's last symbol
                cur = nb;
            }
        } else if (mode == 1) {
            const int need = NBITS - mpos, take = min(nb - cur, 2 * need - mhalf), nbits = (mhalf + take) / 2;
            // bit j of this call and the one before it (the differential code): out = 0x31 ^ (previous ^ bit); the previous of the frame's first bit is '0' (0x30),
            // which leaves that character outside '0' / '1' — the reference's own quirk, kept
            int last_bit = mbit0;
            for (int j0 = 0; j0 < nbits; j0 += 64) {
                const int j = j0 + lane;
                int bit = 0, prev = 0;
                if (j < nbits) {
                    const float s1 = (j == 0 && mhalf) ? ms1 : X(cur + 2 * j - mhalf), s2 = X(cur + 2 * j + 1 - mhalf);
                    bit = (s2 - s1) >= 0.0f;
                }
                prev = __shfl_up(bit, 1);
                if (lane == 0) prev = last_bit;
                if (j < nbits) s_mb[mpos + j] = (char)(0x31 ^ (prev ^ bit));
                const int cnt = min(64, nbits - j0);
                last_bit = __shfl(bit, cnt - 1);
            }
            __builtin_amdgcn_wave_barrier();
            if (nbits > 0) mbit0 = last_bit;
            if ((mhalf + take) & 1) { ms1 = X(cur + take - 1); mhalf = 1; } else mhalf = 0;
            mpos += nbits; cur += take;
            if (mpos == NBITS) {
                const unsigned slot = softin_wave_slot(a.count, lane);
                for (int i = lane; i < 124; i += 64) {
                    unsigned v = 0;
                    if (i < 121) for (int k = 0; k < 8; k++) if (s_mb[8 * i + 7 - k] == '1') v |= 1u << k;
                    s_fr[i] = (unsigned char)v;
                }
                __builtin_amdgcn_wave_barrier();
                if ((int)slot < a.cap) {
                    sonde_m10_frame_t *o = A.out + slot;
                    for (int i = lane; i < 124; i += 64) o->frame[i] = s_fr[i];
                    if (lane == 0) {
                        int aux = s_fr[0] - 0x64;
                        if (aux < 0 || aux > 20) aux = 0;
                        int c = 0;
                        for (int i = 0; i < 99 + aux; i++) {                 // checkM10 (m10mod.c:594-628)
                            unsigned char b = s_fr[i];
                            b = (unsigned char)((b >> 1) | ((b & 1) << 7));
                            b ^= (b >> 2) & 0xFF;
                            const int t6 = (c & 1) ^ ((c >> 2) & 1) ^ ((c >> 4) & 1), t7 = ((c >> 1) & 1) ^ ((c >> 3) & 1) ^ ((c >> 5) & 1);
                            const int t = (c & 0x3F) | (t6 << 6) | (t7 << 7);
                            int sreg = (c >> 7) & 0xFF;
                            sreg ^= (sreg >> 2) & 0xFF;
                            c = (((c & 0xFF) << 8) | ((b ^ t ^ sreg) & 0xFF)) & 0xFFFF;
                        }
                        o->channel = ch; o->nbits = NBITS; o->len = 101 + aux; o->cs_calc = (uint32_t)c;
                        o->cs_ok = ((uint32_t)((s_fr[99 + aux] << 8) | s_fr[100 + aux]) == (uint32_t)c);
                        o->mv = mv_hdr; o->mv_pos = (uint32_t)hdr_bit;
                    }
                }
                mode = 2; mskip = NBITS;
            }
        } else {
            // the rest of the second: one symbol per counted bit up to 5 x 808 (m10mod.c:1494-1506)
            const int take = min(nb - cur, 5 * 808 - mskip);
            mskip += take; cur += take;
            if (mskip >= 5 * 808) mode = 0;
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 32) st->hist[lane] = s_hist[lane];
    for (int i = lane; i < 976; i += 64) st->mbits[i] = s_mb[i];
    if (lane == 0) { st->mode = mode; st->inv = inv; st->mpos = mpos; st->mhalf = mhalf; st->mbit0 = mbit0; st->mskip = mskip; st->ms1 = ms1; st->mv = mv_hdr; st->hdr_bit = hdr_bit; st->bits_in = bits0 + (unsigned long long)nb; }
}

// ------------------------------------------------------------------------------------------------
// M20: m20mod --softin (m20mod.c:1276-1377) — as M10 with 1320 bits a frame, the verdicts of m20mod's print_frame (:875-907: length byte with its clamp, firmware
// byte, frame checksum, block checksum) and the skip as an option (-vvv, auto_rx's form, searches on right behind the frame): sonde_softin_mxx_dev.h, which the
// CPU wave emulator compiles as well.  The call's soft decisions are staged in LDS as for M10 (a second at 9600 Bd: 38.4 KB + 1.6 KB of state, four waves per CU).
// ------------------------------------------------------------------------------------------------
struct SoftinM20Args { SoftinArgs base; SoftinM20Chan *chan; sonde_m20_frame_t *out; int stage_cap, doskip; };

__global__ __launch_bounds__(64)
void k_softin_m20(const SoftinM20Args A) {
    const SoftinArgs &a = A.base;
    extern __shared__ float s_x[];                     // [stage_cap] sgn * x of this call (staged: nb <= stage_cap)
    __shared__ SoftinM20Lds s_l;
    SoftinIn in;
    if (!softin_input(a, in)) return;
    m20_wave_channel(A.chan + in.ch, in.x, in.nb, in.sgn, a.ths, A.doskip, &s_l, s_x, A.stage_cap, A.out, a.count, a.cap, in.ch, threadIdx.x);
}

// ------------------------------------------------------------------------------------------------
// RS92: rs92mod --softin [-i] --ecc (rs92mod.c:1959-2050, :183-196, :1360-1385) — the 60 raw header symbols at 0.8 with the ring emptied on every hit, 234 bytes of
// 10 bits from two soft symbols per bit on a lane per byte, then RS(255,231) of the frame on the same wave: sonde_softin_rs92_dev.h, which the CPU wave emulator
// compiles as well.  The call's soft decisions are staged in LDS as for M10 / M20 (a second at 4800 symbols: 19.2 KB + 1.6 KB of state).  A record per completed
// frame; CRCs, the GPS solution and the text are the host's (sonde_rs92_dec_corrected).
// ------------------------------------------------------------------------------------------------
struct SoftinRs92Args { SoftinArgs base; SoftinRs92Chan *chan; SoftinRs92Rec *out; const unsigned char *gf; int stage_cap, inv; };

__global__ __launch_bounds__(64)
void k_softin_rs92(const SoftinRs92Args A) {
    const SoftinArgs &a = A.base;
    extern __shared__ float s_x[];                     // [stage_cap] sgn * x of this call (staged: nb <= stage_cap)
    __shared__ SoftinRs92Lds s_l;
    SoftinIn in;
    if (!softin_input(a, in)) return;
    rs92_wave_channel(A.chan + in.ch, in.x, in.nb, in.sgn, A.inv, a.ths, A.gf, &s_l, s_x, A.stage_cap, A.out, a.count, a.cap, in.ch, threadIdx.x);
}

// ------------------------------------------------------------------------------------------------
// iMet-54: imet54mod --softin [-i] [--auto] [--ecc] (imet54mod.c:1007-1063, :107-133, :162-303, :350-360, :618-660) — the 40 header symbols at 0.8 with the ring left
// as it is, 220 8N1 characters on a lane per character, then de-interleave + Hamming(8,4) on a lane per codeword, the ecc sums by ballot and both check sums as XOR
// sums of per-bit contribution words on the same wave: sonde_softin_imet54_dev.h, which the CPU wave emulator compiles as well.  The call's soft decisions are
// staged in LDS as for M10 / M20 / RS92 (a second at 4800 symbols: 19.2 KB + 0.75 KB of state).  A record per completed frame; the fields and the text are the
// host's (sonde_imet54_dec_decoded).
// ------------------------------------------------------------------------------------------------
struct SoftinImet54Args { SoftinArgs base; SoftinImet54Chan *chan; SoftinImet54Rec *out; const uint32_t *tab; int stage_cap, ecc; };

__global__ __launch_bounds__(64)
void k_softin_imet54(const SoftinImet54Args A) {
    const SoftinArgs &a = A.base;
    extern __shared__ float s_x[];                     // [stage_cap] sgn * x of this call (staged: nb <= stage_cap)
    __shared__ SoftinImet54Lds s_l;
    SoftinIn in;
    if (!softin_input(a, in)) return;
    imet54_wave_channel(A.chan + in.ch, in.x, in.nb, in.sgn, a.opt_auto, A.ecc, a.ths, A.tab, &s_l, s_x, A.stage_cap, A.out, a.count, a.cap, in.ch, threadIdx.x);
}

// ------------------------------------------------------------------------------------------------
// Meisei iMS-100 / RS-11G: meisei100mod --softin [--ecc] (meisei100mod.c:654-776) — the 48 header half symbols at 0.8 in either polarity with the ring left as it
// is, biphase-S bits on a lane per bit packed by ballot, then the 12 BCH(63,51) blocks one at a time on the same wave (syndromes as an XOR sum, the error positions
// as one ballot of the locator's values, padding and word parities as population counts): sonde_softin_meisei_dev.h, which the CPU wave emulator compiles as well.
// The call's soft decisions are staged in LDS as for M10 / M20 / RS92 / iMet-54 (a second at 2400 half symbols: 9.6 KB + 0.27 KB of state).  A record per completed
// frame; the fields and the text are the host's (sonde_meisei_dec_decoded).
// ------------------------------------------------------------------------------------------------
struct SoftinMeiseiArgs { SoftinArgs base; SoftinMeiseiChan *chan; SoftinMeiseiRec *out; int stage_cap, ecc; };

__global__ __launch_bounds__(64)
void k_softin_meisei(const SoftinMeiseiArgs A) {
    const SoftinArgs &a = A.base;
    extern __shared__ float s_x[];                     // [stage_cap] sgn * x of this call (staged: nb <= stage_cap)
    __shared__ SoftinMeiseiLds s_l;
    SoftinIn in;
    if (!softin_input(a, in)) return;
    meisei_wave_channel(A.chan + in.ch, in.x, in.nb, in.sgn, A.ecc, a.ths, &s_l, s_x, A.stage_cap, A.out, a.count, a.cap, in.ch, threadIdx.x);
}

// ------------------------------------------------------------------------------------------------
// MRZ / MP3-H1: mp3h1mod --softin [-i] [--auto] [--ofs n] (mp3h1mod.c:1151-1242, :157-183, :280-310, :805-815) — the 44 header half symbols at 0.82 with the polarity
// rule and the ring left as it is, Manchester bits (s2 - s1) on a lane per bit packed by ballot, then bytes, frame type and the CRC-16 on the same wave (a lane per
// byte carried through the shifts behind it, the XOR over the wave): the verdict sets the length of the channel's NEXT frame, 408 or 384 bits, inside the same
// call: sonde_softin_mrz_dev.h, which the CPU wave emulator compiles as well.  The call's soft decisions are staged in LDS as for the other staged kinds (a second
// at 2400 half symbols: 9.6 KB + 0.28 KB of state).  A record per completed frame; the fields and the text are the host's (sonde_mrz_dec_decoded).
// ------------------------------------------------------------------------------------------------
struct SoftinMrzArgs { SoftinArgs base; SoftinMrzChan *chan; SoftinMrzRec *out; int stage_cap, classify, bits_ofs; };

__global__ __launch_bounds__(64)
void k_softin_mrz(const SoftinMrzArgs A) {
    const SoftinArgs &a = A.base;
    extern __shared__ float s_x[];                     // [stage_cap] sgn * x of this call (staged: nb <= stage_cap)
    __shared__ SoftinMrzLds s_l;
    SoftinIn in;
    if (!softin_input(a, in)) return;
    mrz_wave_channel(A.chan + in.ch, in.x, in.nb, in.sgn, a.opt_auto, A.classify, A.bits_ofs, a.ths, &s_l, s_x, A.stage_cap, A.out, a.count, a.cap, in.ch, threadIdx.x);
}

// ------------------------------------------------------------------------------------------------
// MTS01: mts01mod --softin (mts01mod.c:543-618, :76-127, :151-162) — the 32 header symbols at 0.8 in either polarity with the ring left as it is, 1048 bits read raw
// on a lane per bit packed by ballot, then the 131 bytes and the CRC-16 on the same wave (two bytes per lane, the XOR over the wave, bit-reversed):
// sonde_softin_mts01_dev.h, which the CPU wave emulator compiles as well.  Staged as the others (a second at 1200 symbols: 4.8 KB + 0.39 KB of state).  A record
// per completed frame; the fields and the text are the host's (sonde_mts01_dec_decoded).
// ------------------------------------------------------------------------------------------------
struct SoftinMts01Args { SoftinArgs base; SoftinMts01Chan *chan; SoftinMts01Rec *out; int stage_cap; };

__global__ __launch_bounds__(64)
void k_softin_mts01(const SoftinMts01Args A) {
    const SoftinArgs &a = A.base;
    extern __shared__ float s_x[];                     // [stage_cap] sgn * x of this call (staged: nb <= stage_cap)
    __shared__ SoftinMts01Lds s_l;
    SoftinIn in;
    if (!softin_input(a, in)) return;
    mts01_wave_channel(A.chan + in.ch, in.x, in.nb, in.sgn, a.ths, &s_l, s_x, A.stage_cap, A.out, a.count, a.cap, in.ch, threadIdx.x);
}

// ------------------------------------------------------------------------------------------------
// Weathex WxR-301D: weathex301d --softin [-i] [--pn9] (weathex301d.c:607-648, :250-256, :272-294, :359-375) — no correlation: the sign of every soft bit goes into the
// 40-bit ring (frame bits too), a frame is the header and the 512 bits behind a ring that equals AA AA AA 2D D4 / AA AA AA C1 94, and at its end the 69 bytes, the PN9
// de-whitening and the xor8 / sum8 check run on the same wave: sonde_softin_wxr_dev.h, which the CPU wave emulator compiles as well.  The soft decisions are read
// once, so nothing is staged: 216 B of LDS.  A record per completed frame; the text is the host's (sonde_wxr_print_decoded).
// ------------------------------------------------------------------------------------------------
struct SoftinWxrArgs { SoftinArgs base; SoftinWxrChan *chan; SoftinWxrRec *out; int inv, pn9; };

__global__ __launch_bounds__(64)
void k_softin_wxr(const SoftinWxrArgs A) {
    const SoftinArgs &a = A.base;
    __shared__ SoftinWxrLds s_l;
    SoftinIn in;
    if (!softin_input(a, in)) return;                  // (both inversions are in A.inv: the sign is not applied here)
    wxr_wave_channel(A.chan + in.ch, in.x, in.nb, A.inv, A.pn9, &s_l, A.out, a.count, a.cap, in.ch, threadIdx.x);
}

// ------------------------------------------------------------------------------------------------
// RD94 / RD41 dropsondes: rd94rd41drop --softin / --softinv [-i] (rd94rd41drop.c:1357-1386) — no correlation: the sign of every soft bit (s >= 0 after the two
// inversions, which cancel each other) goes into the 40-bit ring, a frame is the 2360 raw bits behind a ring that equals FC 1D as Manchester-coded 8N1, and the
// bits of a frame enter the ring too.  64 soft bits a pass: signs by ballot, every lane tests the ring as it stands behind its bit (values and "holds a bit"
// masks, as in k_drop_slice); inside a frame the lanes write up to 64 raw bits a pass.  A finished frame is completed on the device (drop_complete_frame).
// ------------------------------------------------------------------------------------------------
struct SoftinDropChan {
    int found, pos;                                // header open; raw bits of the frame so far (40 = the header alone)
    unsigned long long hist, valid, bits_in, t_hdr;
    unsigned char frame[DROP_RAWBITS];
};
struct SoftinDropArgs { SoftinArgs base; SoftinDropChan *chan; DropFrame *out; int inv; };

// the ring after bits 0 .. k of the pass (bm: bit i = soft bit i of the pass), newest bit lowest
__device__ __forceinline__ void drop_ring_after(unsigned long long hist, unsigned long long valid, unsigned long long bm, int k, unsigned long long &h, unsigned long long &v) {
    constexpr unsigned long long M40 = (1ULL << DROP_HEADLEN) - 1;
    const unsigned long long fresh = __brevll(bm) >> (63 - k), ones = (2ULL << k) - 1;       // bits 0 .. k, bit 0 highest
    h = ((k + 1 >= DROP_HEADLEN ? 0 : hist << (k + 1)) | fresh) & M40;
    v = ((k + 1 >= DROP_HEADLEN ? 0 : valid << (k + 1)) | ones) & M40;
}

__global__ __launch_bounds__(64)
void k_softin_drop(const SoftinDropArgs A) {
    const SoftinArgs &a = A.base;
    constexpr unsigned long long M40 = (1ULL << DROP_HEADLEN) - 1;
    __shared__ unsigned char s_fb[DROP_RAWBITS];
    __shared__ unsigned char s_by[128];
    SoftinIn in;
    if (!softin_input(a, in)) return;
    const int ch = in.ch, nb = in.nb, lane = threadIdx.x;
    const float *x = in.x;                         // (both inversions are in A.inv: the sign is not applied here)
    SoftinDropChan *st = A.chan + ch;
    int found = __builtin_amdgcn_readfirstlane(st->found), pos = __builtin_amdgcn_readfirstlane(st->pos);
    unsigned long long hist = st->hist, valid = st->valid, t_hdr = st->t_hdr;
    const unsigned long long bits0 = st->bits_in;
    for (int i = lane; i < DROP_RAWBITS; i += 64) s_fb[i] = st->frame[i];
    __syncthreads();
    int cur = 0;
    while (cur < nb) {
        if (!found) {
            const int q = cur + lane, nv = min(64, nb - cur);
            const float s = q < nb ? x[q] : 0.f;
            const unsigned long long bm = __ballot(q < nb && (A.inv ? s <= 0.0f : s >= 0.0f));
            unsigned long long h, v;
            drop_ring_after(hist, valid, bm, lane, h, v);
            const unsigned long long hm = __ballot(lane < nv && h == DROP_HDR40 && v == M40);
            const int used = hm ? __builtin_ctzll(hm) + 1 : nv;
            drop_ring_after(hist, valid, bm, used - 1, h, v);
            hist = h; valid = v;
            if (hm) { found = 1; pos = DROP_HEADLEN; t_hdr = bits0 + (unsigned long long)(cur + used); }
            cur += used;
        } else {
            const int take = min(nb - cur, DROP_RAWBITS - pos);
            for (int j = lane; j < take; j += 64) { const float s = x[cur + j]; s_fb[pos + j] = (unsigned char)(A.inv ? s <= 0.0f : s >= 0.0f); }
            pos += take; cur += take;
            if (pos == DROP_RAWBITS) {
                drop_complete_frame(s_fb, DROP_RAWBITS, s_by, A.out, (int *)a.count, a.cap, ch, t_hdr, 1, lane);
                const unsigned long long tail = __ballot(lane < DROP_HEADLEN && s_fb[DROP_RAWBITS - DROP_HEADLEN + lane]);
                hist = __brevll(tail) >> 24; valid = M40;
                found = 0; pos = DROP_HEADLEN;
            }
        }
    }
    __syncthreads();
    for (int i = lane; i < DROP_RAWBITS; i += 64) st->frame[i] = s_fb[i];
    if (lane == 0) { st->found = found; st->pos = pos; st->hist = hist; st->valid = valid; st->t_hdr = t_hdr; st->bits_in = bits0 + (unsigned long long)nb; }
}

// ------------------------------------------------------------------------------------------------
// LMS6 / LMS-X: lms6Xmod --softin --vit | --vit2 (lms6Xmod.c:1352-1433, :232-441) — the 64-symbol raw header at 0.7 in either polarity, 4096 / 4720 raw bits with
// every second one inverted behind 80 sync positions, then the K = 7 Viterbi decoder on the wave (a trellis state per lane), deconv and bits2bytes: sonde_vit_dev.h.
// A record per completed block (block_bytes); RS(255,223), frame sync, CRC and the text are the host's (sonde_lms6_dec_block_bytes).  39 KB of LDS per wave
// (block 19.2 KB + decision words 19.2 KB + ring: 38 656 B): four waves per CU.
// ------------------------------------------------------------------------------------------------
struct SoftinLms6Args { SoftinArgs base; Lms6Chan *chan; Lms6Block *out; int vit, stop_at_block; };

__global__ __launch_bounds__(64)
void k_softin_lms6(const SoftinLms6Args A) {
    const SoftinArgs &a = A.base;
    __shared__ Lms6Lds s_l;
    SoftinIn in;
    if (!softin_input(a, in)) return;
    lms6_wave_channel(A.chan + in.ch, in.x, in.nb, in.sgn, A.vit, A.stop_at_block, a.hdr, &s_l, A.out, a.count, a.cap, in.ch, threadIdx.x);
}

// ------------------------------------------------------------------------------------------------
// The same block codes for the BASE-RATE engine's hits (sonde_engine.cpp): what sonde_engine_fetch_dfm / _m10 used to do per frame on one host thread
// now runs over the records a process call has queued, behind its frame-sync kernel on the same stream.  Only decoded frames come to the host (DFM: 8 x 104 bytes
// a hit instead of 2224 soft bits).
//   DFM (dfm09mod.c:1652-1717, :231-345): a hit = frame 0 (bits 16..279, the header went to the correlator) + 7 x 280 bits; de-interleave, Hamming(8,4) per
//        codeword on a lane (hard, or --ecc2's soft 2-bit pass), block status by ballot
//   M10 (m10mod.c:1484, :141-166, :594-628): differential decoding into the channel's persistent bit characters, bits2bytes, checkM10
// Records [*done, *fcount) of the ring; the last workgroup to finish moves *done up (done[1] is its ticket counter).
// ------------------------------------------------------------------------------------------------
#include "sonde_dev.h"
__global__ __launch_bounds__(64)
void k_dfm_hits(const FrameRec *frames, const float *soft, const int nbits, const int max_frames, const unsigned *fcount, unsigned *done, sonde_dfm_frame_t *out, const int ecc_level) {
    __shared__ unsigned char s_hb[280];
    __shared__ float s_sf[280];
    const int lane = threadIdx.x;
    const unsigned end = *fcount; unsigned start = done[0];
    if ((int)(end - start) > max_frames) start = end - (unsigned)max_frames;       // (what the ring no longer holds)
    for (unsigned i = start + blockIdx.x; (int)(end - i) > 0; i += gridDim.x) {
        const unsigned idx = i % (unsigned)max_frames;
        const FrameRec &r = frames[idx];
        const float *sb = soft + (size_t)idx * nbits;
        for (int f = 0; f < 8; f++) {
            const int first = f == 0 ? 0 : 264 + 280 * (f - 1), skip = f == 0 ? 16 : 0;
            sonde_dfm_frame_t *o = out + (size_t)idx * 8 + f;
            if (first + (280 - skip) > r.nbytes) { if (lane == 0) o->frame_in_hit = -1; continue; }       // nbytes = valid bits of the hit; a partial frame is dropped
            for (int k = lane; k < 280; k += 64) {
                const int b = first + k - skip;
                s_hb[k] = k < skip ? 0 : (unsigned char)((r.frame[b >> 3] >> (b & 7)) & 1);
                s_sf[k] = k < skip ? 0.f : sb[b];
            }
            __builtin_amdgcn_wave_barrier();
            int e = 0; unsigned char nib = 0;
            const int blk = lane < 7 ? 0 : lane < 20 ? 1 : 2, ci = lane < 7 ? lane : lane < 20 ? lane - 7 : lane - 20;
            const int L = blk == 0 ? 7 : 13, off = blk == 0 ? 16 : blk == 1 ? 72 : 176;
            if (lane < 33) {
                unsigned char c[8]; float sv[8];
                for (int j = 0; j < 8; j++) { c[j] = s_hb[off + L * j + ci]; sv[j] = s_sf[off + L * j + ci]; }
                if (ecc_level) e = dfm_dev_check(ecc_level, c, sv);
                nib = (unsigned char)((c[0] << 3) | (c[1] << 2) | (c[2] << 1) | c[3]);
            }
            const unsigned long long fixed = __ballot(lane < 33 && e > 0), bad = __ballot(lane < 33 && e < 0);
            if (lane < 7) o->conf[ci] = nib; else if (lane < 20) o->dat1[ci] = nib; else if (lane < 33) o->dat2[ci] = nib;
            if (lane < 35) { unsigned char rb = 0; for (int b = 0; b < 8; b++) rb |= (unsigned char)((s_hb[8 * lane + b] & 1) << b); o->rawbits[lane] = rb; }
            if (lane == 0) {
                o->channel = r.channel; o->frame_in_hit = f; o->mv = r.mv; o->mv_pos = r.mv_pos; o->frm_count = 0.f;     // (positions relative to the channel's start: the host, which knows it)
                o->inv = r.mv < 0.f; o->pad[0] = o->pad[1] = o->pad[2] = 0; o->pad2 = 0;
                o->ecc[0] = ((bad & 0x7Full) ? -1 : 0) | (int)(fixed & 0x7Full);
                o->ecc[1] = (((bad >> 7) & 0x1FFFull) ? -1 : 0) | (int)((fixed >> 7) & 0x1FFFull);
                o->ecc[2] = (((bad >> 20) & 0x1FFFull) ? -1 : 0) | (int)((fixed >> 20) & 0x1FFFull);
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    __threadfence();
    if (lane == 0 && atomicAdd(&done[1], 1u) == gridDim.x - 1) { done[1] = 0; done[0] = end; }
}

__global__ __launch_bounds__(64)
void k_m10_hits(const FrameRec *frames, const float *soft, const float *soft1, const int chk3, const int nbits, const int max_frames, const unsigned *fcount, unsigned *done,
                char *chan_bits, sonde_m10_frame_t *out) {
    constexpr int NBYTES = 101 + 20, NB = NBYTES * 8;
    __shared__ unsigned char s_fr[124];
    const int lane = threadIdx.x;
    const unsigned end = *fcount; unsigned start = done[0];
    if ((int)(end - start) > max_frames) start = end - (unsigned)max_frames;
    for (unsigned i = start; (int)(end - i) > 0; i++) {
        const unsigned idx = i % (unsigned)max_frames;
        const FrameRec &r = frames[idx];
        if ((unsigned)r.channel % gridDim.x != blockIdx.x) continue;          // a channel's records in order, by one workgroup: its bit characters persist from frame to frame
        char *fb = chan_bits + (size_t)r.channel * (NB + 8);
        const int nv = r.nbytes < NB ? r.nbytes : NB;                          // nbytes = valid bits of the hit
        const float *sb = soft + (size_t)idx * nbits, *sb1 = soft1 ? soft1 + (size_t)idx * nbits : nullptr;
        auto bit_at = [&](const int p) -> int {
            // --chk3 (m10mod.c:1476-1479): the bit from both soft values of read_softbit2p, (sb + 0.25 sb1) >= 0
            if (chk3 && sb1) return ((double)sb[p] + 0.25 * (double)sb1[p]) >= 0.0;
            return (r.frame[p >> 3] >> (p & 7)) & 1;
        };
        for (int p = lane; p < nv; p += 64) {
            const int bit = bit_at(p), prev = p == 0 ? 0x30 : bit_at(p - 1);  // differential decoding: 1 = same as the previous bit; the first against '0' (m10mod.c:1484)
            fb[p] = (char)(0x31 ^ (prev ^ bit));
        }
        if (lane == 0) fb[nv] = 0;
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        for (int k = lane; k < 124; k += 64) {
            unsigned v = 0;
            if (k < NBYTES) for (int q = 0; q < 8; q++) if (fb[8 * k + 7 - q] == '1') v |= 1u << q;       // bits2bytes, big endian; anything but '1' counts as 0
            s_fr[k] = (unsigned char)v;
        }
        __builtin_amdgcn_wave_barrier();
        sonde_m10_frame_t *o = out + idx;
        for (int k = lane; k < 124; k += 64) o->frame[k] = s_fr[k];
        if (lane == 0) {
            int aux = s_fr[0] - 0x64;
            if (aux < 0 || aux > 20) aux = 0;
            int c = 0;
            for (int k = 0; k < 99 + aux; k++) {                            // checkM10 (m10mod.c:594-628)
                unsigned char b = s_fr[k];
                b = (unsigned char)((b >> 1) | ((b & 1) << 7));
                b ^= (b >> 2) & 0xFF;
                const int t6 = (c & 1) ^ ((c >> 2) & 1) ^ ((c >> 4) & 1), t7 = ((c >> 1) & 1) ^ ((c >> 3) & 1) ^ ((c >> 5) & 1);
                const int t = (c & 0x3F) | (t6 << 6) | (t7 << 7);
                int sreg = (c >> 7) & 0xFF;
                sreg ^= (sreg >> 2) & 0xFF;
                c = (((c & 0xFF) << 8) | ((b ^ t ^ sreg) & 0xFF)) & 0xFFFF;
            }
            o->channel = r.channel; o->nbits = nv; o->len = 101 + aux; o->cs_calc = (uint32_t)c;
            o->cs_ok = ((uint32_t)((s_fr[99 + aux] << 8) | s_fr[100 + aux]) == (uint32_t)c);
            o->mv = r.mv; o->mv_pos = r.mv_pos;
        }
        __builtin_amdgcn_wave_barrier();
    }
    __threadfence();
    if (lane == 0 && atomicAdd(&done[1], 1u) == gridDim.x - 1) { done[1] = 0; done[0] = end; }
}

extern "C" void sonde_launch_dfm_hits(const FrameRec *frames, const float *soft, int nbits, int max_frames, const unsigned *fcount, unsigned *done, sonde_dfm_frame_t *out,
                                      int ecc_level, int grid, hipStream_t s) {
    hipLaunchKernelGGL(k_dfm_hits, dim3(grid), dim3(64), 0, s, frames, soft, nbits, max_frames, fcount, done, out, ecc_level);
}
extern "C" void sonde_launch_m10_hits(const FrameRec *frames, const float *soft, const float *soft1, int chk3, int nbits, int max_frames, const unsigned *fcount, unsigned *done,
                                      char *chan_bits, sonde_m10_frame_t *out, int grid, hipStream_t s) {
    hipLaunchKernelGGL(k_m10_hits, dim3(grid), dim3(64), 0, s, frames, soft, soft1, chk3, nbits, max_frames, fcount, done, chan_bits, out);
}

extern "C" void sonde_launch_rs41_ecc_batch_n(uint8_t *frames, const int32_t *flen, const unsigned *count, int cap, int level, int32_t *ecc, int32_t *codes, uint8_t *synd,
                                              const uint8_t *gf_exp, const uint8_t *gf_log, hipStream_t s);
extern "C" int sonde_fsk_wait(sonde_fsk_t *f);
extern "C" int sonde_fsk_host_frames(sonde_fsk_t *f, int32_t *out);
extern "C" void sonde_launch_lms6_rs(const void *recs, long long stride, int off_bytes, int off_blen, int off_decoded, int max_frames, const unsigned *count,
                                     unsigned *done, unsigned n, const uint8_t *tab, sonde_lms6_rs_t *out, int grid, hipStream_t s);
int sonde_lms6_rs_tables(DevMem &mem, const uint8_t **tab);
extern "C" int sonde_fsk_dev_view(sonde_fsk_t *f, const float **d_sd, long long *sd_cap, const FskChan **d_chan, int *bits_per_frame, int *n_ch, hipStream_t *stream);
extern "C" int sonde_fsk_dev_reader_done(sonde_fsk_t *f, hipStream_t consumer_stream);
extern "C" int sonde_fsk_dev_view_prev(sonde_fsk_t *f, const float **d_sd, long long *sd_cap, int *bits_per_frame, int *n_ch, int32_t *frames_out);
extern "C" int sonde_fsk_dev_reader_done_prev(sonde_fsk_t *f, hipStream_t consumer_stream);

// ------------------------------------------------------------------------------------------------
// The host side.  One handle for every kind; what differs from kind to kind is a SoftinKind: the record the kernel leaves, the launch, and what a record counts for.
// ------------------------------------------------------------------------------------------------
#include "sonde_pinned.h"
struct SoftinKind {
    size_t rec;                                    // bytes of a record in d_rec / h_rec; 0 = RS41's three arrays (frames / flen / meta + ecc: what k_rs41_ecc_batch reads)
    void (*launch)(sonde_softin_dev *s, const SoftinArgs &a, int nblocks, hipStream_t st);
    void (*tally)(sonde_softin_dev *s, long long n);   // the n records of a call, on the host: into the queue and the counts (null: LMS6, softin_finish_lms6)
};

struct sonde_softin_dev {
    DevMem mem;                                    // every d_ buffer below; the h_ ones are page-locked landing buffers of their own (sonde_pinned.h)
    ~sonde_softin_dev();
    int C = 0, type = SONDE_RS41, cap = 0;
    int head = 0;                                  // records copied to the host without asking how many there are (what a call of a second normally completes)
    const SoftinKind *kind = nullptr;
    int ecc_level = 0;                             // RS41, DFM09
    int opt = 0;                                   // the kind's own switch: M20 skip, dropsonde / RS92 / WxR inv, iMet-54 / Meisei ecc, LMS6 vit, MRZ classify (not -R)
    int opt2 = 0;                                  // MRZ: --ofs; WxR: --pn9
    SoftinArgs args{};
    hipStream_t stream = nullptr;                  // the consumer's own, made by its first call (softin_enqueue): behind the modem's streams, in the order of use
    void *d_state = nullptr;                       // the channels between calls
    unsigned char *d_rec = nullptr; Pinned<unsigned char> h_rec;      // a call's records, and their landing buffer
    unsigned *d_count = nullptr; Pinned<unsigned> h_count;
    int *d_nbits = nullptr; Pinned<int> h_nbits;   // bits per channel of the modem launch a call consumes
    unsigned char *d_hdr = nullptr, *d_gf = nullptr; uint32_t *d_tab = nullptr;
    // SONDE_RS41: the frames as sonde_launch_rs41_ecc_batch_n takes them
    unsigned char *d_frames = nullptr, *d_synd = nullptr; Pinned<unsigned char> h_frames; int *d_flen = nullptr, *d_ecc = nullptr, *d_codes = nullptr; Pinned<int> h_ecc;
    SoftinMeta *d_meta = nullptr; Pinned<SoftinMeta> h_meta;
    // SONDE_LMS6: the channels of a relaunch, the block length each channel has on the device, the decoders' tallies so far
    int l6_auto = 0; int *d_l6_list = nullptr; Pinned<int> h_l6_list, h_l6_len; std::vector<int> l6_len; std::vector<int64_t> l6_ok;
    // RS(255,223) of a round's blocks on the device (sonde_softin_dev_set_lms6_rs; k_lms6_rs, sonde_lms6_rs.hip): a record per block record, and their landing buffer
    bool l6_rs = false; sonde_lms6_rs_t *d_l6_rs = nullptr; Pinned<sonde_lms6_rs_t> h_l6_rs; const uint8_t *d_l6_rs_tab = nullptr;
    // LMS6 / RS92 / iMet-54 / Meisei / MRZ / MTS01: a host decoder per channel (what a sonde collects — calibration rows, configuration words, counters — is per channel)
    std::vector<void *> dec; void (*dec_free)(void *) = nullptr;
    sonde_gps_dev_t *gps = nullptr; bool gps_on = false;   // RS92: the device subset search of fetch_rs92 (sonde_softin_dev_set_rs92_gps), made on first use
    std::vector<unsigned char> q;                  // the records not yet fetched, in the form the kind's tally queues
    long long frames_total = 0, ecc_ok_total = 0, repaired_total = 0, symbols_total = 0, dropped = 0;
    bool pending = false; hipStream_t pend_stream = nullptr;

    template <class T> bool dalloc(T **p, size_t n) { return mem.dalloc(p, n, false) == 0; }
    template <class T> T *chan() { return (T *)d_state; }
    template <class T> T *recs() { return (T *)d_rec; }
    template <class T> const T &landed(long long i) const { return ((const T *)h_rec.data())[i]; }
    template <class T> void queue(const T &r) { const unsigned char *b = (const unsigned char *)&r; q.insert(q.end(), b, b + sizeof(T)); }
    template <class T> T *decoder(int ch) { return (T *)dec[(size_t)ch]; }
};

sonde_softin_dev::~sonde_softin_dev() {
    if (pending && pend_stream) (void)hipStreamSynchronize(pend_stream);
    if (stream) { hipStreamSynchronize(stream); hipStreamDestroy(stream); }
    for (void *d : dec) dec_free(d);
    sonde_gps_dev_destroy(gps);
}

// ---- the launches.  The staged kinds keep the call's soft decisions in LDS: what a call can hold (a modem launch: its capacity; a pushed stream: its length), up to
// M10_STAGE_MAX; beyond that, or where the device refuses the dynamic LDS, the kernel reads them where they lie.  The attribute is a property of (function, device):
// one high-water mark per kernel (Args names it) and device, as in sonde_fsk.hip.
template <class Args>
static void softin_launch_staged(void (*kern)(const Args), Args m, const int nblocks, hipStream_t st) {
    const SoftinArgs &a = m.base;
    long long need = a.nbits_ch ? a.ch_stride : a.nbits;
    if (need > M10_STAGE_MAX || need < 0) need = 0;
    m.stage_cap = (int)need;
    static size_t attr[FSK_MAX_DEV] = {};
    size_t &hw = attr[fsk_cur_dev()];
    const size_t lds = (size_t)need * sizeof(float);
    if (lds > hw) { if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess) hw = lds; else m.stage_cap = 0; }
    hipLaunchKernelGGL(kern, dim3(nblocks), dim3(64), m.stage_cap ? lds : 0, st, m);
}
static void launch_rs41(sonde_softin_dev *s, const SoftinArgs &a, int nblocks, hipStream_t st) {
    hipLaunchKernelGGL(k_softin_rs41, dim3(nblocks), dim3(64), 0, st, a);
    if (s->ecc_level > 0) sonde_launch_rs41_ecc_batch_n(a.frames, a.flen, a.count, a.cap, s->ecc_level, s->d_ecc, s->d_codes, s->d_synd, s->d_gf, s->d_gf + 512, st);
}
static void launch_dfm(sonde_softin_dev *s, const SoftinArgs &a, int nblocks, hipStream_t st) {
    const SoftinDfmArgs d{a, s->chan<SoftinDfmChan>(), s->recs<sonde_dfm_frame_t>(), s->ecc_level};
    hipLaunchKernelGGL(k_softin_dfm, dim3(nblocks), dim3(64), 0, st, d);
}
static void launch_m10(sonde_softin_dev *s, const SoftinArgs &a, int nblocks, hipStream_t st) {
    softin_launch_staged(k_softin_m10, SoftinM10Args{a, s->chan<SoftinM10Chan>(), s->recs<sonde_m10_frame_t>(), 0}, nblocks, st);
}
static void launch_m20(sonde_softin_dev *s, const SoftinArgs &a, int nblocks, hipStream_t st) {
    softin_launch_staged(k_softin_m20, SoftinM20Args{a, s->chan<SoftinM20Chan>(), s->recs<sonde_m20_frame_t>(), 0, s->opt}, nblocks, st);
}
static void launch_rs92(sonde_softin_dev *s, const SoftinArgs &a, int nblocks, hipStream_t st) {
    softin_launch_staged(k_softin_rs92, SoftinRs92Args{a, s->chan<SoftinRs92Chan>(), s->recs<SoftinRs92Rec>(), s->d_gf, 0, s->opt}, nblocks, st);
}
static void launch_imet54(sonde_softin_dev *s, const SoftinArgs &a, int nblocks, hipStream_t st) {
    softin_launch_staged(k_softin_imet54, SoftinImet54Args{a, s->chan<SoftinImet54Chan>(), s->recs<SoftinImet54Rec>(), s->d_tab, 0, s->opt}, nblocks, st);
}
static void launch_meisei(sonde_softin_dev *s, const SoftinArgs &a, int nblocks, hipStream_t st) {
    softin_launch_staged(k_softin_meisei, SoftinMeiseiArgs{a, s->chan<SoftinMeiseiChan>(), s->recs<SoftinMeiseiRec>(), 0, s->opt}, nblocks, st);
}
static void launch_mrz(sonde_softin_dev *s, const SoftinArgs &a, int nblocks, hipStream_t st) {
    softin_launch_staged(k_softin_mrz, SoftinMrzArgs{a, s->chan<SoftinMrzChan>(), s->recs<SoftinMrzRec>(), 0, s->opt, s->opt2}, nblocks, st);
}
static void launch_mts01(sonde_softin_dev *s, const SoftinArgs &a, int nblocks, hipStream_t st) {
    softin_launch_staged(k_softin_mts01, SoftinMts01Args{a, s->chan<SoftinMts01Chan>(), s->recs<SoftinMts01Rec>(), 0}, nblocks, st);
}
static void launch_wxr(sonde_softin_dev *s, const SoftinArgs &a, int nblocks, hipStream_t st) {
    const SoftinWxrArgs d{a, s->chan<SoftinWxrChan>(), s->recs<SoftinWxrRec>(), s->opt, s->opt2};
    hipLaunchKernelGGL(k_softin_wxr, dim3(nblocks), dim3(64), 0, st, d);
}
static void launch_drop(sonde_softin_dev *s, const SoftinArgs &a, int nblocks, hipStream_t st) {
    const SoftinDropArgs d{a, s->chan<SoftinDropChan>(), s->recs<DropFrame>(), s->opt};
    hipLaunchKernelGGL(k_softin_drop, dim3(nblocks), dim3(64), 0, st, d);
}
static void launch_lms6(sonde_softin_dev *s, const SoftinArgs &a, int nblocks, hipStream_t st) {
    const SoftinLms6Args d{a, s->chan<Lms6Chan>(), s->recs<Lms6Block>(), s->opt, s->l6_auto};
    hipLaunchKernelGGL(k_softin_lms6, dim3(nblocks), dim3(64), 0, st, d);
    if (s->l6_rs)                                  // over the round's block records [0, min(*count, cap)) where they lie, before they are copied
        sonde_launch_lms6_rs(s->d_rec, (long long)sizeof(Lms6Block), (int)offsetof(Lms6Block, bytes), (int)offsetof(Lms6Block, blen), -1, s->cap, a.count, nullptr, 0u,
                             s->d_l6_rs_tab, s->d_l6_rs, std::max(1, std::min(nblocks, 1024)), st);
}

// ---- a call's records on the host, a rule per record.  Frames of one channel stay in order: the slots of a call are handed out in completion order per channel, channels interleave.
template <class R, void (*One)(sonde_softin_dev *, const R &)> static void tally_all(sonde_softin_dev *s, long long n) {
    for (long long i = 0; i < n; i++) One(s, s->landed<R>(i));
}
static void tally_rs41(sonde_softin_dev *s, long long n) {
    for (long long i = 0; i < n; i++) {
        sonde_frame_t f; memset(&f, 0, sizeof f);
        const SoftinMeta &m = s->h_meta[i];
        f.channel = m.channel; f.len = m.len; f.nbytes = m.nbytes; f.mv = m.mv; f.mv_pos = (uint32_t)m.hdr_bit;
        f.ecc = s->ecc_level > 0 ? s->h_ecc[i] : 0;
        memcpy(f.frame, s->h_frames.data() + (size_t)i * 518, 518);
        s->queue(f); s->frames_total++;
        if (f.ecc >= 0) s->ecc_ok_total++;
        if (f.ecc > 0) { s->repaired_total++; s->symbols_total += f.ecc; }
    }
}
static void tally_dfm(sonde_softin_dev *s, const sonde_dfm_frame_t &f) {
    s->queue(f); s->frames_total++;
    const bool okf = f.ecc[0] >= 0 && f.ecc[1] >= 0 && f.ecc[2] >= 0;
    if (okf) s->ecc_ok_total++;
    if (okf && (f.ecc[0] > 0 || f.ecc[1] > 0 || f.ecc[2] > 0)) { s->repaired_total++; s->symbols_total += __builtin_popcount((unsigned)f.ecc[0]) + __builtin_popcount((unsigned)f.ecc[1]) + __builtin_popcount((unsigned)f.ecc[2]); }
}
static void tally_m10(sonde_softin_dev *s, const sonde_m10_frame_t &f) { s->queue(f); s->frames_total++; if (f.cs_ok) s->ecc_ok_total++; }
static void tally_m20(sonde_softin_dev *s, const sonde_m20_frame_t &f) { s->queue(f); s->frames_total++; if (f.cs_ok) s->ecc_ok_total++; }
static void tally_drop(sonde_softin_dev *s, const DropFrame &g) {
    sonde_drop_frame_t f; memset(&f, 0, sizeof f);
    f.channel = g.channel; f.nraw = g.nraw; f.complete = g.complete; f.err94 = g.err94; f.err41 = g.err41; f.sample = g.sample;
    memcpy(f.bytes, g.bytes, sizeof f.bytes);
    s->queue(f); s->frames_total++;
    // print_frame's type choice and frm_ok (rd94rd41drop.c:1028-1038, :1213): more than two failing RD41 blocks = RD94
    if (__builtin_popcount((unsigned)g.err41) > 2 ? g.err94 == 0 : g.err41 == 0) s->ecc_ok_total++;
}
static void tally_rs92(sonde_softin_dev *s, const SoftinRs92Rec &r) {
    if (r.channel < 0 || r.channel >= s->C) return;
    s->queue(r); s->frames_total++;
    if (r.ec >= 0) s->ecc_ok_total++;
    if (r.ec > 0) { s->repaired_total++; s->symbols_total += r.ec; }
}
static void tally_imet54(sonde_softin_dev *s, const SoftinImet54Rec &r) {
    if (r.channel < 0 || r.channel >= s->C) return;
    s->queue(r); s->frames_total++;
    // the JSON rule without the status bits (imet54mod.c:583): frm_ok and a check sum good, or every codeword of the standard frame clean
    if (r.ecc_frm >= 0 && (r.crc_std || r.crc_cont || r.ecc_std == 0)) s->ecc_ok_total++;
    if (r.ecc_frm > 0) { s->repaired_total++; s->symbols_total += r.ecc_frm; }
}
static void tally_meisei(sonde_softin_dev *s, const SoftinMeiseiRec &r) {
    if (r.channel < 0 || r.channel >= s->C) return;
    s->queue(r); s->frames_total++;
    int bad = 0, fixed = 0;
    for (int k = 0; k < MEISEI_BLOCKS; k++) { if (r.block_err[k] >= 0xE) bad++; else fixed += r.block_err[k]; }
    if (!bad) s->ecc_ok_total++;
    if (fixed) { s->repaired_total++; s->symbols_total += fixed; }
}
static void tally_mrz(sonde_softin_dev *s, const SoftinMrzRec &r) {
    if (r.channel < 0 || r.channel >= s->C) return;
    s->queue(r); s->frames_total++;
    if (r.crc_ok) s->ecc_ok_total++;
}
static void tally_mts01(sonde_softin_dev *s, const SoftinMts01Rec &r) {
    if (r.channel < 0 || r.channel >= s->C) return;
    s->queue(r); s->frames_total++;
    if (r.crc_ok) s->ecc_ok_total++;
}
static void tally_wxr(sonde_softin_dev *s, const SoftinWxrRec &r) {
    if (r.channel < 0 || r.channel >= s->C) return;
    s->queue(r); s->frames_total++;
    if (r.chk_ok) s->ecc_ok_total++;
}

static const SoftinKind *softin_kind(const int type) {
    static const SoftinKind rs41{0, launch_rs41, tally_rs41}, dfm{sizeof(sonde_dfm_frame_t), launch_dfm, tally_all<sonde_dfm_frame_t, tally_dfm>},
        m10{sizeof(sonde_m10_frame_t), launch_m10, tally_all<sonde_m10_frame_t, tally_m10>}, m20{sizeof(sonde_m20_frame_t), launch_m20, tally_all<sonde_m20_frame_t, tally_m20>},
        drop{sizeof(DropFrame), launch_drop, tally_all<DropFrame, tally_drop>}, lms6{sizeof(Lms6Block), launch_lms6, nullptr},
        rs92{sizeof(SoftinRs92Rec), launch_rs92, tally_all<SoftinRs92Rec, tally_rs92>}, imet54{sizeof(SoftinImet54Rec), launch_imet54, tally_all<SoftinImet54Rec, tally_imet54>},
        meisei{sizeof(SoftinMeiseiRec), launch_meisei, tally_all<SoftinMeiseiRec, tally_meisei>},
        mrz{sizeof(SoftinMrzRec), launch_mrz, tally_all<SoftinMrzRec, tally_mrz>}, mts01{sizeof(SoftinMts01Rec), launch_mts01, tally_all<SoftinMts01Rec, tally_mts01>},
        wxr{sizeof(SoftinWxrRec), launch_wxr, tally_all<SoftinWxrRec, tally_wxr>};
    switch (type) {
        case SONDE_RS41: return &rs41;     case SONDE_DFM09: return &dfm;   case SONDE_M10: return &m10;       case SONDE_M20: return &m20;       case SONDE_RD94RD41: return &drop;
        case SONDE_LMS6: return &lms6;     case SONDE_RS92: return &rs92;   case SONDE_IMET54: return &imet54; case SONDE_MEISEI: return &meisei;
        case SONDE_MRZ: return &mrz;       case SONDE_MTS01: return &mts01;   case SONDE_WXR301: return &wxr;
    }
    return nullptr;
}

// A new consumer of `type`: what every kind has.  A call can hold per_cap records per channel + 16 and normally completes per_head per channel + 16 (include/sonde_fsk.h);
// every channel starts as *init.  What only the kind has (header, tables, host decoders, options) is the caller's.
static int softin_new(const int32_t n_channels, const int type, const int per_cap, const int per_head, const float ths, const int32_t invert_stream,
                      const void *init, const size_t chan_bytes, sonde_softin_dev **out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { fprintf(stderr, "libsonde_hip: no usable HIP device (the batched soft-bit framer has no CPU fallback)\n"); return SONDE_E_NOGPU; }
    std::unique_ptr<sonde_softin_dev> owner(new sonde_softin_dev());
    sonde_softin_dev *s = owner.get();
    s->C = n_channels; s->type = type; s->kind = softin_kind(type);
    s->cap = per_cap * n_channels + 16; s->head = std::min(s->cap, per_head * n_channels + 16);
    const size_t C = (size_t)n_channels, cap = (size_t)s->cap;
    std::vector<unsigned char> img(C * chan_bytes);
    for (size_t c = 0; c < C; c++) memcpy(img.data() + c * chan_bytes, init, chan_bytes);
    unsigned char *state = nullptr;
    bool ok = s->dalloc(&state, img.size()) && s->dalloc(&s->d_count, 2) && s->h_count.alloc(2) && s->dalloc(&s->d_nbits, C) && s->h_nbits.alloc(C)
           && hipMemcpy(state, img.data(), img.size(), hipMemcpyHostToDevice) == hipSuccess;
    if (ok && s->kind->rec) ok = s->dalloc(&s->d_rec, cap * s->kind->rec) && s->h_rec.alloc(cap * s->kind->rec);
    if (!ok) return SONDE_E_NOMEM;
    s->d_state = state;
    SoftinArgs &a = s->args;
    a.n_ch = n_channels; a.inv_in = invert_stream ? 1 : 0; a.ths = ths; a.count = s->d_count; a.cap = s->cap;
    *out = owner.release();
    return 0;
}
// the option checks of a kind's host decoder, before the device is touched; and a decoder per channel
template <class D, class O> static int softin_probe(const O *o, int (*create)(const O *, D **), void (*destroy)(D *)) {
    D *probe = nullptr;
    const int rc = create(o, &probe);
    if (!rc) destroy(probe);
    return rc;
}
template <class D, class O, void (*Destroy)(D *)> static int softin_decoders(sonde_softin_dev *s, const O *o, int (*create)(const O *, D **)) {
    s->dec_free = [](void *d) { Destroy((D *)d); };
    for (int c = 0; c < s->C; c++) {
        D *d = nullptr;
        if (create(o, &d)) return SONDE_E_NOMEM;
        s->dec.push_back(d);
    }
    return 0;
}
// the end of every create: what the kind added is in place (ok) and the handle is the caller's, or it goes
static int softin_created(sonde_softin_dev *s, const bool ok, sonde_softin_dev **out) {
    std::unique_ptr<sonde_softin_dev> owner(s);
    (void)hipGetLastError();
    if (!ok) return SONDE_E_NOMEM;
    *out = owner.release();
    return 0;
}

extern "C" {

int sonde_softin_dev_create(int32_t n_channels, int32_t sonde_type, int32_t ecc_level, int32_t invert_stream, int32_t opt_inv, int32_t opt_auto, sonde_softin_dev_t **out) {
    if (!out || n_channels < 1 || (sonde_type != SONDE_RS41 && sonde_type != SONDE_DFM09 && sonde_type != SONDE_M10 && sonde_type != SONDE_M20 && sonde_type != SONDE_RD94RD41) || ecc_level < 0 || ecc_level > 2) return SONDE_E_ARG;
    // frames a call of about a second can complete per channel: RS41 two, DFM09 six (280 bits at 1250 b/s), M10 two (one per second; the rest of the second is skipped),
    // dropsondes three (two a second), M20 four (without the skip a frame can complete every 32 + 2640 symbols of the 9600 a second)
    const int per_cap = sonde_type == SONDE_DFM09 ? 8 : sonde_type == SONDE_RD94RD41 || sonde_type == SONDE_M20 ? 4 : 2;
    const int per_head = sonde_type == SONDE_DFM09 ? 5 : sonde_type == SONDE_RD94RD41 ? 2 : 1;
    const float ths = sonde_type == SONDE_M10 || sonde_type == SONDE_M20 ? 0.8f : 0.7f;
    const int inv = opt_inv ? 1 : 0;
    sonde_softin_dev *s = nullptr;
    auto make = [&](const void *c, const size_t bytes) { return softin_new(n_channels, sonde_type, per_cap, per_head, ths, invert_stream, c, bytes, &s); };
    int rc = 0;
    if (sonde_type == SONDE_RS41) {
        SoftinChan c; memset(&c, 0, sizeof c);
        c.inv = inv; memcpy(c.frame, sonde::kRs41HeaderBytes, 8);
        rc = make(&c, sizeof c);
    } else if (sonde_type == SONDE_DFM09) {
        SoftinDfmChan c; memset(&c, 0, sizeof c);
        static const char kDfmHdr[] = "0100010111001111";                                 // dfm09mod.c:1503-1506: the header's 16 bits in front of the first frame of a hit
        c.inv = inv; c.dpos = 16; for (int i = 0; i < 16; i++) c.dhb[i] = (unsigned char)(kDfmHdr[i] & 1);
        rc = make(&c, sizeof c);
    } else if (sonde_type == SONDE_M10) {
        SoftinM10Chan c; memset(&c, 0, sizeof c);
        c.inv = inv; c.mbit0 = '0';
        rc = make(&c, sizeof c);
    } else if (sonde_type == SONDE_M20) {
        SoftinM20Chan c; memset((void *)&c, 0, sizeof c);
        c.inv = inv; c.mbit0 = '0';
        rc = make(&c, sizeof c);
    } else {
        SoftinDropChan c; memset(&c, 0, sizeof c);
        c.pos = DROP_HEADLEN; for (int i = 0; i < DROP_HEADLEN; i++) c.frame[i] = (unsigned char)((DROP_HDR40 >> (DROP_HEADLEN - 1 - i)) & 1);
        rc = make(&c, sizeof c);
    }
    if (rc) return rc;
    s->ecc_level = ecc_level; s->args.opt_auto = opt_auto ? 1 : 0;
    s->opt = sonde_type == SONDE_M20 ? 1 : sonde_type == SONDE_RD94RD41 ? (invert_stream ? 1 : 0) ^ inv : 0;
    unsigned char hdr[136];
    memset(hdr, 0, sizeof hdr);
    if (sonde_type == SONDE_RS41) { memcpy(hdr, sonde::kRs41Header, 64); memcpy(hdr + 64, sonde::kRs41HeaderBytes, 8); memcpy(hdr + 72, sonde::kRs41Mask, 64); }
    else memcpy(hdr, sonde_type == SONDE_DFM09 ? sonde::kDfmRawHeader : sonde::kM10RawHeader, 32);
    bool ok = s->dalloc(&s->d_hdr, sizeof hdr) && hipMemcpy(s->d_hdr, hdr, sizeof hdr, hipMemcpyHostToDevice) == hipSuccess;
    if (ok && sonde_type == SONDE_RS41) {
        const size_t cap = (size_t)s->cap;
        ok = s->dalloc(&s->d_frames, cap * 518) && s->dalloc(&s->d_gf, 768) && s->dalloc(&s->d_synd, cap * 48) && s->dalloc(&s->d_flen, cap) && s->dalloc(&s->d_ecc, cap)
          && s->dalloc(&s->d_codes, cap * 2) && s->dalloc(&s->d_meta, cap) && s->h_ecc.alloc(cap) && s->h_meta.alloc(cap) && s->h_frames.alloc(cap * 518)
          && hipMemcpy(s->d_gf, sonde::gf_exp_table(), 512, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(s->d_gf + 512, sonde::gf_log_table(), 256, hipMemcpyHostToDevice) == hipSuccess
          && hipMemset(s->d_ecc, 0, cap * 4) == hipSuccess;
        SoftinArgs &a = s->args;
        a.chan = s->chan<SoftinChan>(); a.frames = s->d_frames; a.flen = s->d_flen; a.meta = s->d_meta;
    }
    s->args.hdr = s->d_hdr;
    return softin_created(s, ok, out);
}

int sonde_softin_dev_create_lms6(int32_t n_channels, const sonde_lms6_opts_t *opts, int32_t invert_stream, sonde_softin_dev_t **out) {
    if (!out || n_channels < 1 || !opts) return SONDE_E_ARG;
    sonde_lms6_opts_t o = *opts;
    if (o.json) { if (!o.ecc) o.ecc = 1; if (!o.vit) o.vit = 1; }                              // lms6Xmod.c:1153-1157
    if (o.vit != 1 && o.vit != 2) return SONDE_E_ARG;                                          // the algebraic decoder alone has no device form
    if (o.ecc == 3) return SONDE_E_ARG;                                                        // --ecc3 needs the second soft value of a sample-rate demodulator
    sonde_lms6_dec_t *probe = nullptr;                                                         // the option checks of the host decoder, before the device is touched
    if (const int rc = sonde_lms6_dec_create(&o, &probe)) return rc;
    const int len0 = sonde_lms6_dec_block_bits(probe) + LMS6_BLOCKSTART;
    sonde_lms6_dec_destroy(probe);
    sonde_softin_dev *s = nullptr;
    Lms6Chan c; memset((void *)&c, 0, sizeof c);
    c.pos = LMS6_BLOCKSTART; c.rawblk_len = len0;
    // blocks a call can hold over all channels (sonde_fsk.h): a channel completes at most two in a second of 4800 soft bits
    if (const int rc = softin_new(n_channels, SONDE_LMS6, 4, 1, 0.7f, invert_stream, &c, sizeof c, &s)) return rc;
    const size_t C = (size_t)n_channels;
    s->opt = o.vit; s->l6_auto = o.typ == 0;
    s->l6_len.assign(C, len0); s->l6_ok.assign(C, 0);
    const bool ok = softin_decoders<sonde_lms6_dec_t, sonde_lms6_opts_t, sonde_lms6_dec_destroy>(s, &o, sonde_lms6_dec_create) == 0
                 && s->dalloc(&s->d_l6_list, C) && s->h_l6_list.alloc(C) && s->h_l6_len.alloc(C) && s->dalloc(&s->d_hdr, 64)
                 && hipMemcpy(s->d_hdr, sonde_lms6_raw_header(), 64, hipMemcpyHostToDevice) == hipSuccess;
    s->args.hdr = s->d_hdr;
    return softin_created(s, ok, out);
}

int sonde_softin_dev_create_rs92(int32_t n_channels, const sonde_rs92_opts_t *opts, int32_t invert_stream, sonde_softin_dev_t **out) {
    if (!out || n_channels < 1 || !opts) return SONDE_E_ARG;
    if (opts->gps_verbose == 8 || opts->dbg) return SONDE_E_ARG;                               // -gg / --dbg: lines without a bound per frame
    if (const int rc = softin_probe(opts, sonde_rs92_dec_create, sonde_rs92_dec_destroy)) return rc;
    sonde_softin_dev *s = nullptr;
    SoftinRs92Chan c; memset((void *)&c, 0, sizeof c);
    // frames a call can hold over all channels (sonde_fsk.h): a channel completes one per 4740 symbols at the least; a frame a second and channel
    if (const int rc = softin_new(n_channels, SONDE_RS92, 4, 1, 0.8f, invert_stream, &c, sizeof c, &s)) return rc;
    s->opt = opts->inv ? 1 : 0;
    const bool ok = softin_decoders<sonde_rs92_dec_t, sonde_rs92_opts_t, sonde_rs92_dec_destroy>(s, opts, sonde_rs92_dec_create) == 0 && s->dalloc(&s->d_gf, 768)
                 && hipMemcpy(s->d_gf, sonde::gf_exp_table(), 512, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(s->d_gf + 512, sonde::gf_log_table(), 256, hipMemcpyHostToDevice) == hipSuccess;
    return softin_created(s, ok, out);
}

int sonde_softin_dev_create_imet54(int32_t n_channels, const sonde_imet54_opts_t *opts, int32_t invert_stream, sonde_softin_dev_t **out) {
    if (!out || n_channels < 1 || !opts) return SONDE_E_ARG;
    if (const int rc = softin_probe(opts, sonde_imet54_dec_create, sonde_imet54_dec_destroy)) return rc;
    sonde_softin_dev *s = nullptr;
    SoftinImet54Chan c; memset((void *)&c, 0, sizeof c);
    c.inv = opts->inv ? 1 : 0;
    // frames a call can hold over all channels (sonde_fsk.h): a channel completes one per 2240 symbols at the most; a frame a second and channel
    if (const int rc = softin_new(n_channels, SONDE_IMET54, 4, 1, 0.8f, invert_stream, &c, sizeof c, &s)) return rc;
    s->opt = (opts->ecc || opts->json) ? 1 : 0;                                                // --json implies --ecc (imet54mod.c:899)
    s->args.opt_auto = opts->aut ? 1 : 0;
    std::vector<uint32_t> tab(IMET54_TAB_N);
    imet54_crc_table(tab.data());
    const bool ok = softin_decoders<sonde_imet54_dec_t, sonde_imet54_opts_t, sonde_imet54_dec_destroy>(s, opts, sonde_imet54_dec_create) == 0 && s->dalloc(&s->d_tab, IMET54_TAB_N)
                 && hipMemcpy(s->d_tab, tab.data(), IMET54_TAB_N * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
    return softin_created(s, ok, out);
}

int sonde_softin_dev_create_meisei(int32_t n_channels, const sonde_meisei_opts_t *opts, int32_t invert_stream, sonde_softin_dev_t **out) {
    if (!out || n_channels < 1 || !opts) return SONDE_E_ARG;
    if (const int rc = softin_probe(opts, sonde_meisei_dec_create, sonde_meisei_dec_destroy)) return rc;
    sonde_softin_dev *s = nullptr;
    SoftinMeiseiChan c; memset((void *)&c, 0, sizeof c);
    // frames a call can hold over all channels (sonde_fsk.h): a channel completes one per 1200 half symbols at the most; two frames a second and channel
    if (const int rc = softin_new(n_channels, SONDE_MEISEI, 4, 2, 0.8f, invert_stream, &c, sizeof c, &s)) return rc;
    s->opt = (opts->ecc || opts->json) ? 1 : 0;                                                // --json implies --ecc (sonde_meisei.h)
    const bool ok = softin_decoders<sonde_meisei_dec_t, sonde_meisei_opts_t, sonde_meisei_dec_destroy>(s, opts, sonde_meisei_dec_create) == 0;
    return softin_created(s, ok, out);
}

int sonde_softin_dev_create_mrz(int32_t n_channels, const sonde_mrz_opts_t *opts, int32_t invert_stream, sonde_softin_dev_t **out) {
    if (!out || n_channels < 1 || !opts) return SONDE_E_ARG;
    if (const int rc = softin_probe(opts, sonde_mrz_dec_create, sonde_mrz_dec_destroy)) return rc;
    sonde_softin_dev *s = nullptr;
    SoftinMrzChan c; memset((void *)&c, 0, sizeof c);
    c.inv = opts->inv ? 1 : 0; c.bitfrm_len = MRZ_MAXBITS;
    // frames a call can hold over all channels (sonde_fsk.h): a channel completes one per 44 + 2 (384 - 22) = 768 half symbols at the most, so seven in two seconds
    // at 2400; a second normally completes three at the most
    if (const int rc = softin_new(n_channels, SONDE_MRZ, 8, 3, 0.82f, invert_stream, &c, sizeof c, &s)) return rc;
    s->opt = opts->raw == 2 ? 0 : 1;                                                           // -R: the reference never looks at the bytes (mp3h1mod.c:793-797)
    s->opt2 = opts->bits_ofs_given ? opts->bits_ofs : 8;
    s->args.opt_auto = opts->aut ? 1 : 0;
    const bool ok = softin_decoders<sonde_mrz_dec_t, sonde_mrz_opts_t, sonde_mrz_dec_destroy>(s, opts, sonde_mrz_dec_create) == 0;
    return softin_created(s, ok, out);
}

int sonde_softin_dev_create_mts01(int32_t n_channels, const sonde_mts01_opts_t *opts, int32_t invert_stream, sonde_softin_dev_t **out) {
    if (!out || n_channels < 1 || !opts) return SONDE_E_ARG;
    if (const int rc = softin_probe(opts, sonde_mts01_dec_create, sonde_mts01_dec_destroy)) return rc;
    sonde_softin_dev *s = nullptr;
    SoftinMts01Chan c; memset((void *)&c, 0, sizeof c);
    // frames a call can hold over all channels (sonde_fsk.h): a channel completes one per 32 + 1048 = 1080 symbols at the most; a frame a second and channel
    if (const int rc = softin_new(n_channels, SONDE_MTS01, 4, 1, 0.8f, invert_stream, &c, sizeof c, &s)) return rc;
    const bool ok = softin_decoders<sonde_mts01_dec_t, sonde_mts01_opts_t, sonde_mts01_dec_destroy>(s, opts, sonde_mts01_dec_create) == 0;
    return softin_created(s, ok, out);
}

static_assert(sizeof(SoftinWxrRec) == sizeof(sonde_wxr_softin_rec_t) && sizeof(SoftinWxrRec) == 176, "the WxR record is the C ABI's");
static_assert(offsetof(SoftinWxrRec, hdr_bit) == offsetof(sonde_wxr_softin_rec_t, hdr_bit) && offsetof(SoftinWxrRec, raw) == offsetof(sonde_wxr_softin_rec_t, raw)
           && offsetof(SoftinWxrRec, x) == offsetof(sonde_wxr_softin_rec_t, x) && offsetof(SoftinWxrRec, chkval) == offsetof(sonde_wxr_softin_rec_t, chkval)
           && offsetof(SoftinWxrRec, chk_ok) == offsetof(sonde_wxr_softin_rec_t, chk_ok) && offsetof(SoftinWxrRec, frid) == offsetof(sonde_wxr_softin_rec_t, frid)
           && offsetof(SoftinWxrRec, sn) == offsetof(sonde_wxr_softin_rec_t, sn) && offsetof(SoftinWxrRec, cnt) == offsetof(sonde_wxr_softin_rec_t, cnt), "field for field");

int sonde_softin_dev_create_wxr(int32_t n_channels, const sonde_wxr_softin_opts_t *opts, int32_t invert_stream, sonde_softin_dev_t **out) {
    if (!out || n_channels < 1 || !opts) return SONDE_E_ARG;
    sonde_softin_dev *s = nullptr;
    SoftinWxrChan c; memset((void *)&c, 0, sizeof c);                                          // the ring holds no bit at all
    // frames a call can hold over all channels (sonde_fsk.h): a call of n bits completes at most n / 552 + 1 per channel, ten for a second at 5000 Bd; twenty for
    // two seconds.  A second normally completes nine.
    if (const int rc = softin_new(n_channels, SONDE_WXR301, 20, 10, 0.f, invert_stream, &c, sizeof c, &s)) return rc;
    s->opt = (invert_stream ? 1 : 0) ^ (opts->invert ? 1 : 0);                                 // the two inversions cancel each other, as for the dropsondes
    s->opt2 = opts->pn9 ? 1 : 0;
    return softin_created(s, true, out);
}

int sonde_softin_dev_rs92_load_ephemeris(sonde_softin_dev_t *s, const char *path) {
    if (!s || s->type != SONDE_RS92 || !path) return SONDE_E_ARG;
    for (int c = 0; c < s->C; c++) { const int rc = sonde_rs92_dec_load_ephemeris(s->decoder<sonde_rs92_dec_t>(c), path); if (rc) return rc; }
    return 0;
}
int sonde_softin_dev_rs92_load_almanac(sonde_softin_dev_t *s, const char *path) {
    if (!s || s->type != SONDE_RS92 || !path) return SONDE_E_ARG;
    for (int c = 0; c < s->C; c++) { const int rc = sonde_rs92_dec_load_almanac(s->decoder<sonde_rs92_dec_t>(c), path); if (rc) return rc; }
    return 0;
}

void sonde_softin_dev_destroy(sonde_softin_dev_t *s) { delete s; }

// one pass of the framer (and rs41_ecc() over the frames it completes) over the channels of ch_list (null: all)
static int softin_pass(sonde_softin_dev *s, hipStream_t st, const int nblocks, const int *ch_list) {
    SoftinArgs a = s->args;
    a.ch_list = ch_list;
    HIPCHK(hipMemsetAsync(a.count, 0, 4, st));
    s->kind->launch(s, a, nblocks, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s->h_count.data(), a.count, 4, hipMemcpyDeviceToHost, st));
    return 0;
}
// records [from, to) of the call to the host
static int softin_copy(sonde_softin_dev *s, hipStream_t st, const int from, const int to) {
    if (to <= from) return 0;
    const size_t n = (size_t)(to - from), rec = s->kind->rec;
    if (s->l6_rs) HIPCHK(hipMemcpyAsync(s->h_l6_rs.data() + from, s->d_l6_rs + from, n * sizeof(sonde_lms6_rs_t), hipMemcpyDeviceToHost, st));
    if (rec) HIPCHK(hipMemcpyAsync(s->h_rec.data() + from * rec, s->d_rec + from * rec, n * rec, hipMemcpyDeviceToHost, st));
    else {
        HIPCHK(hipMemcpyAsync(s->h_meta.data() + from, s->d_meta + from, n * sizeof(SoftinMeta), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(s->h_ecc.data() + from, s->d_ecc + from, n * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(s->h_frames.data() + (size_t)from * 518, s->d_frames + (size_t)from * 518, n * 518, hipMemcpyDeviceToHost, st));   // 518 bytes per frame and second: not the soft decisions
    }
    return 0;
}
// LMS6: every block of the round goes through its channel's host decoder (RS(255,223), frame sync, CRC, text).  With auto detection a channel stopped at its block
// (Lms6Block.more): the decoder says how long the next block is (lms6Xmod.c:1436-1462), the channel's rawblk_len on the device follows, and the channels with input
// left are launched again until the call is consumed.
static int softin_finish_lms6(sonde_softin_dev *s, hipStream_t st, long long n) {
    for (;;) {
        int nlist = 0;
        for (long long i = 0; i < n; i++) {
            const Lms6Block &b = s->landed<Lms6Block>(i);
            if (b.channel < 0 || b.channel >= s->C) continue;
            sonde_lms6_dec_t *d = s->decoder<sonde_lms6_dec_t>(b.channel);
            sonde_lms6_softin_t r; memset(&r, 0, sizeof r);
            const float nanv = __builtin_nanf("");             // dsp_t stays zeroed with soft input: frm_rate and the elapsed time are 0 / 0
            const int len = s->l6_rs ? sonde_lms6_dec_block_rs(d, b.bytes, b.blen, b.pos, b.mv, nanv, (double)nanv, &s->h_l6_rs[i], r.text, sizeof r.text)
                                     : sonde_lms6_dec_block_bytes(d, b.bytes, b.blen, b.pos, b.mv, nanv, (double)nanv, r.text, sizeof r.text);
            if (len < 0) return len;
            r.channel = b.channel; r.type = sonde_lms6_dec_type(d, nullptr); r.mv = b.mv; r.text_len = len; r.hdr_bit = b.hdr_bit; r.blen = b.blen; r.err = b.err;
            s->queue(r);
            s->frames_total++;
            int64_t ok = 0;
            (void)sonde_lms6_dec_counts(d, nullptr, &ok);                 // the decoder's own tally of CRC-good frames, whatever the output form
            s->ecc_ok_total += ok - s->l6_ok[(size_t)b.channel]; s->l6_ok[(size_t)b.channel] = ok;
            const int want = sonde_lms6_dec_block_bits(d) + LMS6_BLOCKSTART;
            if (want != s->l6_len[(size_t)b.channel]) {
                s->l6_len[(size_t)b.channel] = want; s->h_l6_len[b.channel] = want;
                HIPCHK(hipMemcpyAsync(&s->chan<Lms6Chan>()[b.channel].rawblk_len, &s->h_l6_len[b.channel], sizeof(int), hipMemcpyHostToDevice, st));
            }
            if (b.more && nlist < s->C) s->h_l6_list[nlist++] = b.channel;
        }
        if (!nlist) return 0;
        HIPCHK(hipMemcpyAsync(s->d_l6_list, s->h_l6_list.data(), (size_t)nlist * sizeof(int), hipMemcpyHostToDevice, st));
        { const int rc = softin_pass(s, st, nlist, s->d_l6_list); if (rc) return rc; }
        { const int rc = softin_copy(s, st, 0, std::min(nlist, s->cap)); if (rc) return rc; }
        HIPCHK(hipStreamSynchronize(st));
        n = std::min<long long>(s->h_count[0], std::min(nlist, s->cap));
    }
}

static int softin_own_stream(sonde_softin_dev *s) {
    if (!s->stream) HIPCHK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    return 0;
}
// enqueue a call: the framer over what args.sd / nbits describe, the block code, the counter and the records a call normally completes (`head`) on their way to the host
static int softin_enqueue(sonde_softin_dev *s) {
    if (s->pending) return SONDE_E_ARG;
    { const int rc = softin_pass(s, s->stream, s->C, nullptr); if (rc) return rc; }
    { const int rc = softin_copy(s, s->stream, 0, s->head); if (rc) return rc; }
    s->pending = true; s->pend_stream = s->stream;
    return 0;
}
// the other half: wait, take what the head did not cover, queue the frames and add up the tallies
static int softin_finish(sonde_softin_dev *s) {
    if (!s->pending) return 0;
    hipStream_t st = s->pend_stream;
    s->pending = false;
    HIPCHK(hipStreamSynchronize(st));
    long long n = s->h_count[0];
    if (n > s->cap) { s->dropped += n - s->cap; n = s->cap; }
    const int have = (int)std::min<long long>(n, s->head);
    if (n > have) { const int rc = softin_copy(s, st, have, (int)n); if (rc) return rc; HIPCHK(hipStreamSynchronize(st)); }
    if (s->type == SONDE_LMS6) return softin_finish_lms6(s, st, n);
    s->kind->tally(s, n);
    return 0;
}

// A launch of the modem as this call's input: its soft decisions where that launch left them (d_sd, `cap` a channel), the bits per channel — h_nbits holds the
// channels' frame counts, bpf bits each — uploaded; then the call is enqueued.  LMS6 with auto detection launches again per completed block and reads the soft
// decisions each time: its call is completed here, so that the point of the stream the modem is told about next lies behind every read — whatever the caller
// does before sonde_softin_dev_collect.
static int softin_consume_launch(sonde_softin_dev *s, const float *d_sd, const long long cap, const int bpf) {
    for (int c = 0; c < s->C; c++) s->h_nbits[c] = s->h_nbits[c] > 0 ? s->h_nbits[c] * bpf : 0;
    HIPCHK(hipMemcpyAsync(s->d_nbits, s->h_nbits.data(), (size_t)s->C * sizeof(int), hipMemcpyHostToDevice, s->stream));
    SoftinArgs &a = s->args;
    a.sd = d_sd; a.ch_stride = cap; a.nbits_ch = s->d_nbits; a.nbits = 0;
    { const int rc = softin_enqueue(s); if (rc) return rc; }
    if (s->type == SONDE_LMS6 && s->l6_auto) return softin_finish(s);
    return 0;
}

// Submit waits for the modem's launch (sonde_fsk_wait: its channels' frame counts come from the host's copy of the records, and whatever the modem had to repeat is
// repeated by then), then enqueues the consumer's kernels and the copies of its frames on the consumer's OWN stream and returns; collect waits for them.  In between
// the modem can be given its next second (sonde_fsk_submit_device): the modem keeps the soft decisions of two launches (they alternate between two buffers), so the
// consumer of second k runs beside the modem of second k + 1.  Collect before the modem's launch after that.
int sonde_softin_dev_submit_fsk(sonde_softin_dev_t *s, sonde_fsk_t *modem) {
    if (!s || !modem) return SONDE_E_ARG;
    { const int rc = softin_finish(s); if (rc) return rc; }
    { const int rc = softin_own_stream(s); if (rc) return rc; }
    const float *d_sd = nullptr; long long cap = 0; const FskChan *d_chan = nullptr; int bpf = 0, nch = 0; hipStream_t ms = nullptr;
    { const int rc = sonde_fsk_wait(modem); if (rc) return rc; }
    { const int rc = sonde_fsk_dev_view(modem, &d_sd, &cap, &d_chan, &bpf, &nch, &ms); if (rc) return rc; }
    if (nch != s->C) return SONDE_E_ARG;
    { const int rc = sonde_fsk_host_frames(modem, s->h_nbits.data()); if (rc) return rc; }
    { const int rc = softin_consume_launch(s, d_sd, cap, bpf); if (rc) return rc; }
    // the modem's launch that reuses this buffer of soft decisions (the next but one) waits for the consumer's kernels: submitting the modem twice before
    // sonde_softin_dev_collect is slower, not wrong
    return sonde_fsk_dev_reader_done(modem, s->stream);
}
int sonde_softin_dev_push_fsk(sonde_softin_dev_t *s, sonde_fsk_t *modem) {
    const int rc = sonde_softin_dev_submit_fsk(s, modem);
    return rc ? rc : softin_finish(s);
}
// The consumer over the launch BEFORE the one the modem has in flight: for a caller that hands the modem its next second first (sonde_fsk_wait (k - 1),
// sonde_fsk_submit_device (k), then this for k - 1) — the modem's stream never waits for the host's decoder bookkeeping.  Nothing waits here; with no launch in
// flight this is sonde_softin_dev_submit_fsk.
int sonde_softin_dev_submit_fsk_behind(sonde_softin_dev_t *s, sonde_fsk_t *modem) {
    if (!s || !modem) return SONDE_E_ARG;
    { const int rc = softin_finish(s); if (rc) return rc; }
    { const int rc = softin_own_stream(s); if (rc) return rc; }
    const float *d_sd = nullptr; long long cap = 0; int bpf = 0, nch = s->C;
    const int have = sonde_fsk_dev_view_prev(modem, &d_sd, &cap, &bpf, &nch, s->h_nbits.data());
    if (have < 0) return have;
    if (have == 0) return sonde_softin_dev_submit_fsk(s, modem);
    if (nch != s->C) return SONDE_E_ARG;
    // (the modem's launch in flight is the one that overwrites these soft decisions next)
    { const int rc = softin_consume_launch(s, d_sd, cap, bpf); if (rc) return rc; }
    return sonde_fsk_dev_reader_done_prev(modem, s->stream);
}
int sonde_softin_dev_collect(sonde_softin_dev_t *s) {
    if (!s) return SONDE_E_ARG;
    return softin_finish(s);
}

int sonde_softin_dev_push_device(sonde_softin_dev_t *s, const float *d_soft, int64_t ch_stride, int32_t n_bits) {
    if (!s || !d_soft || n_bits < 0 || ch_stride < n_bits) return SONDE_E_ARG;
    { const int rc = softin_finish(s); if (rc) return rc; }
    { const int rc = softin_own_stream(s); if (rc) return rc; }
    SoftinArgs &a = s->args;
    a.sd = d_soft; a.ch_stride = ch_stride; a.nbits_ch = nullptr; a.nbits = n_bits;
    { const int rc = softin_enqueue(s); if (rc) return rc; }
    return softin_finish(s);
}

}  // extern "C"

// Every fetch call: up to max of the queued records Q of a consumer of `type`, each through conv into out[i].  A consumer of another kind has no such records; the
// calls of the kinds whose records carry a text made at fetch time (RS92, iMet-54, Meisei, MRZ, MTS01), of M20 and of WxR-301D say so (SONDE_E_ARG), and so does
// every call on a consumer of one of those kinds but M20; the older calls on the older kinds return an empty queue.
static bool softin_text_kind(const int t) { return t == SONDE_RS92 || t == SONDE_IMET54 || t == SONDE_MEISEI || t == SONDE_MRZ || t == SONDE_MTS01 || t == SONDE_WXR301; }
// -> how many records of `rec` bytes this call takes from the front of the queue, or the error
static int softin_fetch_count(sonde_softin_dev *s, const int type, const bool have_out, const int32_t max, const size_t rec) {
    if (!s) return SONDE_E_ARG;
    if (s->type != type && (type == SONDE_M20 || softin_text_kind(type) || softin_text_kind(s->type))) return SONDE_E_ARG;
    if (!have_out && max > 0) return SONDE_E_ARG;
    { const int rc = softin_finish(s); if (rc) return rc; }
    if (s->type != type) return 0;
    return (int)std::min<size_t>(s->q.size() / rec, (size_t)(max < 0 ? 0 : max));
}
template <class T> static int softin_fetch_plain(sonde_softin_dev *s, const int type, T *out, const int32_t max) {
    const int n = softin_fetch_count(s, type, out != nullptr, max, sizeof(T));
    if (n > 0) { memcpy((void *)out, s->q.data(), (size_t)n * sizeof(T)); s->q.erase(s->q.begin(), s->q.begin() + (size_t)n * sizeof(T)); }
    return n;
}
template <class Q, class O, class F>
static int softin_fetch(sonde_softin_dev *s, const int type, O *out, const int32_t max, const F &conv) {
    const int n = softin_fetch_count(s, type, out != nullptr, max, sizeof(Q));
    for (int i = 0; i < n; i++) { Q r; memcpy((void *)&r, s->q.data() + (size_t)i * sizeof(Q), sizeof(Q)); conv(r, out[i]); }
    if (n > 0) s->q.erase(s->q.begin(), s->q.begin() + (size_t)n * sizeof(Q));
    return n;
}

extern "C" {

int sonde_softin_dev_fetch(sonde_softin_dev_t *s, sonde_frame_t *out, int32_t max) { return softin_fetch_plain(s, SONDE_RS41, out, max); }
int sonde_softin_dev_fetch_dfm(sonde_softin_dev_t *s, sonde_dfm_frame_t *out, int32_t max) { return softin_fetch_plain(s, SONDE_DFM09, out, max); }
int sonde_softin_dev_fetch_m10(sonde_softin_dev_t *s, sonde_m10_frame_t *out, int32_t max) { return softin_fetch_plain(s, SONDE_M10, out, max); }
int sonde_softin_dev_fetch_m20(sonde_softin_dev_t *s, sonde_m20_frame_t *out, int32_t max) { return softin_fetch_plain(s, SONDE_M20, out, max); }
int sonde_softin_dev_fetch_drop(sonde_softin_dev_t *s, sonde_drop_frame_t *out, int32_t max) { return softin_fetch_plain(s, SONDE_RD94RD41, out, max); }
int sonde_softin_dev_fetch_lms6(sonde_softin_dev_t *s, sonde_lms6_softin_t *out, int32_t max) { return softin_fetch_plain(s, SONDE_LMS6, out, max); }

int sonde_softin_dev_set_lms6_rs(sonde_softin_dev_t *s, int32_t on) {
    if (!s || s->type != SONDE_LMS6) return SONDE_E_ARG;
    { const int rc = softin_finish(s); if (rc) return rc; }       // (a call in flight was launched under the switch as it stood)
    if (on && !s->d_l6_rs) {
        if (!s->dalloc(&s->d_l6_rs, (size_t)s->cap) || !s->h_l6_rs.alloc((size_t)s->cap)) return SONDE_E_NOGPU;
        TRY(sonde_lms6_rs_tables(s->mem, &s->d_l6_rs_tab));
    }
    s->l6_rs = on != 0;
    return 0;
}

int sonde_softin_dev_lms6_rs_stats(sonde_softin_dev_t *s, int64_t *used, int64_t *missed) {
    if (!s || s->type != SONDE_LMS6) return SONDE_E_ARG;
    int64_t u = 0, m = 0;
    for (int c = 0; c < s->C; c++) { int64_t a = 0, b = 0; (void)sonde_lms6_dec_rs_stats(s->decoder<sonde_lms6_dec_t>(c), &a, &b); u += a; m += b; }
    if (used) *used = u;
    if (missed) *missed = m;
    return 0;
}

int sonde_softin_dev_set_m20_skip(sonde_softin_dev_t *s, int32_t skip) {
    if (!s || s->type != SONDE_M20) return SONDE_E_ARG;
    s->opt = skip != 0;                            // (takes effect with the next call; a call in flight has its own copy)
    return 0;
}

// The text of a record is made here, by the channel's own decoder and from the device's bytes and verdicts, not in the push call: collect stays short.
// (a negative text_len: the text did not fit; the frame is delivered all the same)
int sonde_softin_dev_set_rs92_gps(sonde_softin_dev_t *s, int32_t on) {
    if (!s || s->type != SONDE_RS92) return SONDE_E_ARG;
    if (on && !s->gps) TRY(sonde_gps_dev_create(std::max(s->cap, 64), &s->gps));      // (a fetch holds what the push calls since the last one left: larger ones go in chunks)
    s->gps_on = on != 0;
    return 0;
}
int sonde_softin_dev_rs92_gps_stats(sonde_softin_dev_t *s, sonde_gps_stats_t *out) {
    if (!s || !out || s->type != SONDE_RS92) return SONDE_E_ARG;
    if (!s->gps) { memset(out, 0, sizeof *out); return 0; }
    return sonde_gps_dev_stats(s->gps, out);
}

// with the switch on: the records of the fetch through begin / one device solve / end, in rounds where a channel has several (sonde_gps_rs92_text_batch)
static int softin_fetch_rs92_gps(sonde_softin_dev *s, sonde_rs92_softin_t *out, const int32_t max) {
    const int n = softin_fetch_count(s, SONDE_RS92, out != nullptr, max, sizeof(SoftinRs92Rec));
    if (n <= 0) return n;
    std::vector<sonde_rs92_dec_t *> decs((size_t)n);
    std::vector<int32_t> ec((size_t)n), len((size_t)n);
    std::vector<uint8_t> frames((size_t)n * SONDE_RS92_FRAME_LEN);
    for (int i = 0; i < n; i++) {
        SoftinRs92Rec r; memcpy((void *)&r, s->q.data() + (size_t)i * sizeof r, sizeof r);
        sonde_rs92_softin_t &o = out[i];
        o.channel = r.channel; o.ec = r.ec; o.mv = r.mv; o.hdr_bit = r.hdr_bit;
        memcpy(o.frame, r.frame, sizeof o.frame);
        memcpy(frames.data() + (size_t)i * SONDE_RS92_FRAME_LEN, r.frame, SONDE_RS92_FRAME_LEN);
        decs[(size_t)i] = s->decoder<sonde_rs92_dec_t>(r.channel); ec[(size_t)i] = r.ec;
    }
    const int rc = sonde_gps_rs92_text_batch(s->gps, decs.data(), (const uint8_t (*)[SONDE_RS92_FRAME_LEN])frames.data(), ec.data(), n, out[0].text, sizeof(sonde_rs92_softin_t),
                                             len.data());
    for (int i = 0; i < n; i++) { out[i].text_len = len[(size_t)i]; if (len[(size_t)i] < 0) out[i].text[0] = 0; }
    s->q.erase(s->q.begin(), s->q.begin() + (size_t)n * sizeof(SoftinRs92Rec));
    return rc < 0 ? rc : n;
}

int sonde_softin_dev_fetch_rs92(sonde_softin_dev_t *s, sonde_rs92_softin_t *out, int32_t max) {
    if (s && s->gps_on && s->gps) return softin_fetch_rs92_gps(s, out, max);
    return softin_fetch<SoftinRs92Rec>(s, SONDE_RS92, out, max, [s](const SoftinRs92Rec &r, sonde_rs92_softin_t &o) {
        // print_frame behind rs92_ecc (the decoder's calibration rows, its orbit data)
        o.channel = r.channel; o.ec = r.ec; o.mv = r.mv; o.hdr_bit = r.hdr_bit;
        memcpy(o.frame, r.frame, sizeof o.frame);
        o.text_len = sonde_rs92_dec_corrected(s->decoder<sonde_rs92_dec_t>(r.channel), r.frame, r.ec, o.text, sizeof o.text);
        if (o.text_len < 0) o.text[0] = 0;
    });
}
int sonde_softin_dev_fetch_imet54(sonde_softin_dev_t *s, sonde_imet54_softin_t *out, int32_t max) {
    return softin_fetch<SoftinImet54Rec>(s, SONDE_IMET54, out, max, [s](const SoftinImet54Rec &r, sonde_imet54_softin_t &o) {
        // print_frame behind the Hamming step
        o.channel = r.channel; o.ecc_frm = r.ecc_frm; o.ecc_tlm = r.ecc_tlm; o.ecc_std = r.ecc_std; o.crc = r.crc_std ? 1 : r.crc_cont ? 2 : 0; o.mv = r.mv; o.hdr_bit = r.hdr_bit;
        memcpy(o.frame, r.frame, sizeof o.frame);
        o.text_len = sonde_imet54_dec_decoded(s->decoder<sonde_imet54_dec_t>(r.channel), r.frame, r.ecc_frm, r.ecc_tlm, r.ecc_std, r.crc_std, r.crc_cont, o.text, sizeof o.text);
        if (o.text_len < 0) o.text[0] = 0;
    });
}
int sonde_softin_dev_fetch_meisei(sonde_softin_dev_t *s, sonde_meisei_softin_t *out, int32_t max) {
    return softin_fetch<SoftinMeiseiRec>(s, SONDE_MEISEI, out, max, [s](const SoftinMeiseiRec &r, sonde_meisei_softin_t &o) {
        // the printers behind the block loop
        o.channel = r.channel; o.mv = r.mv; o.hdr_bit = r.hdr_bit; o.err_frm = 0; o.err_blks = 0;
        for (int k = 0; k < MEISEI_BLOCKS; k++) { o.block_err[k] = r.block_err[k]; o.err_frm += r.block_err[k] >= 0xE; o.err_blks += r.block_err[k] != 0; }
        memcpy(o.bits, r.bits, sizeof o.bits);
        o.text_len = sonde_meisei_dec_decoded(s->decoder<sonde_meisei_dec_t>(r.channel), r.bits, r.block_err, o.text, sizeof o.text);
        if (o.text_len < 0) o.text[0] = 0;
    });
}
int sonde_softin_dev_fetch_mrz(sonde_softin_dev_t *s, sonde_mrz_softin_t *out, int32_t max) {
    return softin_fetch<SoftinMrzRec>(s, SONDE_MRZ, out, max, [s](const SoftinMrzRec &r, sonde_mrz_softin_t &o) {
        // print_frame from the device's bits and the device's CRC verdict
        o.channel = r.channel; o.nbits = r.nbits; o.inv = r.inv; o.crc_ok = r.crc_ok; o.crclen = r.crclen; o.mv = r.mv; o.hdr_bit = r.hdr_bit;
        memcpy(o.bits, r.bits, sizeof o.bits);
        o.text_len = sonde_mrz_dec_decoded(s->decoder<sonde_mrz_dec_t>(r.channel), r.bits, r.nbits, r.crc_ok, o.text, sizeof o.text);
        if (o.text_len < 0) o.text[0] = 0;
    });
}
int sonde_softin_dev_fetch_mts01(sonde_softin_dev_t *s, sonde_mts01_softin_t *out, int32_t max) {
    return softin_fetch<SoftinMts01Rec>(s, SONDE_MTS01, out, max, [s](const SoftinMts01Rec &r, sonde_mts01_softin_t &o) {
        // print_frame from the device's bytes, CRC value and verdict
        o.channel = r.channel; o.crcval = r.crcval; o.crcdat = r.crcdat; o.crc_ok = r.crc_ok; o.mv = r.mv; o.hdr_bit = r.hdr_bit;
        memcpy(o.bytes, r.bytes, sizeof o.bytes);
        o.text_len = sonde_mts01_dec_decoded(s->decoder<sonde_mts01_dec_t>(r.channel), r.bytes, r.crcval, r.crc_ok, o.text, sizeof o.text);
        if (o.text_len < 0) o.text[0] = 0;
    });
}

int sonde_softin_dev_fetch_wxr(sonde_softin_dev_t *s, sonde_wxr_softin_rec_t *out, int32_t max) {
    return softin_fetch<SoftinWxrRec>(s, SONDE_WXR301, out, max, [](const SoftinWxrRec &r, sonde_wxr_softin_rec_t &o) { memcpy((void *)&o, (const void *)&r, sizeof o); });
}

int sonde_softin_dev_counts(sonde_softin_dev_t *s, int64_t *frames, int64_t *ecc_ok, int64_t *repaired, int64_t *symbols, int64_t *dropped) {
    if (!s) return SONDE_E_ARG;
    { const int rc = softin_finish(s); if (rc) return rc; }
    if (frames) *frames = s->frames_total;
    if (ecc_ok) *ecc_ok = s->ecc_ok_total;
    if (repaired) *repaired = s->repaired_total;
    if (symbols) *symbols = s->symbols_total;
    if (dropped) *dropped = s->dropped;
    return 0;
}

}  // extern "C"
