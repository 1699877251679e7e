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
#include "sonde_pinned.h"
#include "sonde_drop_dev.h"
#include "sonde_softhdr_dev.h"
#include "sonde_vit_dev.h"
#include "sonde_softin_mxx_dev.h"
#include "sonde_softin_rs92_dev.h"
#include "sonde_softin_imet54_dev.h"
#include "sonde_softin_meisei_dev.h"
#include "../../include/sonde_drop.h"
#include "../../include/sonde_rs92.h"
#include "../../include/sonde_imet54.h"
#include "../../include/sonde_meisei.h"
#include <cstdio>
#include <cstring>
#include <vector>

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "libsonde_hip: %s failed: %s\n", #x, hipGetErrorString(e_)); return SONDE_E_NOGPU; } } while (0)

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
    const FskChan *fsk_chan; int bits_per_frame;   // or: frames of the modem's last launch x bits per frame
    const int *ch_list;                            // the channels of this launch (one workgroup each); null: all of them
    int n_ch, inv_in, opt_auto; float ths;
    SoftinChan *chan;
    unsigned char *frames; int *flen; SoftinMeta *meta; unsigned *count; int cap;
    const unsigned char *hdr;                      // 64 header bits ('0'/'1'), 8 header bytes, 64 mask bytes
};

__global__ __launch_bounds__(64)
void k_softin_rs41(const SoftinArgs a) {
    __shared__ float s_hist[64];
    __shared__ unsigned char s_frame[520];
    __shared__ float s_carry[8];
    const int ch = a.ch_list ? a.ch_list[blockIdx.x] : (int)blockIdx.x, lane = threadIdx.x;
    if (ch >= a.n_ch) return;
    SoftinChan *st = a.chan + ch;
    int nb = a.nbits;
    if (a.fsk_chan) { const int fr = a.fsk_chan[ch].frames; nb = fr > 0 ? fr * a.bits_per_frame : 0; }
    else if (a.nbits_ch) nb = a.nbits_ch[ch];
    const float *x = a.sd + (size_t)ch * a.ch_stride;
    int mode = st->mode, inv = st->inv, body_done = st->body_done, carry_n = st->carry_n;
    float mv_hdr = st->mv; unsigned long long hdr_bit = st->hdr_bit; const unsigned long long bits0 = st->bits_in;
    s_hist[lane] = st->hist[lane];
    for (int i = lane; i < 520; i += 64) s_frame[i] = st->frame[i];
    if (lane < 8) s_carry[lane] = st->carry[lane];
    // the header as +-1, one element per lane (for the dot products every lane needs all 64: from LDS-free registers via the constant array)
    __builtin_amdgcn_wave_barrier();
    const float sgn = a.inv_in ? -1.f : 1.f;
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
                unsigned slot = 0;
                if (lane == 0) slot = atomicAdd(a.count, 1u);
                slot = __shfl(slot, 0);
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
    const int ch = a.ch_list ? a.ch_list[blockIdx.x] : (int)blockIdx.x, lane = threadIdx.x;
    if (ch >= a.n_ch) return;
    SoftinDfmChan *st = A.chan + ch;
    int nb = a.nbits;
    if (a.fsk_chan) { const int fr = a.fsk_chan[ch].frames; nb = fr > 0 ? fr * a.bits_per_frame : 0; }
    else if (a.nbits_ch) nb = a.nbits_ch[ch];
    const float *x = a.sd + (size_t)ch * a.ch_stride;
    int mode = st->mode, inv = st->inv, dpos = st->dpos, dfrm = st->dfrm, dhalf = st->dhalf;
    float ds1 = st->ds1, mv_hdr = st->mv; unsigned hdrcnt = st->hdrcnt; unsigned long long hdr_bit = st->hdr_bit; const unsigned long long bits0 = st->bits_in;
    if (lane < 32) s_hist[lane] = st->hist[lane];
    for (int i = lane; i < 280; i += 64) { s_hb[i] = st->dhb[i]; s_sf[i] = st->dsf[i]; }
    __builtin_amdgcn_wave_barrier();
    const float sgn = a.inv_in ? -1.f : 1.f;
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
                unsigned slot = 0;
                if (lane == 0) slot = atomicAdd(a.count, 1u);
                slot = __shfl(slot, 0);
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
// (M10_STAGE_MAX, the soft decisions of a call the kernel keeps in LDS: sonde_softin_mxx_dev.h)

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
    const int ch = a.ch_list ? a.ch_list[blockIdx.x] : (int)blockIdx.x, lane = threadIdx.x;
    if (ch >= a.n_ch) return;
    SoftinM10Chan *st = A.chan + ch;
    int nb = a.nbits;
    if (a.fsk_chan) { const int fr = a.fsk_chan[ch].frames; nb = fr > 0 ? fr * a.bits_per_frame : 0; }
    else if (a.nbits_ch) nb = a.nbits_ch[ch];
    const float *x = a.sd + (size_t)ch * a.ch_stride;
    constexpr int NBITS = 121 * 8;
    int mode = st->mode, inv = st->inv, mpos = st->mpos, mhalf = st->mhalf, mbit0 = st->mbit0, mskip = st->mskip;
    float ms1 = st->ms1, mv_hdr = st->mv; unsigned long long hdr_bit = st->hdr_bit; const unsigned long long bits0 = st->bits_in;
    if (lane < 32) s_hist[lane] = st->hist[lane];
    for (int i = lane; i < 976; i += 64) s_mb[i] = st->mbits[i];
    const float sgn = a.inv_in ? -1.f : 1.f;
    const bool staged = nb <= A.stage_cap;
    if (staged) for (int i = lane; i < nb; i += 64) s_x[i] = sgn * x[i];
    __builtin_amdgcn_wave_barrier();
    auto X = [&](int p) -> float { return staged ? s_x[p] : sgn * x[p]; };       // soft decision p of this call, in the polarity in effect
    unsigned hbits = 0;                                                          // the 32 header symbols as a bit mask
    for (int i = 0; i < 32; i++) hbits |= (unsigned)(a.hdr[i] & 1) << i;
    int cur = 0;
    while (cur < nb) {
        if (mode == 0) {
            bool found = false;
            for (int base = cur; base < nb && !found; base += 64) {
                const int q = base + lane;
                float mv = 0.f;
                if (q < nb) {
                    const int e = 32 + (q - cur);
                    float fs = 0.f, fn = 0.f;
                    for (int i = 0; i < 32; i++) {
                        const int k = e - 31 + i;
                        const float v = k < 32 ? s_hist[k] : X(cur + (k - 32));
                        fs += ((hbits >> i) & 1u) ? v : -v;
                        fn = fmaf(v, v, fn);
                    }
                    mv = fs * __builtin_amdgcn_rsqf(fn * 32.0f);
                    if (!(fabsf(mv) < a.ths - 1e-3f)) {                   // (also NaN: an all-zero window is the reference's 0 / 0)
                        double sum = 0.0, normx = 0.0;
                        for (int i = 0; i < 32; i++) {
                            const int k = e - 31 + i;
                            const float v = k < 32 ? s_hist[k] : X(cur + (k - 32));
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
                    const int l = __builtin_ctzll(hits);
                    const float mvl = __shfl(mv, l);
                    if ((double)mvl * (0.5 - inv) < 0) inv ^= 1;            // irrelevant for the differential code (m10mod.c:1447)
                    found = true;
                    const int qs = base + l, e = 32 + (qs - cur), k = e - 31 + (lane & 31);
                    const float v = k < 32 ? s_hist[k] : X(cur + (k - 32));
                    __builtin_amdgcn_wave_barrier();
                    if (lane < 32) s_hist[lane] = v;
                    __builtin_amdgcn_wave_barrier();
                    mode = 1; mpos = 0; mhalf = 0; mbit0 = '0'; mv_hdr = mvl; hdr_bit = bits0 + (unsigned long long)qs + 1ull;
                    cur = qs + 1;
                }
            }
            if (!found) {
                const int e = 32 + (nb - 1 - cur), k = e - 31 + (lane & 31);
                const float v = k < 32 ? s_hist[k] : X(cur + (k - 32));
                __builtin_amdgcn_wave_barrier();
                if (lane < 32) s_hist[lane] = v;
                __builtin_amdgcn_wave_barrier();
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
                unsigned slot = 0;
                if (lane == 0) slot = atomicAdd(a.count, 1u);
                slot = __shfl(slot, 0);
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
    const int ch = a.ch_list ? a.ch_list[blockIdx.x] : (int)blockIdx.x, lane = threadIdx.x;
    if (ch >= a.n_ch || ch < 0) return;
    int nb = a.nbits;
    if (a.fsk_chan) { const int fr = a.fsk_chan[ch].frames; nb = fr > 0 ? fr * a.bits_per_frame : 0; }
    else if (a.nbits_ch) nb = a.nbits_ch[ch];
    nb = __builtin_amdgcn_readfirstlane(nb);
    if ((long long)nb > a.ch_stride) return;                                     // (never: a channel's count lies within its stride)
    m20_wave_channel(A.chan + ch, a.sd + (size_t)ch * a.ch_stride, nb, a.inv_in ? -1.f : 1.f, a.ths, A.doskip, &s_l, s_x, A.stage_cap, A.out, a.count, a.cap, ch, lane);
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
    const int ch = a.ch_list ? a.ch_list[blockIdx.x] : (int)blockIdx.x, lane = threadIdx.x;
    if (ch >= a.n_ch || ch < 0) return;
    int nb = a.nbits;
    if (a.fsk_chan) { const int fr = a.fsk_chan[ch].frames; nb = fr > 0 ? fr * a.bits_per_frame : 0; }
    else if (a.nbits_ch) nb = a.nbits_ch[ch];
    nb = __builtin_amdgcn_readfirstlane(nb);
    if ((long long)nb > a.ch_stride) return;                                     // (never: a channel's count lies within its stride)
    rs92_wave_channel(A.chan + ch, a.sd + (size_t)ch * a.ch_stride, nb, a.inv_in ? -1.f : 1.f, A.inv, a.ths, A.gf, &s_l, s_x, A.stage_cap, A.out, a.count, a.cap, ch, lane);
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
    const int ch = a.ch_list ? a.ch_list[blockIdx.x] : (int)blockIdx.x, lane = threadIdx.x;
    if (ch >= a.n_ch || ch < 0) return;
    int nb = a.nbits;
    if (a.fsk_chan) { const int fr = a.fsk_chan[ch].frames; nb = fr > 0 ? fr * a.bits_per_frame : 0; }
    else if (a.nbits_ch) nb = a.nbits_ch[ch];
    nb = __builtin_amdgcn_readfirstlane(nb);
    if ((long long)nb > a.ch_stride) return;                                     // (never: a channel's count lies within its stride)
    imet54_wave_channel(A.chan + ch, a.sd + (size_t)ch * a.ch_stride, nb, a.inv_in ? -1.f : 1.f, a.opt_auto, A.ecc, a.ths, A.tab, &s_l, s_x, A.stage_cap, A.out, a.count, a.cap, ch, lane);
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
    const int ch = a.ch_list ? a.ch_list[blockIdx.x] : (int)blockIdx.x, lane = threadIdx.x;
    if (ch >= a.n_ch || ch < 0) return;
    int nb = a.nbits;
    if (a.fsk_chan) { const int fr = a.fsk_chan[ch].frames; nb = fr > 0 ? fr * a.bits_per_frame : 0; }
    else if (a.nbits_ch) nb = a.nbits_ch[ch];
    nb = __builtin_amdgcn_readfirstlane(nb);
    if ((long long)nb > a.ch_stride) return;                                     // (never: a channel's count lies within its stride)
    meisei_wave_channel(A.chan + ch, a.sd + (size_t)ch * a.ch_stride, nb, a.inv_in ? -1.f : 1.f, A.ecc, a.ths, &s_l, s_x, A.stage_cap, A.out, a.count, a.cap, ch, lane);
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
    const int ch = a.ch_list ? a.ch_list[blockIdx.x] : (int)blockIdx.x, lane = threadIdx.x;
    if (ch >= a.n_ch) return;
    SoftinDropChan *st = A.chan + ch;
    int nb = a.nbits;
    if (a.fsk_chan) { const int fr = a.fsk_chan[ch].frames; nb = fr > 0 ? fr * a.bits_per_frame : 0; }
    else if (a.nbits_ch) nb = a.nbits_ch[ch];
    nb = __builtin_amdgcn_readfirstlane(nb);
    const float *x = a.sd + (size_t)ch * a.ch_stride;
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
    const int ch = a.ch_list ? a.ch_list[blockIdx.x] : (int)blockIdx.x, lane = threadIdx.x;
    if (ch >= a.n_ch || ch < 0) return;
    int nb = a.nbits;
    if (a.nbits_ch) nb = a.nbits_ch[ch];
    nb = __builtin_amdgcn_readfirstlane(nb);
    lms6_wave_channel(A.chan + ch, a.sd + (size_t)ch * a.ch_stride, nb, a.inv_in ? -1.f : 1.f, A.vit, A.stop_at_block, a.hdr, &s_l, A.out, a.count, a.cap, ch, lane);
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
extern "C" int sonde_fsk_dev_view(sonde_fsk_t *f, const float **d_sd, long long *sd_cap, const FskChan **d_chan, int *bits_per_frame, int *n_ch, hipStream_t *stream);
extern "C" int sonde_fsk_dev_reader_done(sonde_fsk_t *f, hipStream_t consumer_stream);
extern "C" int sonde_fsk_dev_view_prev(sonde_fsk_t *f, const float **d_sd, long long *sd_cap, int *bits_per_frame, int *n_ch, int32_t *frames_out);
extern "C" int sonde_fsk_dev_reader_done_prev(sonde_fsk_t *f, hipStream_t consumer_stream);

struct sonde_softin_dev {
    int C = 0, ecc_level = 0, cap = 0, type = SONDE_RS41;
    SoftinDfmChan *d_dfm_chan = nullptr; sonde_dfm_frame_t *d_dfm_out = nullptr; std::vector<sonde_dfm_frame_t> qdfm; Pinned<sonde_dfm_frame_t> h_dfm;
    SoftinM10Chan *d_m10_chan = nullptr; sonde_m10_frame_t *d_m10_out = nullptr; std::vector<sonde_m10_frame_t> qm10; Pinned<sonde_m10_frame_t> h_m10;
    SoftinM20Chan *d_m20_chan = nullptr; sonde_m20_frame_t *d_m20_out = nullptr; std::vector<sonde_m20_frame_t> qm20; Pinned<sonde_m20_frame_t> h_m20; int m20_skip = 1;
    SoftinDropChan *d_drop_chan = nullptr; DropFrame *d_drop_out = nullptr; std::vector<sonde_drop_frame_t> qdrop; Pinned<DropFrame> h_drop; int drop_inv = 0;
    // SONDE_LMS6: a host decoder per channel (what follows block_bytes), the channels of a relaunch, the block length each channel has on the device
    Lms6Chan *d_l6_chan = nullptr; Lms6Block *d_l6_out = nullptr; Pinned<Lms6Block> h_l6; std::vector<sonde_lms6_softin_t> ql6; std::vector<sonde_lms6_dec_t *> l6_dec;
    int l6_vit = 0, l6_auto = 0; int *d_l6_list = nullptr; Pinned<int> h_l6_list, h_l6_len; std::vector<int> l6_len; std::vector<int64_t> l6_ok;
    // SONDE_RS92: a host decoder per channel (the calibration rows a channel collects are per sonde); the text of a record is made when it is fetched
    SoftinRs92Chan *d_r92_chan = nullptr; SoftinRs92Rec *d_r92_out = nullptr; Pinned<SoftinRs92Rec> h_r92; std::vector<SoftinRs92Rec> qr92; std::vector<sonde_rs92_dec_t *> r92_dec; int r92_inv = 0;
    // SONDE_IMET54: a host decoder per channel (print_position keeps its fields in the object); the text of a record is made when it is fetched
    SoftinImet54Chan *d_i54_chan = nullptr; SoftinImet54Rec *d_i54_out = nullptr; uint32_t *d_i54_tab = nullptr; Pinned<SoftinImet54Rec> h_i54; std::vector<SoftinImet54Rec> qi54;
    std::vector<sonde_imet54_dec_t *> i54_dec; int i54_ecc = 0;
    // SONDE_MEISEI: a host decoder per channel (the variant in effect, the 64-word configuration, the counters); the text of a record is made when it is fetched
    SoftinMeiseiChan *d_mei_chan = nullptr; SoftinMeiseiRec *d_mei_out = nullptr; Pinned<SoftinMeiseiRec> h_mei; std::vector<SoftinMeiseiRec> qmei;
    std::vector<sonde_meisei_dec_t *> mei_dec; int mei_ecc = 0;
    SoftinArgs args{};
    hipStream_t stream = nullptr; bool own_stream = false;
    SoftinChan *d_chan = nullptr; unsigned char *d_frames = nullptr, *d_hdr = nullptr, *d_gf = nullptr, *d_synd = nullptr;
    int *d_flen = nullptr, *d_ecc = nullptr, *d_codes = nullptr; SoftinMeta *d_meta = nullptr; unsigned *d_count = nullptr;
    std::vector<sonde_frame_t> queue;
    long long frames_total = 0, ecc_ok_total = 0, repaired_total = 0, symbols_total = 0, dropped = 0;
    Pinned<int> h_ecc; Pinned<SoftinMeta> h_meta; Pinned<unsigned char> h_frames;       // page-locked landing buffers of a call's records (sonde_pinned.h)
    unsigned *h_count = nullptr;                   // pinned: the counters of a call's two passes
    int head = 0;                                  // records copied to the host without asking how many there are (what a call of a second normally completes)
    bool pending = false; hipStream_t pend_stream = nullptr;
    int *h_nbits = nullptr, *d_nbits = nullptr;    // bits per channel of the modem launch a call consumes (pinned host copy, device copy)
};

extern "C" {

int sonde_softin_dev_create(int32_t n_channels, int32_t sonde_type, int32_t ecc_level, int32_t invert_stream, int32_t opt_inv, int32_t opt_auto, sonde_softin_dev_t **out) {
    if (!out || n_channels < 1 || (sonde_type != SONDE_RS41 && sonde_type != SONDE_DFM09 && sonde_type != SONDE_M10 && sonde_type != SONDE_M20 && sonde_type != SONDE_RD94RD41) || ecc_level < 0 || ecc_level > 2) return SONDE_E_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { fprintf(stderr, "libsonde_hip: no usable HIP device (the batched soft-bit framer has no CPU fallback)\n"); return SONDE_E_NOGPU; }
    sonde_softin_dev *s = new sonde_softin_dev();
    s->C = n_channels; s->ecc_level = ecc_level; s->type = sonde_type;
    // frames a call of about a second can complete per channel: RS41 two, DFM09 six (280 bits at 1250 b/s), M10 two (one per second; the rest of the second is skipped),
    // dropsondes three (two a second), M20 four (without the skip a frame can complete every 32 + 2640 symbols of the 9600 a second)
    s->cap = (sonde_type == SONDE_DFM09 ? 8 : sonde_type == SONDE_RD94RD41 || sonde_type == SONDE_M20 ? 4 : 2) * n_channels + 16;
    const size_t C = (size_t)n_channels, cap = (size_t)s->cap;
    std::vector<SoftinChan> init(C);
    memset(init.data(), 0, C * sizeof(SoftinChan));
    for (auto &c : init) { c.inv = opt_inv ? 1 : 0; memcpy(c.frame, sonde::kRs41HeaderBytes, 8); }
    unsigned char hdr[136];
    memset(hdr, 0, sizeof hdr);
    if (sonde_type == SONDE_RS41) { memcpy(hdr, sonde::kRs41Header, 64); memcpy(hdr + 64, sonde::kRs41HeaderBytes, 8); memcpy(hdr + 72, sonde::kRs41Mask, 64); }
    else memcpy(hdr, sonde_type == SONDE_DFM09 ? sonde::kDfmRawHeader : sonde::kM10RawHeader, 32);
    bool ok = hipMalloc((void **)&s->d_chan, C * sizeof(SoftinChan)) == hipSuccess && hipMalloc((void **)&s->d_frames, cap * 518) == hipSuccess
           && hipMalloc((void **)&s->d_hdr, sizeof hdr) == hipSuccess && hipMalloc((void **)&s->d_gf, 768) == hipSuccess && hipMalloc((void **)&s->d_synd, cap * 48) == hipSuccess
           && hipMalloc((void **)&s->d_flen, cap * 4) == hipSuccess && hipMalloc((void **)&s->d_ecc, cap * 4) == hipSuccess && hipMalloc((void **)&s->d_codes, cap * 8) == hipSuccess
           && hipMalloc((void **)&s->d_meta, cap * sizeof(SoftinMeta)) == hipSuccess && hipMalloc((void **)&s->d_count, 8) == hipSuccess && hipHostMalloc((void **)&s->h_count, 8) == hipSuccess;
    ok = ok && hipMemcpy(s->d_chan, init.data(), C * sizeof(SoftinChan), hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(s->d_hdr, hdr, sizeof hdr, hipMemcpyHostToDevice) == hipSuccess
            && hipMemcpy(s->d_gf, sonde::gf_exp_table(), 512, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(s->d_gf + 512, sonde::gf_log_table(), 256, hipMemcpyHostToDevice) == hipSuccess
            && hipMemset(s->d_ecc, 0, cap * 4) == hipSuccess;
    if (ok && sonde_type == SONDE_DFM09) {
        std::vector<SoftinDfmChan> di(C);
        memset(di.data(), 0, C * sizeof(SoftinDfmChan));
        static const char kDfmHdr[] = "0100010111001111";                                 // dfm09mod.c:1503-1506: the header's 16 bits in front of the first frame of a hit
        for (auto &c : di) { c.inv = opt_inv ? 1 : 0; c.dpos = 16; for (int i = 0; i < 16; i++) c.dhb[i] = (unsigned char)(kDfmHdr[i] & 1); }
        ok = hipMalloc((void **)&s->d_dfm_chan, C * sizeof(SoftinDfmChan)) == hipSuccess && hipMalloc((void **)&s->d_dfm_out, cap * sizeof(sonde_dfm_frame_t)) == hipSuccess
          && hipMemcpy(s->d_dfm_chan, di.data(), C * sizeof(SoftinDfmChan), hipMemcpyHostToDevice) == hipSuccess;
        ok = ok && s->h_dfm.alloc(cap);
    }
    if (ok && sonde_type == SONDE_M10) {
        std::vector<SoftinM10Chan> mi(C);
        memset(mi.data(), 0, C * sizeof(SoftinM10Chan));
        for (auto &c : mi) { c.inv = opt_inv ? 1 : 0; c.mbit0 = '0'; }
        ok = hipMalloc((void **)&s->d_m10_chan, C * sizeof(SoftinM10Chan)) == hipSuccess && hipMalloc((void **)&s->d_m10_out, cap * sizeof(sonde_m10_frame_t)) == hipSuccess
          && hipMemcpy(s->d_m10_chan, mi.data(), C * sizeof(SoftinM10Chan), hipMemcpyHostToDevice) == hipSuccess;
        ok = ok && s->h_m10.alloc(cap);
    }
    if (ok && sonde_type == SONDE_M20) {
        std::vector<SoftinM20Chan> mi(C);
        memset((void *)mi.data(), 0, C * sizeof(SoftinM20Chan));
        for (auto &c : mi) { c.inv = opt_inv ? 1 : 0; c.mbit0 = '0'; }
        ok = hipMalloc((void **)&s->d_m20_chan, C * sizeof(SoftinM20Chan)) == hipSuccess && hipMalloc((void **)&s->d_m20_out, cap * sizeof(sonde_m20_frame_t)) == hipSuccess
          && hipMemcpy(s->d_m20_chan, mi.data(), C * sizeof(SoftinM20Chan), hipMemcpyHostToDevice) == hipSuccess;
        ok = ok && s->h_m20.alloc(cap);
    }
    if (ok && sonde_type == SONDE_RD94RD41) {
        std::vector<SoftinDropChan> di(C);
        memset(di.data(), 0, C * sizeof(SoftinDropChan));
        for (auto &c : di) { c.pos = DROP_HEADLEN; for (int i = 0; i < DROP_HEADLEN; i++) c.frame[i] = (unsigned char)((DROP_HDR40 >> (DROP_HEADLEN - 1 - i)) & 1); }
        s->drop_inv = (invert_stream ? 1 : 0) ^ (opt_inv ? 1 : 0);
        ok = hipMalloc((void **)&s->d_drop_chan, C * sizeof(SoftinDropChan)) == hipSuccess && hipMalloc((void **)&s->d_drop_out, cap * sizeof(DropFrame)) == hipSuccess
          && hipMemcpy(s->d_drop_chan, di.data(), C * sizeof(SoftinDropChan), hipMemcpyHostToDevice) == hipSuccess;
        ok = ok && s->h_drop.alloc(cap);
    }
    if (!ok) { sonde_softin_dev_destroy(s); return SONDE_E_NOMEM; }
    SoftinArgs &a = s->args;
    a.n_ch = n_channels; a.inv_in = invert_stream ? 1 : 0; a.opt_auto = opt_auto ? 1 : 0; a.ths = sonde_type == SONDE_M10 || sonde_type == SONDE_M20 ? 0.8f : 0.7f;
    a.chan = s->d_chan; a.frames = s->d_frames; a.flen = s->d_flen; a.meta = s->d_meta; a.count = s->d_count; a.cap = s->cap; a.hdr = s->d_hdr;
    if (!s->h_ecc.alloc(cap) || !s->h_meta.alloc(cap) || !s->h_frames.alloc(cap * 518)) { sonde_softin_dev_destroy(s); return SONDE_E_NOMEM; }
    s->head = std::min(s->cap, (sonde_type == SONDE_DFM09 ? 5 : sonde_type == SONDE_RD94RD41 ? 2 : 1) * n_channels + 16);
    (void)hipGetLastError();
    *out = s;
    return 0;
}

int sonde_softin_dev_create_lms6(int32_t n_channels, const sonde_lms6_opts_t *opts, int32_t invert_stream, sonde_softin_dev_t **out) {
    if (!out || n_channels < 1 || !opts) return SONDE_E_ARG;
    sonde_lms6_opts_t o = *opts;
    if (o.json) { if (!o.ecc) o.ecc = 1; if (!o.vit) o.vit = 1; }                              // lms6Xmod.c:1153-1157
    if (o.vit != 1 && o.vit != 2) return SONDE_E_ARG;                                          // the algebraic decoder alone has no device form
    if (o.ecc == 3) return SONDE_E_ARG;                                                        // --ecc3 needs the second soft value of a sample-rate demodulator
    {   sonde_lms6_dec_t *probe = nullptr;                                                     // the option checks of the host decoder, before the device is touched
        const int rc = sonde_lms6_dec_create(&o, &probe);
        if (rc) return rc;
        sonde_lms6_dec_destroy(probe);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { fprintf(stderr, "libsonde_hip: no usable HIP device (the batched soft-bit framer has no CPU fallback)\n"); return SONDE_E_NOGPU; }
    sonde_softin_dev *s = new sonde_softin_dev();
    s->C = n_channels; s->type = SONDE_LMS6; s->l6_vit = o.vit; s->l6_auto = o.typ == 0;
    s->cap = 4 * n_channels + 16;                              // blocks a call can hold over all channels (sonde_fsk.h): a channel completes at most two in a second of 4800 soft bits
    const size_t C = (size_t)n_channels, cap = (size_t)s->cap;
    for (size_t c = 0; c < C; c++) {
        sonde_lms6_dec_t *d = nullptr;
        if (sonde_lms6_dec_create(&o, &d)) { sonde_softin_dev_destroy(s); return SONDE_E_NOMEM; }
        s->l6_dec.push_back(d);
    }
    const int len0 = sonde_lms6_dec_block_bits(s->l6_dec[0]) + LMS6_BLOCKSTART;
    s->l6_len.assign(C, len0); s->l6_ok.assign(C, 0);
    bool ok = hipMalloc((void **)&s->d_l6_chan, C * sizeof(Lms6Chan)) == hipSuccess && hipMalloc((void **)&s->d_l6_out, cap * sizeof(Lms6Block)) == hipSuccess
           && hipMalloc((void **)&s->d_l6_list, C * sizeof(int)) == hipSuccess && hipMalloc((void **)&s->d_hdr, 64) == hipSuccess
           && hipMalloc((void **)&s->d_count, 8) == hipSuccess && hipHostMalloc((void **)&s->h_count, 8) == hipSuccess
           && s->h_l6.alloc(cap) && s->h_l6_list.alloc(C) && s->h_l6_len.alloc(C);
    if (ok) {
        std::vector<Lms6Chan> init(C);
        memset((void *)init.data(), 0, C * sizeof(Lms6Chan));
        for (auto &c : init) { c.pos = LMS6_BLOCKSTART; c.rawblk_len = len0; }
        ok = hipMemcpy(s->d_l6_chan, init.data(), C * sizeof(Lms6Chan), hipMemcpyHostToDevice) == hipSuccess
          && hipMemcpy(s->d_hdr, sonde_lms6_raw_header(), 64, hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) { sonde_softin_dev_destroy(s); return SONDE_E_NOMEM; }
    SoftinArgs &a = s->args;
    a.n_ch = n_channels; a.inv_in = invert_stream ? 1 : 0; a.ths = 0.7f; a.count = s->d_count; a.cap = s->cap; a.hdr = s->d_hdr;
    s->head = std::min(s->cap, n_channels + 16);
    (void)hipGetLastError();
    *out = s;
    return 0;
}

int sonde_softin_dev_create_rs92(int32_t n_channels, const sonde_rs92_opts_t *opts, int32_t invert_stream, sonde_softin_dev_t **out) {
    if (!out || n_channels < 1 || !opts) return SONDE_E_ARG;
    if (opts->gps_verbose == 8 || opts->dbg) return SONDE_E_ARG;                               // -gg / --dbg: lines without a bound per frame
    {   sonde_rs92_dec_t *probe = nullptr;                                                     // the option checks of the host decoder, before the device is touched
        const int rc = sonde_rs92_dec_create(opts, &probe);
        if (rc) return rc;
        sonde_rs92_dec_destroy(probe);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { fprintf(stderr, "libsonde_hip: no usable HIP device (the batched soft-bit framer has no CPU fallback)\n"); return SONDE_E_NOGPU; }
    sonde_softin_dev *s = new sonde_softin_dev();
    s->C = n_channels; s->type = SONDE_RS92; s->r92_inv = opts->inv ? 1 : 0;
    s->cap = 4 * n_channels + 16;                              // frames a call can hold over all channels (sonde_fsk.h): a channel completes one per 4740 symbols at the least
    const size_t C = (size_t)n_channels, cap = (size_t)s->cap;
    for (size_t c = 0; c < C; c++) {
        sonde_rs92_dec_t *d = nullptr;
        if (sonde_rs92_dec_create(opts, &d)) { sonde_softin_dev_destroy(s); return SONDE_E_NOMEM; }
        s->r92_dec.push_back(d);
    }
    bool ok = hipMalloc((void **)&s->d_r92_chan, C * sizeof(SoftinRs92Chan)) == hipSuccess && hipMalloc((void **)&s->d_r92_out, cap * sizeof(SoftinRs92Rec)) == hipSuccess
           && hipMalloc((void **)&s->d_gf, 768) == hipSuccess && hipMalloc((void **)&s->d_count, 8) == hipSuccess && hipHostMalloc((void **)&s->h_count, 8) == hipSuccess
           && s->h_r92.alloc(cap);
    ok = ok && hipMemset(s->d_r92_chan, 0, C * sizeof(SoftinRs92Chan)) == hipSuccess
            && hipMemcpy(s->d_gf, sonde::gf_exp_table(), 512, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(s->d_gf + 512, sonde::gf_log_table(), 256, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) { sonde_softin_dev_destroy(s); return SONDE_E_NOMEM; }
    SoftinArgs &a = s->args;
    a.n_ch = n_channels; a.inv_in = invert_stream ? 1 : 0; a.ths = 0.8f; a.count = s->d_count; a.cap = s->cap;
    s->head = std::min(s->cap, n_channels + 16);               // (a frame a second and channel)
    (void)hipGetLastError();
    *out = s;
    return 0;
}

int sonde_softin_dev_create_imet54(int32_t n_channels, const sonde_imet54_opts_t *opts, int32_t invert_stream, sonde_softin_dev_t **out) {
    if (!out || n_channels < 1 || !opts) return SONDE_E_ARG;
    {   sonde_imet54_dec_t *probe = nullptr;                                                   // the option checks of the host decoder, before the device is touched
        const int rc = sonde_imet54_dec_create(opts, &probe);
        if (rc) return rc;
        sonde_imet54_dec_destroy(probe);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { fprintf(stderr, "libsonde_hip: no usable HIP device (the batched soft-bit framer has no CPU fallback)\n"); return SONDE_E_NOGPU; }
    sonde_softin_dev *s = new sonde_softin_dev();
    s->C = n_channels; s->type = SONDE_IMET54; s->i54_ecc = (opts->ecc || opts->json) ? 1 : 0;     // --json implies --ecc (imet54mod.c:899)
    s->cap = 4 * n_channels + 16;                              // frames a call can hold over all channels (sonde_fsk.h): a channel completes one per 2240 symbols at the most
    const size_t C = (size_t)n_channels, cap = (size_t)s->cap;
    for (size_t c = 0; c < C; c++) {
        sonde_imet54_dec_t *d = nullptr;
        if (sonde_imet54_dec_create(opts, &d)) { sonde_softin_dev_destroy(s); return SONDE_E_NOMEM; }
        s->i54_dec.push_back(d);
    }
    std::vector<SoftinImet54Chan> init(C);
    memset((void *)init.data(), 0, C * sizeof(SoftinImet54Chan));
    for (auto &c : init) c.inv = opts->inv ? 1 : 0;
    std::vector<uint32_t> tab(IMET54_TAB_N);
    imet54_crc_table(tab.data());
    bool ok = hipMalloc((void **)&s->d_i54_chan, C * sizeof(SoftinImet54Chan)) == hipSuccess && hipMalloc((void **)&s->d_i54_out, cap * sizeof(SoftinImet54Rec)) == hipSuccess
           && hipMalloc((void **)&s->d_i54_tab, IMET54_TAB_N * sizeof(uint32_t)) == hipSuccess && hipMalloc((void **)&s->d_count, 8) == hipSuccess
           && hipHostMalloc((void **)&s->h_count, 8) == hipSuccess && s->h_i54.alloc(cap);
    ok = ok && hipMemcpy(s->d_i54_chan, init.data(), C * sizeof(SoftinImet54Chan), hipMemcpyHostToDevice) == hipSuccess
            && hipMemcpy(s->d_i54_tab, tab.data(), IMET54_TAB_N * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) { sonde_softin_dev_destroy(s); return SONDE_E_NOMEM; }
    SoftinArgs &a = s->args;
    a.n_ch = n_channels; a.inv_in = invert_stream ? 1 : 0; a.opt_auto = opts->aut ? 1 : 0; a.ths = 0.8f; a.count = s->d_count; a.cap = s->cap;
    s->head = std::min(s->cap, n_channels + 16);               // (a frame a second and channel)
    (void)hipGetLastError();
    *out = s;
    return 0;
}

int sonde_softin_dev_create_meisei(int32_t n_channels, const sonde_meisei_opts_t *opts, int32_t invert_stream, sonde_softin_dev_t **out) {
    if (!out || n_channels < 1 || !opts) return SONDE_E_ARG;
    {   sonde_meisei_dec_t *probe = nullptr;                                                   // the option checks of the host decoder, before the device is touched
        const int rc = sonde_meisei_dec_create(opts, &probe);
        if (rc) return rc;
        sonde_meisei_dec_destroy(probe);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { fprintf(stderr, "libsonde_hip: no usable HIP device (the batched soft-bit framer has no CPU fallback)\n"); return SONDE_E_NOGPU; }
    sonde_softin_dev *s = new sonde_softin_dev();
    s->C = n_channels; s->type = SONDE_MEISEI; s->mei_ecc = (opts->ecc || opts->json) ? 1 : 0;     // --json implies --ecc (sonde_meisei.h)
    s->cap = 4 * n_channels + 16;                              // frames a call can hold over all channels (sonde_fsk.h): a channel completes one per 1200 half symbols at the most
    const size_t C = (size_t)n_channels, cap = (size_t)s->cap;
    for (size_t c = 0; c < C; c++) {
        sonde_meisei_dec_t *d = nullptr;
        if (sonde_meisei_dec_create(opts, &d)) { sonde_softin_dev_destroy(s); return SONDE_E_NOMEM; }
        s->mei_dec.push_back(d);
    }
    std::vector<SoftinMeiseiChan> init(C);
    memset((void *)init.data(), 0, C * sizeof(SoftinMeiseiChan));
    bool ok = hipMalloc((void **)&s->d_mei_chan, C * sizeof(SoftinMeiseiChan)) == hipSuccess && hipMalloc((void **)&s->d_mei_out, cap * sizeof(SoftinMeiseiRec)) == hipSuccess
           && hipMalloc((void **)&s->d_count, 8) == hipSuccess && hipHostMalloc((void **)&s->h_count, 8) == hipSuccess && s->h_mei.alloc(cap);
    ok = ok && hipMemcpy(s->d_mei_chan, init.data(), C * sizeof(SoftinMeiseiChan), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) { sonde_softin_dev_destroy(s); return SONDE_E_NOMEM; }
    SoftinArgs &a = s->args;
    a.n_ch = n_channels; a.inv_in = invert_stream ? 1 : 0; a.ths = 0.8f; a.count = s->d_count; a.cap = s->cap;
    s->head = std::min(s->cap, 2 * n_channels + 16);           // (two frames a second and channel)
    (void)hipGetLastError();
    *out = s;
    return 0;
}

int sonde_softin_dev_rs92_load_ephemeris(sonde_softin_dev_t *s, const char *path) {
    if (!s || s->type != SONDE_RS92 || !path) return SONDE_E_ARG;
    for (sonde_rs92_dec_t *d : s->r92_dec) { const int rc = sonde_rs92_dec_load_ephemeris(d, path); if (rc) return rc; }
    return 0;
}
int sonde_softin_dev_rs92_load_almanac(sonde_softin_dev_t *s, const char *path) {
    if (!s || s->type != SONDE_RS92 || !path) return SONDE_E_ARG;
    for (sonde_rs92_dec_t *d : s->r92_dec) { const int rc = sonde_rs92_dec_load_almanac(d, path); if (rc) return rc; }
    return 0;
}

void sonde_softin_dev_destroy(sonde_softin_dev_t *s) {
    if (!s) return;
    if (s->pending && s->pend_stream) (void)hipStreamSynchronize(s->pend_stream);
    if (s->own_stream && s->stream) { hipStreamSynchronize(s->stream); hipStreamDestroy(s->stream); }
    if (s->h_count) hipHostFree(s->h_count);
    if (s->h_nbits) hipHostFree(s->h_nbits);
    if (s->d_nbits) hipFree(s->d_nbits);
    (void)hipGetLastError();
    void *p[] = { s->d_chan, s->d_frames, s->d_hdr, s->d_gf, s->d_synd, s->d_flen, s->d_ecc, s->d_codes, s->d_meta, s->d_count, s->d_dfm_chan, s->d_dfm_out, s->d_m10_chan, s->d_m10_out, s->d_m20_chan, s->d_m20_out, s->d_drop_chan, s->d_drop_out, s->d_l6_chan, s->d_l6_out, s->d_l6_list, s->d_r92_chan, s->d_r92_out, s->d_i54_chan, s->d_i54_out, s->d_i54_tab, s->d_mei_chan, s->d_mei_out };
    for (void *q : p) if (q) hipFree(q);
    for (sonde_lms6_dec_t *d : s->l6_dec) sonde_lms6_dec_destroy(d);
    for (sonde_rs92_dec_t *d : s->r92_dec) sonde_rs92_dec_destroy(d);
    for (sonde_imet54_dec_t *d : s->i54_dec) sonde_imet54_dec_destroy(d);
    for (sonde_meisei_dec_t *d : s->mei_dec) sonde_meisei_dec_destroy(d);
    delete s;
}

// one pass of the framer (and rs41_ecc() over the frames it completes) over the channels of ch_list (null: all), its records behind the `off` records the
// call already has; counter `which` of d_count
static int softin_finish_lms6(sonde_softin_dev *s, hipStream_t st, long long n);
static int softin_pass(sonde_softin_dev *s, hipStream_t st, const int off, const int nblocks, const int *ch_list, const int which) {
    SoftinArgs a = s->args;
    if (s->type != SONDE_LMS6 && s->type != SONDE_RS92 && s->type != SONDE_IMET54 && s->type != SONDE_MEISEI) { a.frames += (size_t)off * 518; a.flen += off; a.meta += off; }
    a.cap = s->cap - off; a.count = s->d_count + which; a.ch_list = ch_list;
    HIPCHK(hipMemsetAsync(a.count, 0, 4, st));
    if (s->type == SONDE_DFM09) { SoftinDfmArgs d{a, s->d_dfm_chan, s->d_dfm_out + off, s->ecc_level}; hipLaunchKernelGGL(k_softin_dfm, dim3(nblocks), dim3(64), 0, st, d); }
    else if (s->type == SONDE_M10) {
        // LDS for the call's soft decisions: what a call can hold (a modem launch: its capacity; a pushed stream: its length), up to M10_STAGE_MAX
        long long need = a.fsk_chan || a.nbits_ch ? a.ch_stride : a.nbits;
        if (need > M10_STAGE_MAX || need < 0) need = 0;
        SoftinM10Args m{a, s->d_m10_chan, s->d_m10_out + off, (int)need};
        static size_t attr = 0;
        const size_t lds = (size_t)need * sizeof(float);
        if (lds > attr) { if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_softin_m10), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess) attr = lds; else m.stage_cap = 0; }
        hipLaunchKernelGGL(k_softin_m10, dim3(nblocks), dim3(64), m.stage_cap ? lds : 0, st, m);
    }
    else if (s->type == SONDE_M20) {
        // (LDS for the call's soft decisions as for M10)
        long long need = a.fsk_chan || a.nbits_ch ? a.ch_stride : a.nbits;
        if (need > M10_STAGE_MAX || need < 0) need = 0;
        SoftinM20Args m{a, s->d_m20_chan, s->d_m20_out + off, (int)need, s->m20_skip};
        static size_t attr = 0;
        const size_t lds = (size_t)need * sizeof(float);
        if (lds > attr) { if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_softin_m20), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess) attr = lds; else m.stage_cap = 0; }
        hipLaunchKernelGGL(k_softin_m20, dim3(nblocks), dim3(64), m.stage_cap ? lds : 0, st, m);
    }
    else if (s->type == SONDE_RS92) {
        // (LDS for the call's soft decisions as for M10)
        long long need = a.fsk_chan || a.nbits_ch ? a.ch_stride : a.nbits;
        if (need > M10_STAGE_MAX || need < 0) need = 0;
        SoftinRs92Args m{a, s->d_r92_chan, s->d_r92_out + off, s->d_gf, (int)need, s->r92_inv};
        static size_t attr = 0;
        const size_t lds = (size_t)need * sizeof(float);
        if (lds > attr) { if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_softin_rs92), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess) attr = lds; else m.stage_cap = 0; }
        hipLaunchKernelGGL(k_softin_rs92, dim3(nblocks), dim3(64), m.stage_cap ? lds : 0, st, m);
    }
    else if (s->type == SONDE_IMET54) {
        // (LDS for the call's soft decisions as for M10)
        long long need = a.fsk_chan || a.nbits_ch ? a.ch_stride : a.nbits;
        if (need > M10_STAGE_MAX || need < 0) need = 0;
        SoftinImet54Args m{a, s->d_i54_chan, s->d_i54_out + off, s->d_i54_tab, (int)need, s->i54_ecc};
        static size_t attr = 0;
        const size_t lds = (size_t)need * sizeof(float);
        if (lds > attr) { if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_softin_imet54), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess) attr = lds; else m.stage_cap = 0; }
        hipLaunchKernelGGL(k_softin_imet54, dim3(nblocks), dim3(64), m.stage_cap ? lds : 0, st, m);
    }
    else if (s->type == SONDE_MEISEI) {
        // (LDS for the call's soft decisions as for M10)
        long long need = a.fsk_chan || a.nbits_ch ? a.ch_stride : a.nbits;
        if (need > M10_STAGE_MAX || need < 0) need = 0;
        SoftinMeiseiArgs m{a, s->d_mei_chan, s->d_mei_out + off, (int)need, s->mei_ecc};
        static size_t attr = 0;
        const size_t lds = (size_t)need * sizeof(float);
        if (lds > attr) { if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_softin_meisei), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess) attr = lds; else m.stage_cap = 0; }
        hipLaunchKernelGGL(k_softin_meisei, dim3(nblocks), dim3(64), m.stage_cap ? lds : 0, st, m);
    }
    else if (s->type == SONDE_RD94RD41) { SoftinDropArgs d{a, s->d_drop_chan, s->d_drop_out + off, s->drop_inv}; hipLaunchKernelGGL(k_softin_drop, dim3(nblocks), dim3(64), 0, st, d); }
    else if (s->type == SONDE_LMS6) { SoftinLms6Args d{a, s->d_l6_chan, s->d_l6_out + off, s->l6_vit, s->l6_auto}; hipLaunchKernelGGL(k_softin_lms6, dim3(nblocks), dim3(64), 0, st, d); }
    else {
        hipLaunchKernelGGL(k_softin_rs41, dim3(nblocks), dim3(64), 0, st, a);
        if (s->ecc_level > 0)
            sonde_launch_rs41_ecc_batch_n(a.frames, a.flen, a.count, a.cap, s->ecc_level, s->d_ecc + off, s->d_codes + 2 * (size_t)off, s->d_synd + 48 * (size_t)off, s->d_gf, s->d_gf + 512, st);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s->h_count + which, a.count, 4, hipMemcpyDeviceToHost, st));
    return 0;
}
// records [from, to) of the call to the host
static int softin_copy(sonde_softin_dev *s, hipStream_t st, const int from, const int to) {
    if (to <= from) return 0;
    const size_t n = (size_t)(to - from);
    if (s->type == SONDE_DFM09) HIPCHK(hipMemcpyAsync(s->h_dfm.data() + from, s->d_dfm_out + from, n * sizeof(sonde_dfm_frame_t), hipMemcpyDeviceToHost, st));
    else if (s->type == SONDE_M10) HIPCHK(hipMemcpyAsync(s->h_m10.data() + from, s->d_m10_out + from, n * sizeof(sonde_m10_frame_t), hipMemcpyDeviceToHost, st));
    else if (s->type == SONDE_M20) HIPCHK(hipMemcpyAsync(s->h_m20.data() + from, s->d_m20_out + from, n * sizeof(sonde_m20_frame_t), hipMemcpyDeviceToHost, st));
    else if (s->type == SONDE_RD94RD41) HIPCHK(hipMemcpyAsync(s->h_drop.data() + from, s->d_drop_out + from, n * sizeof(DropFrame), hipMemcpyDeviceToHost, st));
    else if (s->type == SONDE_RS92) HIPCHK(hipMemcpyAsync(s->h_r92.data() + from, s->d_r92_out + from, n * sizeof(SoftinRs92Rec), hipMemcpyDeviceToHost, st));
    else if (s->type == SONDE_IMET54) HIPCHK(hipMemcpyAsync(s->h_i54.data() + from, s->d_i54_out + from, n * sizeof(SoftinImet54Rec), hipMemcpyDeviceToHost, st));
    else if (s->type == SONDE_MEISEI) HIPCHK(hipMemcpyAsync(s->h_mei.data() + from, s->d_mei_out + from, n * sizeof(SoftinMeiseiRec), hipMemcpyDeviceToHost, st));
    else if (s->type == SONDE_LMS6) HIPCHK(hipMemcpyAsync(s->h_l6.data() + from, s->d_l6_out + from, n * sizeof(Lms6Block), hipMemcpyDeviceToHost, st));
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
            const Lms6Block &b = s->h_l6[i];
            if (b.channel < 0 || b.channel >= s->C) continue;
            sonde_lms6_dec_t *d = s->l6_dec[(size_t)b.channel];
            sonde_lms6_softin_t r; memset(&r, 0, sizeof r);
            const float nanv = __builtin_nanf("");             // dsp_t stays zeroed with soft input: frm_rate and the elapsed time are 0 / 0
            const int len = sonde_lms6_dec_block_bytes(d, b.bytes, b.blen, b.pos, b.mv, nanv, (double)nanv, r.text, sizeof r.text);
            if (len < 0) return len;
            r.channel = b.channel; r.type = sonde_lms6_dec_type(d, nullptr); r.mv = b.mv; r.text_len = len; r.hdr_bit = b.hdr_bit; r.blen = b.blen; r.err = b.err;
            s->ql6.push_back(r);
            s->frames_total++;
            int64_t ok = 0;
            (void)sonde_lms6_dec_counts(d, nullptr, &ok);                 // the decoder's own tally of CRC-good frames, whatever the output form
            s->ecc_ok_total += ok - s->l6_ok[(size_t)b.channel]; s->l6_ok[(size_t)b.channel] = ok;
            const int want = sonde_lms6_dec_block_bits(d) + LMS6_BLOCKSTART;
            if (want != s->l6_len[(size_t)b.channel]) {
                s->l6_len[(size_t)b.channel] = want; s->h_l6_len[(size_t)b.channel] = want;
                HIPCHK(hipMemcpyAsync(&s->d_l6_chan[b.channel].rawblk_len, &s->h_l6_len[(size_t)b.channel], sizeof(int), hipMemcpyHostToDevice, st));
            }
            if (b.more && nlist < s->C) s->h_l6_list[(size_t)nlist++] = b.channel;
        }
        if (!nlist) return 0;
        HIPCHK(hipMemcpyAsync(s->d_l6_list, s->h_l6_list.data(), (size_t)nlist * sizeof(int), hipMemcpyHostToDevice, st));
        { const int rc = softin_pass(s, st, 0, nlist, s->d_l6_list, 0); if (rc) return rc; }
        { const int rc = softin_copy(s, st, 0, std::min(nlist, s->cap)); if (rc) return rc; }
        HIPCHK(hipStreamSynchronize(st));
        n = std::min<long long>(s->h_count[0], std::min(nlist, s->cap));
    }
}

// enqueue a call: the framer over what args.sd / nbits describe, the block code, the counter and the records a call normally completes (`head`) on their way to the host
static int softin_enqueue(sonde_softin_dev *s, hipStream_t st) {
    if (s->pending) return SONDE_E_ARG;
    { const int rc = softin_pass(s, st, 0, s->C, nullptr, 0); if (rc) return rc; }
    { const int rc = softin_copy(s, st, 0, s->head); if (rc) return rc; }
    s->pending = true; s->pend_stream = st;
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
    if (s->type == SONDE_RS92) {
        // (frames of one channel in order: the slots of a call are handed out in completion order per channel, channels interleave)
        for (long long i = 0; i < n; i++) {
            const SoftinRs92Rec &r = s->h_r92[i];
            if (r.channel < 0 || r.channel >= s->C) continue;
            s->qr92.push_back(r); s->frames_total++;
            if (r.ec >= 0) s->ecc_ok_total++;
            if (r.ec > 0) { s->repaired_total++; s->symbols_total += r.ec; }
        }
        return 0;
    }
    if (s->type == SONDE_IMET54) {
        for (long long i = 0; i < n; i++) {
            const SoftinImet54Rec &r = s->h_i54[i];
            if (r.channel < 0 || r.channel >= s->C) continue;
            s->qi54.push_back(r); s->frames_total++;
            // the JSON rule without the status bits (imet54mod.c:583): frm_ok and a check sum good, or every codeword of the standard frame clean
            if (r.ecc_frm >= 0 && (r.crc_std || r.crc_cont || r.ecc_std == 0)) s->ecc_ok_total++;
            if (r.ecc_frm > 0) { s->repaired_total++; s->symbols_total += r.ecc_frm; }
        }
        return 0;
    }
    if (s->type == SONDE_MEISEI) {
        for (long long i = 0; i < n; i++) {
            const SoftinMeiseiRec &r = s->h_mei[i];
            if (r.channel < 0 || r.channel >= s->C) continue;
            s->qmei.push_back(r); s->frames_total++;
            int bad = 0, fixed = 0;
            for (int k = 0; k < MEISEI_BLOCKS; k++) { if (r.block_err[k] >= 0xE) bad++; else fixed += r.block_err[k]; }
            if (!bad) s->ecc_ok_total++;
            if (fixed) { s->repaired_total++; s->symbols_total += fixed; }
        }
        return 0;
    }
    if (s->type == SONDE_DFM09) {
        // (frames of one channel in order: the slots of a call are handed out in completion order per channel, channels interleave)
        for (long long i = 0; i < n; i++) {
            const sonde_dfm_frame_t &f = s->h_dfm[i];
            s->qdfm.push_back(f); s->frames_total++;
            const bool okf = f.ecc[0] >= 0 && f.ecc[1] >= 0 && f.ecc[2] >= 0;
            if (okf) s->ecc_ok_total++;
            if (okf && (f.ecc[0] > 0 || f.ecc[1] > 0 || f.ecc[2] > 0)) { s->repaired_total++; s->symbols_total += __builtin_popcount((unsigned)f.ecc[0]) + __builtin_popcount((unsigned)f.ecc[1]) + __builtin_popcount((unsigned)f.ecc[2]); }
        }
    } else if (s->type == SONDE_M10) {
        for (long long i = 0; i < n; i++) { s->qm10.push_back(s->h_m10[i]); s->frames_total++; if (s->h_m10[i].cs_ok) s->ecc_ok_total++; }
    } else if (s->type == SONDE_M20) {
        for (long long i = 0; i < n; i++) { s->qm20.push_back(s->h_m20[i]); s->frames_total++; if (s->h_m20[i].cs_ok) s->ecc_ok_total++; }
    } else if (s->type == SONDE_RD94RD41) {
        for (long long i = 0; i < n; i++) {
            const DropFrame &g = s->h_drop[i];
            sonde_drop_frame_t f; memset(&f, 0, sizeof f);
            f.channel = g.channel; f.nraw = g.nraw; f.complete = g.complete; f.err94 = g.err94; f.err41 = g.err41; f.sample = g.sample;
            memcpy(f.bytes, g.bytes, sizeof f.bytes);
            s->qdrop.push_back(f); s->frames_total++;
            // print_frame's type choice and frm_ok (rd94rd41drop.c:1028-1038, :1213): more than two failing RD41 blocks = RD94
            if (__builtin_popcount((unsigned)g.err41) > 2 ? g.err94 == 0 : g.err41 == 0) s->ecc_ok_total++;
        }
    } else {
        for (long long i = 0; i < n; i++) {
            sonde_frame_t f; memset(&f, 0, sizeof f);
            const SoftinMeta &m = s->h_meta[i];
            f.channel = m.channel; f.len = m.len; f.nbytes = m.nbytes; f.mv = m.mv; f.mv_pos = (uint32_t)m.hdr_bit;
            f.ecc = s->ecc_level > 0 ? s->h_ecc[i] : 0;
            memcpy(f.frame, s->h_frames.data() + (size_t)i * 518, 518);
            s->queue.push_back(f);
            s->frames_total++;
            if (f.ecc >= 0) s->ecc_ok_total++;
            if (f.ecc > 0) { s->repaired_total++; s->symbols_total += f.ecc; }
        }
    }
    return 0;
}

// the modem's last launch (waited for first: its channels' frame counts come from the host's copy of the records, and whatever the modem had to repeat is repeated by
// then) as this call's input: the soft decisions where that launch left them, the bits per channel uploaded
static int softin_bind_fsk(sonde_softin_dev *s, sonde_fsk_t *modem, hipStream_t st) {
    const float *d_sd = nullptr; long long cap = 0; const FskChan *d_chan = nullptr; int bpf = 0, nch = 0; hipStream_t ms = nullptr;
    { const int rc = sonde_fsk_wait(modem); if (rc) return rc; }
    const int rc = sonde_fsk_dev_view(modem, &d_sd, &cap, &d_chan, &bpf, &nch, &ms);
    if (rc) return rc;
    if (nch != s->C) return SONDE_E_ARG;
    if (!s->h_nbits) {
        if (hipHostMalloc((void **)&s->h_nbits, (size_t)s->C * sizeof(int)) != hipSuccess || hipMalloc((void **)&s->d_nbits, (size_t)s->C * sizeof(int)) != hipSuccess) return SONDE_E_NOMEM;
    }
    { const int rc2 = sonde_fsk_host_frames(modem, s->h_nbits); if (rc2) return rc2; }
    for (int c = 0; c < s->C; c++) s->h_nbits[c] = s->h_nbits[c] > 0 ? s->h_nbits[c] * bpf : 0;
    HIPCHK(hipMemcpyAsync(s->d_nbits, s->h_nbits, (size_t)s->C * sizeof(int), hipMemcpyHostToDevice, st));
    SoftinArgs &a = s->args;
    a.sd = d_sd; a.ch_stride = cap; a.fsk_chan = nullptr; a.bits_per_frame = bpf; a.nbits_ch = s->d_nbits; a.nbits = 0;
    return 0;
}
static int softin_own_stream(sonde_softin_dev *s) {
    if (!s->stream) { HIPCHK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking)); s->own_stream = true; }
    return 0;
}
int sonde_softin_dev_push_fsk(sonde_softin_dev_t *s, sonde_fsk_t *modem) {
    if (!s || !modem) return SONDE_E_ARG;
    { const int rc = softin_finish(s); if (rc) return rc; }
    { const int rc = softin_own_stream(s); if (rc) return rc; }
    { const int rc = softin_bind_fsk(s, modem, s->stream); if (rc) return rc; }
    { const int rc = softin_enqueue(s, s->stream); if (rc) return rc; }
    { const int rc = sonde_fsk_dev_reader_done(modem, s->stream); if (rc) return rc; }
    return softin_finish(s);
}
// the same in two halves: submit waits for the modem's launch (sonde_fsk_wait), then enqueues the consumer's kernels and the copies of its frames on the consumer's OWN
// stream and returns; collect waits for them.  In between the modem can be given its next second (sonde_fsk_submit_device): the modem keeps the soft decisions of two
// launches (they alternate between two buffers), so the consumer of second k runs beside the modem of second k + 1.  Collect before the modem's launch after that.
int sonde_softin_dev_submit_fsk(sonde_softin_dev_t *s, sonde_fsk_t *modem) {
    if (!s || !modem) return SONDE_E_ARG;
    { const int rc = softin_finish(s); if (rc) return rc; }
    { const int rc = softin_own_stream(s); if (rc) return rc; }
    { const int rc = softin_bind_fsk(s, modem, s->stream); if (rc) return rc; }
    { const int rc = softin_enqueue(s, s->stream); if (rc) return rc; }
    // LMS6 with auto detection launches again per completed block and reads the soft decisions each time: the call is completed here, so that the point of the
    // stream the modem is told about below lies behind every read — whatever the caller does before sonde_softin_dev_collect
    if (s->type == SONDE_LMS6 && s->l6_auto) { const int rc = softin_finish(s); if (rc) return rc; }
    // the modem's launch that reuses this buffer of soft decisions (the next but one) waits for the consumer's kernels: submitting the modem twice before
    // sonde_softin_dev_collect is slower, not wrong
    return sonde_fsk_dev_reader_done(modem, s->stream);
}
// The consumer over the launch BEFORE the one the modem has in flight: for a caller that hands the modem its next second first (sonde_fsk_wait (k - 1),
// sonde_fsk_submit_device (k), then this for k - 1) — the modem's stream never waits for the host's decoder bookkeeping.  Nothing waits here; with no launch in
// flight this is sonde_softin_dev_submit_fsk.
int sonde_softin_dev_submit_fsk_behind(sonde_softin_dev_t *s, sonde_fsk_t *modem) {
    if (!s || !modem) return SONDE_E_ARG;
    { const int rc = softin_finish(s); if (rc) return rc; }
    { const int rc = softin_own_stream(s); if (rc) return rc; }
    if (!s->h_nbits) {
        if (hipHostMalloc((void **)&s->h_nbits, (size_t)s->C * sizeof(int)) != hipSuccess || hipMalloc((void **)&s->d_nbits, (size_t)s->C * sizeof(int)) != hipSuccess) return SONDE_E_NOMEM;
    }
    const float *d_sd = nullptr; long long cap = 0; int bpf = 0, nch = s->C;
    const int have = sonde_fsk_dev_view_prev(modem, &d_sd, &cap, &bpf, &nch, s->h_nbits);
    if (have < 0) return have;
    if (have == 0) return sonde_softin_dev_submit_fsk(s, modem);
    if (nch != s->C) return SONDE_E_ARG;
    for (int c = 0; c < s->C; c++) s->h_nbits[c] = s->h_nbits[c] > 0 ? s->h_nbits[c] * bpf : 0;
    HIPCHK(hipMemcpyAsync(s->d_nbits, s->h_nbits, (size_t)s->C * sizeof(int), hipMemcpyHostToDevice, s->stream));
    SoftinArgs &a = s->args;
    a.sd = d_sd; a.ch_stride = cap; a.fsk_chan = nullptr; a.bits_per_frame = bpf; a.nbits_ch = s->d_nbits; a.nbits = 0;
    { const int rc = softin_enqueue(s, s->stream); if (rc) return rc; }
    // (LMS6 with auto detection reads the soft decisions again in its later rounds, and the modem's launch in flight is the one that overwrites them next)
    if (s->type == SONDE_LMS6 && s->l6_auto) { const int rc = softin_finish(s); if (rc) return rc; }
    return sonde_fsk_dev_reader_done_prev(modem, s->stream);
}
int sonde_softin_dev_collect(sonde_softin_dev_t *s) {
    if (!s) return SONDE_E_ARG;
    return softin_finish(s);
}

int sonde_softin_dev_push_device(sonde_softin_dev_t *s, const float *d_soft, int64_t ch_stride, int32_t n_bits) {
    if (!s || !d_soft || n_bits < 0 || ch_stride < n_bits) return SONDE_E_ARG;
    { const int rc = softin_finish(s); if (rc) return rc; }
    if (!s->stream) { HIPCHK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking)); s->own_stream = true; }
    SoftinArgs &a = s->args;
    a.sd = d_soft; a.ch_stride = ch_stride; a.fsk_chan = nullptr; a.nbits_ch = nullptr; a.nbits = n_bits;
    { const int rc = softin_enqueue(s, s->stream); if (rc) return rc; }
    return softin_finish(s);
}

int sonde_softin_dev_fetch(sonde_softin_dev_t *s, sonde_frame_t *out, int32_t max) {
    if (s && (s->type == SONDE_RS92 || s->type == SONDE_IMET54 || s->type == SONDE_MEISEI)) return SONDE_E_ARG;
    if (s && s->pending) { const int rc_ = softin_finish(s); if (rc_) return rc_; }
    if (!s || (!out && max > 0)) return SONDE_E_ARG;
    const int n = (int)std::min<size_t>(s->queue.size(), (size_t)(max < 0 ? 0 : max));
    for (int i = 0; i < n; i++) out[i] = s->queue[i];
    s->queue.erase(s->queue.begin(), s->queue.begin() + n);
    return n;
}

int sonde_softin_dev_fetch_dfm(sonde_softin_dev_t *s, sonde_dfm_frame_t *out, int32_t max) {
    if (s && (s->type == SONDE_RS92 || s->type == SONDE_IMET54 || s->type == SONDE_MEISEI)) return SONDE_E_ARG;
    if (s && s->pending) { const int rc_ = softin_finish(s); if (rc_) return rc_; }
    if (!s || (!out && max > 0)) return SONDE_E_ARG;
    const int n = (int)std::min<size_t>(s->qdfm.size(), (size_t)(max < 0 ? 0 : max));
    for (int i = 0; i < n; i++) out[i] = s->qdfm[i];
    s->qdfm.erase(s->qdfm.begin(), s->qdfm.begin() + n);
    return n;
}

int sonde_softin_dev_fetch_m10(sonde_softin_dev_t *s, sonde_m10_frame_t *out, int32_t max) {
    if (s && (s->type == SONDE_RS92 || s->type == SONDE_IMET54 || s->type == SONDE_MEISEI)) return SONDE_E_ARG;
    if (s && s->pending) { const int rc_ = softin_finish(s); if (rc_) return rc_; }
    if (!s || (!out && max > 0)) return SONDE_E_ARG;
    const int n = (int)std::min<size_t>(s->qm10.size(), (size_t)(max < 0 ? 0 : max));
    for (int i = 0; i < n; i++) out[i] = s->qm10[i];
    s->qm10.erase(s->qm10.begin(), s->qm10.begin() + n);
    return n;
}

int sonde_softin_dev_set_m20_skip(sonde_softin_dev_t *s, int32_t skip) {
    if (!s || s->type != SONDE_M20) return SONDE_E_ARG;
    s->m20_skip = skip != 0;                       // (takes effect with the next call; a call in flight has its own copy)
    return 0;
}

int sonde_softin_dev_fetch_m20(sonde_softin_dev_t *s, sonde_m20_frame_t *out, int32_t max) {
    if (!s || s->type != SONDE_M20 || (!out && max > 0)) return SONDE_E_ARG;
    if (s->pending) { const int rc_ = softin_finish(s); if (rc_) return rc_; }
    const int n = (int)std::min<size_t>(s->qm20.size(), (size_t)(max < 0 ? 0 : max));
    for (int i = 0; i < n; i++) out[i] = s->qm20[i];
    s->qm20.erase(s->qm20.begin(), s->qm20.begin() + n);
    return n;
}

int sonde_softin_dev_fetch_drop(sonde_softin_dev_t *s, sonde_drop_frame_t *out, int32_t max) {
    if (s && (s->type == SONDE_RS92 || s->type == SONDE_IMET54 || s->type == SONDE_MEISEI)) return SONDE_E_ARG;
    if (s && s->pending) { const int rc_ = softin_finish(s); if (rc_) return rc_; }
    if (!s || (!out && max > 0)) return SONDE_E_ARG;
    const int n = (int)std::min<size_t>(s->qdrop.size(), (size_t)(max < 0 ? 0 : max));
    for (int i = 0; i < n; i++) out[i] = s->qdrop[i];
    s->qdrop.erase(s->qdrop.begin(), s->qdrop.begin() + n);
    return n;
}

int sonde_softin_dev_fetch_lms6(sonde_softin_dev_t *s, sonde_lms6_softin_t *out, int32_t max) {
    if (s && (s->type == SONDE_RS92 || s->type == SONDE_IMET54 || s->type == SONDE_MEISEI)) return SONDE_E_ARG;
    if (s && s->pending) { const int rc_ = softin_finish(s); if (rc_) return rc_; }
    if (!s || (!out && max > 0)) return SONDE_E_ARG;
    const int n = (int)std::min<size_t>(s->ql6.size(), (size_t)(max < 0 ? 0 : max));
    for (int i = 0; i < n; i++) out[i] = s->ql6[i];
    s->ql6.erase(s->ql6.begin(), s->ql6.begin() + n);
    return n;
}

int sonde_softin_dev_fetch_rs92(sonde_softin_dev_t *s, sonde_rs92_softin_t *out, int32_t max) {
    if (!s || s->type != SONDE_RS92 || (!out && max > 0)) return SONDE_E_ARG;
    if (s->pending) { const int rc_ = softin_finish(s); if (rc_) return rc_; }
    const int n = (int)std::min<size_t>(s->qr92.size(), (size_t)(max < 0 ? 0 : max));
    for (int i = 0; i < n; i++) {
        // print_frame behind rs92_ecc, by the channel's own decoder (its calibration rows, its orbit data): here, not in the push call, so that collect stays short
        const SoftinRs92Rec &r = s->qr92[i];
        sonde_rs92_softin_t &o = out[i];
        o.channel = r.channel; o.ec = r.ec; o.mv = r.mv; o.hdr_bit = r.hdr_bit;
        memcpy(o.frame, r.frame, sizeof o.frame);
        const int len = sonde_rs92_dec_corrected(s->r92_dec[(size_t)r.channel], r.frame, r.ec, o.text, sizeof o.text);
        o.text_len = len;                                      // (negative: the text did not fit; the frame is delivered all the same)
        if (len < 0) o.text[0] = 0;
    }
    s->qr92.erase(s->qr92.begin(), s->qr92.begin() + n);
    return n;
}

int sonde_softin_dev_fetch_imet54(sonde_softin_dev_t *s, sonde_imet54_softin_t *out, int32_t max) {
    if (!s || s->type != SONDE_IMET54 || (!out && max > 0)) return SONDE_E_ARG;
    if (s->pending) { const int rc_ = softin_finish(s); if (rc_) return rc_; }
    const int n = (int)std::min<size_t>(s->qi54.size(), (size_t)(max < 0 ? 0 : max));
    for (int i = 0; i < n; i++) {
        // print_frame behind the Hamming step, by the channel's own decoder and from the device's verdicts: here, not in the push call, so that collect stays short
        const SoftinImet54Rec &r = s->qi54[i];
        sonde_imet54_softin_t &o = out[i];
        o.channel = r.channel; o.ecc_frm = r.ecc_frm; o.ecc_tlm = r.ecc_tlm; o.ecc_std = r.ecc_std; o.crc = r.crc_std ? 1 : r.crc_cont ? 2 : 0; o.mv = r.mv; o.hdr_bit = r.hdr_bit;
        memcpy(o.frame, r.frame, sizeof o.frame);
        const int len = sonde_imet54_dec_decoded(s->i54_dec[(size_t)r.channel], r.frame, r.ecc_frm, r.ecc_tlm, r.ecc_std, r.crc_std, r.crc_cont, o.text, sizeof o.text);
        o.text_len = len;                                      // (negative: the text did not fit; the frame is delivered all the same)
        if (len < 0) o.text[0] = 0;
    }
    s->qi54.erase(s->qi54.begin(), s->qi54.begin() + n);
    return n;
}

int sonde_softin_dev_fetch_meisei(sonde_softin_dev_t *s, sonde_meisei_softin_t *out, int32_t max) {
    if (!s || s->type != SONDE_MEISEI || (!out && max > 0)) return SONDE_E_ARG;
    if (s->pending) { const int rc_ = softin_finish(s); if (rc_) return rc_; }
    const int n = (int)std::min<size_t>(s->qmei.size(), (size_t)(max < 0 ? 0 : max));
    for (int i = 0; i < n; i++) {
        // the printers behind the block loop, by the channel's own decoder and from the device's bits and verdicts: here, not in the push call, so that collect stays short
        const SoftinMeiseiRec &r = s->qmei[i];
        sonde_meisei_softin_t &o = out[i];
        o.channel = r.channel; o.mv = r.mv; o.hdr_bit = r.hdr_bit; o.err_frm = 0; o.err_blks = 0;
        for (int k = 0; k < MEISEI_BLOCKS; k++) { o.block_err[k] = r.block_err[k]; o.err_frm += r.block_err[k] >= 0xE; o.err_blks += r.block_err[k] != 0; }
        memcpy(o.bits, r.bits, sizeof o.bits);
        const int len = sonde_meisei_dec_decoded(s->mei_dec[(size_t)r.channel], r.bits, r.block_err, o.text, sizeof o.text);
        o.text_len = len;                                      // (negative: the text did not fit; the frame is delivered all the same)
        if (len < 0) o.text[0] = 0;
    }
    s->qmei.erase(s->qmei.begin(), s->qmei.begin() + n);
    return n;
}

int sonde_softin_dev_counts(sonde_softin_dev_t *s, int64_t *frames, int64_t *ecc_ok, int64_t *repaired, int64_t *symbols, int64_t *dropped) {
    if (s && s->pending) { const int rc_ = softin_finish(s); if (rc_) return rc_; }
    if (!s) return SONDE_E_ARG;
    if (frames) *frames = s->frames_total;
    if (ecc_ok) *ecc_ok = s->ecc_ok_total;
    if (repaired) *repaired = s->repaired_total;
    if (symbols) *symbols = s->symbols_total;
    if (dropped) *dropped = s->dropped;
    return 0;
}

}  // extern "C"
