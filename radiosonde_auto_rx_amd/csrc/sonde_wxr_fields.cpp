// sonde_wxr_fields.cpp — host-only part of include/sonde_wxr.h: the printer (print_frame of the reference's weathex/weathex301d.c:359-527), on a frame's bits
// (sonde_wxr_print_frame) or on a record of the device soft-bit consumer (sonde_wxr_print_decoded), and the --softin bit loop of its main (:607-648) for one
// stream.  No GPU.
#include "../../include/sonde_hip.h"
#include "../../include/sonde_wxr.h"
#include "../../include/sonde_fsk.h"
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <deque>
#include <new>
#include <string>

namespace {

constexpr int FRAMELEN = 69, HEADLEN = 40;

// PN9 whitening sequence of the format, 64 bytes from frame byte 6 on (TI SWRA322)
const uint8_t PN9b[64] = { 0xFF, 0x87, 0xB8, 0x59, 0xB7, 0xA1, 0xCC, 0x24, 0x57, 0x5E, 0x4B, 0x9C, 0x0E, 0xE9, 0xEA, 0x50,
                           0x2A, 0xBE, 0xB4, 0x1B, 0xB6, 0xB0, 0x5D, 0xF1, 0xE6, 0x9A, 0xE3, 0x45, 0xFD, 0x2C, 0x53, 0x18,
                           0x0C, 0xCA, 0xC9, 0xFB, 0x49, 0x37, 0xE5, 0xA8, 0x51, 0x3B, 0x2F, 0x61, 0xAA, 0x72, 0x18, 0x84,
                           0x02, 0x23, 0x23, 0xAB, 0x63, 0x89, 0x51, 0xB3, 0xE7, 0x8B, 0x72, 0x90, 0x4C, 0xE8, 0xFB, 0xC1 };

const uint8_t HDR[2][5] = { { 0xAA, 0xAA, 0xAA, 0x2D, 0xD4 }, { 0xAA, 0xAA, 0xAA, 0xC1, 0x94 } };

void put(std::string &s, const char *fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    const int n = vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (n > 0) s.append(buf, (size_t)n);
}

uint32_t xor8sum(const uint8_t *b, int len) {
    uint8_t x = 0, s = 0;
    for (int j = 0; j < len; j++) { x ^= b[j]; s = (uint8_t)(s + b[j]); }
    return ((uint32_t)x << 8) | s;
}

}  // namespace

struct sonde_wxr_printer {
    sonde_wxr_opts_t o{};
    // gpx_t: what outlives a frame
    uint32_t sn1 = 0, cnt1 = 0, sn2 = 0, cnt2 = 0;
    int chk1ok = 0, chk2ok = 0;
    uint8_t hrs = 0, min = 0, sec = 0;
    float lat = 0, lon = 0, alt = 0;
};

extern "C" int sonde_wxr_xor8sum(const uint8_t *bytes, int32_t len) {
    if (!bytes || len < 0) return SONDE_E_ARG;
    return (int)xor8sum(bytes, len);
}

extern "C" int sonde_wxr_printer_create(const sonde_wxr_opts_t *opts, sonde_wxr_printer_t **out) {
    if (!opts || !out) return SONDE_E_ARG;
    auto *p = new (std::nothrow) sonde_wxr_printer();
    if (!p) return SONDE_E_NOMEM;
    p->o = *opts;
    p->o.version[sizeof p->o.version - 1] = 0;
    *out = p;
    return 0;
}

extern "C" void sonde_wxr_printer_destroy(sonde_wxr_printer_t *p) { delete p; }

// what a frame's text is made from: the bytes behind PN9, the check as computed and as stored, the verdict, frame id, serial and counter — from the frame's bits
// (sonde_wxr_print_frame) or as the device left them (sonde_wxr_print_decoded)
struct WxrDecoded { const uint8_t *x; int chkval, chkdat, chk_ok; uint8_t frid; uint32_t sn, cnt; };

// print_frame behind the verdict (:377-527); bit(j) = the character -R prints for frame bit j
template <class BitF>
static int wxr_print(sonde_wxr_printer_t *p, const WxrDecoded &d, const BitF &bit, const std::string &prefix, char *out, size_t outlen) {
    const sonde_wxr_opts_t &o = p->o;
    const int ofs = o.pn9 ? 8 : 6;
    const uint8_t *x = d.x;
    const int chkval = d.chkval, chkdat = d.chkdat, chk_ok = d.chk_ok;
    std::string s = prefix;
    if (o.raw) {
        if (o.raw == 1) {
            for (int j = 0; j < FRAMELEN; j++) put(s, "%02X ", x[j]);
            put(s, " #  %s", chk_ok ? "[OK]" : "[NO]");
            if (o.vbs) put(s, " # [%04X:%04X]", chkdat, chkval);
        } else {
            for (int j = 0; j < SONDE_WXR_BITS; j++) s.push_back(bit(j));
        }
        s.push_back('\n');
    } else {
        const uint32_t sn = d.sn, cnt = d.cnt;
        const uint8_t frid = d.frid;
        if (frid == 1) {
            p->chk1ok = chk_ok; p->sn1 = sn; p->cnt1 = cnt;
            if (o.vbs) {
                put(s, " (%u) ", sn);
                put(s, " [%5d] ", cnt);
                put(s, "  %s", chk_ok ? "[OK]" : "[NO]");
                put(s, " # [%04X:%04X]", chkdat, chkval);
                s.push_back('\n');
            }
        } else if (frid == 2) {
            p->chk2ok = chk_ok; p->sn2 = sn; p->cnt2 = cnt;
            put(s, " (%u) ", sn);
            put(s, " [%5d] ", cnt);
            int hms = x[ofs + 7] | (x[ofs + 8] << 8) | (x[ofs + 9] << 16);
            hms &= 0x3FFFF;
            const uint8_t h = (uint8_t)(hms / 10000), m = (uint8_t)((hms % 10000) / 100), sc = (uint8_t)(hms % 100);
            put(s, " %02d:%02d:%02d ", h, m, sc);
            p->hrs = h; p->min = m; p->sec = sc;
            int val = x[ofs + 13] | (x[ofs + 14] << 8) | (x[ofs + 15] << 16);
            val >>= 4;
            val &= 0x7FFFF;
            const int val_alt = val;
            const float alt = val / 10.0f;
            put(s, " alt: %.1f ", alt);
            p->alt = alt;
            val = (int)(x[ofs + 15] | (x[ofs + 16] << 8) | (x[ofs + 17] << 16) | ((uint32_t)x[ofs + 18] << 24));
            val >>= 7;
            val &= 0x1FFFFFF;
            const int val_lat = val;
            const float lat = val / 1e5f;
            put(s, " lat: %.4f ", lat);
            p->lat = lat;
            val = (int)(x[ofs + 19] | (x[ofs + 20] << 8) | (x[ofs + 21] << 16) | ((uint32_t)x[ofs + 22] << 24));
            val &= 0x3FFFFFF;
            const int val_lon = val;
            const float lon = val / 1e5f;
            put(s, " lon: %.4f ", lon);
            p->lon = lon;
            const bool zero_pos = val_alt == 0 && val_lat == 0 && val_lon == 0;
            put(s, "  %s", chk_ok ? "[OK]" : "[NO]");
            if (o.vbs) put(s, " # [%04X:%04X]", chkdat, chkval);
            s.push_back('\n');
            // the checksum is weak: JSON only if the id-1 frame before agrees on serial and counter
            if (o.json && p->chk2ok && !zero_pos && p->chk1ok && p->sn2 == p->sn1 && p->cnt2 == p->cnt1) {
                put(s, "{ \"type\": \"%s\"", "WXR301");
                put(s, ", \"frame\": %u", p->cnt2);
                put(s, ", \"id\": \"WXR-%u\"", p->sn2);
                put(s, ", \"datetime\": \"%02d:%02d:%02dZ\", \"lat\": %.5f, \"lon\": %.5f, \"alt\": %.2f", p->hrs, p->min, p->sec, p->lat, p->lon, p->alt);
                if (o.pn9) put(s, ", \"subtype\": \"WXR_PN9\"");
                if (o.jsn_freq_khz > 0) put(s, ", \"freq\": %d", o.jsn_freq_khz);
                put(s, ", \"ref_datetime\": \"%s\"", "UTC");
                put(s, ", \"ref_position\": \"%s\"", "MSL");
                if (o.version[0]) put(s, ", \"version\": \"%s\"", o.version);
                put(s, " }\n");
                put(s, "\n");
            }
        }
    }
    if (s.size() + 1 > outlen) return SONDE_E_RANGE;
    memcpy(out, s.data(), s.size());
    out[s.size()] = 0;
    return (int)s.size();
}

extern "C" int sonde_wxr_print_frame(sonde_wxr_printer_t *p, const uint8_t *bits, char *out, size_t outlen) {
    if (!p || !bits || !out) return SONDE_E_ARG;
    const sonde_wxr_opts_t &o = p->o;
    const int ofs = o.pn9 ? 8 : 6;
    uint8_t x[FRAMELEN + 1];
    for (int j = 0; j < FRAMELEN; j++) {                                    // bits2bytes, MSB first; whatever is not '1' counts as 0
        int v = 0;
        for (int i = 0; i < 8; i++) v = (v << 1) | (bits[8 * j + i] == 1);
        if (o.pn9 && j >= 6) v ^= PN9b[(j - 6) % 64];
        x[j] = (uint8_t)v;
    }
    WxrDecoded d;
    d.x = x;
    d.chkval = (int)xor8sum(x + ofs, 53);
    d.chkdat = (x[ofs + 53] << 8) | x[ofs + 54];
    d.chk_ok = d.chkdat == d.chkval;
    d.sn = x[ofs] | (x[ofs + 1] << 8) | (x[ofs + 2] << 16) | ((uint32_t)x[ofs + 3] << 24);
    d.cnt = x[ofs + 4] | (x[ofs + 5] << 8);
    d.frid = x[ofs + 6];
    return wxr_print(p, d, [bits](int j) { return bits[j] == 0 ? '0' : bits[j] == 1 ? '1' : '\0'; }, std::string(), out, outlen);
}

extern "C" int sonde_wxr_print_decoded(sonde_wxr_printer_t *p, const sonde_wxr_softin_rec_t *rec, char *out, size_t outlen) {
    if (!p || !rec || !out) return SONDE_E_ARG;
    const WxrDecoded d{rec->x, (int)rec->chkval, (int)rec->chkdat, rec->chk_ok ? 1 : 0, rec->frid, rec->sn, rec->cnt};
    std::string prefix;
    // the --softin loop's -t (main :628): bits read before the matching one over the bit rate, printed when the header is found
    if (p->o.ts) put(prefix, "<%8.3f> ", (double)rec->hdr_bit / (double)(p->o.pn9 ? 5000 : 4800));
    const uint8_t *raw = rec->raw;
    return wxr_print(p, d, [raw](int j) { return (raw[j >> 3] >> (7 - (j & 7))) & 1 ? '1' : '0'; }, prefix, out, outlen);
}

// ------------------------------------------------------------------ --softin (main :607-648)
struct sonde_wxr_softin {
    int pn9 = 0, inv = 0, found = 0, bit_count = 0;
    uint64_t hist = 0, count = 0, t_hdr = 0;          // the last 40 bits (buf); bits read
    int hist_n = 0;                                    // bits in hist, up to 40 (buf starts as 'x' / NUL: no match before 40 bits)
    uint64_t hdr = 0;
    uint8_t frame[SONDE_WXR_BITS];
    std::deque<sonde_wxr_frame_t> done;
};

extern "C" int sonde_wxr_softin_create(int32_t pn9, int32_t invert, sonde_wxr_softin_t **out) {
    if (!out) return SONDE_E_ARG;
    auto *s = new (std::nothrow) sonde_wxr_softin();
    if (!s) return SONDE_E_NOMEM;
    s->pn9 = pn9 ? 1 : 0; s->inv = invert ? 1 : 0;
    for (int i = 0; i < 5; i++) s->hdr = (s->hdr << 8) | HDR[s->pn9][i];
    memset(s->frame, SONDE_WXR_BIT_UNSET, sizeof s->frame);
    *out = s;
    return 0;
}

extern "C" void sonde_wxr_softin_destroy(sonde_wxr_softin_t *s) { delete s; }

static void softin_frame(const sonde_wxr_softin *s, int complete, sonde_wxr_frame_t &f) {
    memset(&f, 0, sizeof f);
    f.nbits = complete ? SONDE_WXR_BITS : s->bit_count; f.complete = complete; f.sample = s->t_hdr;
    memcpy(f.bits, s->frame, sizeof f.bits);
}

extern "C" int sonde_wxr_softin_push(sonde_wxr_softin_t *s, const float *soft, int32_t n, sonde_wxr_frame_t *out, int32_t max) {
    if (!s || (!soft && n > 0) || n < 0 || (!out && max > 0) || max < 0) return SONDE_E_ARG;
    const uint64_t mask = (1ULL << HEADLEN) - 1;
    for (int i = 0; i < n; i++) {
        const int bit = s->inv ? (soft[i] <= 0.0f) : (soft[i] >= 0.0f);
        s->hist = ((s->hist << 1) | (uint64_t)bit) & mask;
        if (s->hist_n < HEADLEN) s->hist_n++;
        if (!s->found) {
            if (s->hist_n == HEADLEN && s->hist == s->hdr) {
                s->found = 1;
                s->t_hdr = s->count;
                for (int k = 0; k < HEADLEN; k++) s->frame[k] = (uint8_t)((s->hdr >> (HEADLEN - 1 - k)) & 1);
                s->bit_count += HEADLEN;
            }
        } else {
            s->frame[s->bit_count++] = (uint8_t)bit;
        }
        if (s->bit_count >= SONDE_WXR_BITS) {
            sonde_wxr_frame_t f;
            softin_frame(s, 1, f);
            s->done.push_back(f);
            s->bit_count = 0; s->found = 0;
        }
        s->count++;
    }
    int k = 0;
    while (k < max && !s->done.empty()) { out[k++] = s->done.front(); s->done.pop_front(); }
    return k;
}

extern "C" int sonde_wxr_softin_finish(sonde_wxr_softin_t *s, sonde_wxr_frame_t *out) {
    if (!s || !out) return SONDE_E_ARG;
    if (!s->found) return 0;
    softin_frame(s, 0, *out);
    return 1;
}
