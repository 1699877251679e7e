// LMS6-1680 / MkIIa printer (include/sonde_mk2a.h): host code, no GPU.  Mirrors mk2a1680mod.c print_frame :1950-2071 with bits2bytes :1742-1769,
// crc16_0 / check_CRC :1773-1826 and the field readers :1828-1948.  What the reference keeps in gpx between frames (the id, the last frame
// number and time, prev_frnr) lives in the printer object.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>

#include "../../include/sonde_hip.h"
#include "../../include/sonde_mk2a.h"

namespace {

constexpr int BITS = 10, FRAME_LEN = 176, BITFRAME_LEN = FRAME_LEN * BITS;
constexpr int OFS = 2;
constexpr int pos_SondeID = OFS + 0x02, pos_FrameNb = OFS + 0x04, pos_GPSTOW = OFS + 0x08, pos_GPSlat = OFS + 0x10, pos_GPSlon = OFS + 0x14,
              pos_GPSalt = OFS + 0x18, pos_GPSvO = OFS + 0x1C, pos_GPSvN = OFS + 0x1F, pos_GPSvV = OFS + 0x22, pos_FullID = OFS + 0x30;
const char weekday[7][4] = {"Sun", "Mon", "Tue", "Wed", "Thu", "Fri", "Sat"};

int32_t be32(const uint8_t *p) { return (int32_t)(((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]); }
int vel24(const uint8_t *p) {
    int v = p[0] << 16 | p[1] << 8 | p[2];
    if (v > 0x7FFFFF) v -= 0x1000000;
    return v;
}

}  // namespace

struct sonde_mk2a_printer {
    sonde_mk2a_opts_t o;
    uint8_t bytes[FRAME_LEN + 8];        // check_CRC reads up to two bytes behind a full-length frame (zero padding of the reference's struct)
    int frnr, prev_frnr;
    uint32_t id;
    int wday, std_, min;
    float sek;
    double lat, lon, alt, vH, vD, vV;
    std::string out;

    void put(const char *fmt, ...) __attribute__((format(printf, 2, 3))) {
        char tmp[640];
        va_list ap;
        va_start(ap, fmt);
        const int n = vsnprintf(tmp, sizeof tmp, fmt, ap);
        va_end(ap);
        out.append(tmp, n < (int)sizeof tmp ? n : (int)sizeof tmp - 1);
    }
    int crc_err(int len) const {
        const uint32_t crcdat = (bytes[len] << 8) | bytes[len + 1];
        return crcdat != (uint32_t)sonde_mk2a_crc16(bytes, len);
    }
};

extern "C" int sonde_mk2a_crc16(const uint8_t *b, int32_t len) {
    int rem = 0;
    for (int i = 0; i < len; i++) {
        rem ^= b[i] << 8;
        for (int j = 0; j < 8; j++) {
            rem = (rem & 0x8000) ? (rem << 1) ^ 0x1021 : rem << 1;
            rem &= 0xFFFF;
        }
    }
    return rem;
}

extern "C" int sonde_mk2a_printer_create(const sonde_mk2a_opts_t *opts, sonde_mk2a_printer_t **out) {
    if (!opts || !out) return SONDE_E_ARG;
    auto *p = new (std::nothrow) sonde_mk2a_printer();
    if (!p) return SONDE_E_NOMEM;
    p->o = *opts;
    p->o.version[sizeof p->o.version - 1] = 0;
    if (p->o.json) { p->o.crc = 1; if (!p->o.vbs) p->o.vbs = 1; }           // main :2205-2209
    memset(p->bytes, 0, sizeof p->bytes);
    p->frnr = p->prev_frnr = 0; p->id = 0; p->wday = p->std_ = p->min = 0; p->sek = 0;
    p->lat = p->lon = p->alt = p->vH = p->vD = p->vV = 0;
    *out = p;
    return 0;
}

extern "C" void sonde_mk2a_printer_destroy(sonde_mk2a_printer_t *p) { delete p; }

extern "C" int sonde_mk2a_print_frame(sonde_mk2a_printer_t *p, const uint8_t *bits, int32_t len, float mv, double df, char *outbuf, size_t outlen) {
    if (!p || !bits || !outbuf || outlen < 1 || len < 2 * BITS || len > BITFRAME_LEN) return SONDE_E_ARG;
    p->out.clear();
    uint8_t *fb = p->bytes;
    // bits2bytes: 8N1, data bits LSB first; a byte the bit string ends in is dropped, the rest of the frame is zero
    int nbytes = 0;
    while (nbytes < FRAME_LEN && nbytes * BITS + BITS - 1 <= len) {
        int v = 0;
        for (int i = 1; i < BITS - 1; i++) if (bits[nbytes * BITS + i] & 1) v |= 1 << (i - 1);
        fb[nbytes++] = (uint8_t)v;
    }
    for (int i = nbytes; i < FRAME_LEN; i++) fb[i] = 0;
    int flen = len / BITS;
    while (flen > 2 && fb[flen - 1] == 0xCA) flen--;                          // trailing fill
    int crc_err = p->crc_err(flen - 2);
    if (crc_err) {                                                            // CRC bytes that look like fill
        crc_err = p->crc_err(flen - 1);
        if (crc_err == 0) flen += 1;
        else {
            crc_err = p->crc_err(flen);
            if (crc_err == 0) flen += 2;
        }
    }
    const sonde_mk2a_opts_t &o = p->o;
    if (o.raw) {
        for (int i = 0; i < flen; i++) p->put("%02x ", fb[i]);
        if (o.crc) p->put(crc_err == 0 ? " [OK]" : " [NO]");
        p->put("\n");
    }
    if (fb[OFS] == 0x4D && len / BITS > pos_FullID + 4) {
        if (!crc_err && fb[pos_SondeID] == fb[pos_FullID] && fb[pos_SondeID + 1] == fb[pos_FullID + 1])
            p->id = ((uint32_t)fb[pos_FullID + 2] << 24) | ((uint32_t)fb[pos_FullID + 3] << 16) | ((uint32_t)fb[pos_FullID] << 8) | fb[pos_FullID + 1];
    }
    if (fb[OFS] == 0x54 && len / BITS > pos_GPSalt + 4) {
        p->frnr = (fb[pos_FrameNb] << 8) + fb[pos_FrameNb + 1];
        {                                                                     // get_GPStime
            int gpstime = be32(fb + pos_GPSTOW);
            const float ms = (float)(gpstime % 1000);
            gpstime /= 1000;
            const int day = gpstime / (24 * 3600);
            gpstime %= (24 * 3600);
            if (!(day < 0 || day > 6)) {
                p->wday = day;
                p->std_ = gpstime / 3600;
                p->min = (gpstime % 3600) / 60;
                p->sek = (float)(gpstime % 60 + ms / 1000.0);
            }
        }
        p->lat = be32(fb + pos_GPSlat) / (double)0xB60B60;
        p->lon = be32(fb + pos_GPSlon) / (double)0xB60B60;
        p->alt = be32(fb + pos_GPSalt) / 1000.0;
        if (o.vbs >= 2) {
            p->put("<");
            p->put("s=%+.2f", mv);
            if (o.show_df) {
                p->put(" Df=%+.1fkHz", df / 1e3);
                if (o.vbs == 3) {
                    p->put(" (IF=%+.4f,", df / (double)o.if_rate);
                    p->put("IQ=%+.4f)", df / (double)(uint32_t)o.sample_rate);
                }
            }
            p->put("> ");
        }
        if (!crc_err) {
            const uint32_t id16 = (fb[pos_SondeID] << 8) | fb[pos_SondeID + 1];
            if ((p->id & 0xFFFF) != id16) p->id = id16;
        }
        if (o.vbs && !crc_err) {
            if (p->id & 0xFFFF0000) p->put(" (%u)", p->id);
            else if (p->id) p->put(" (0x%04X)", p->id);
        }
        p->put(" [%5d] ", p->frnr);
        p->put("%s ", weekday[p->wday]);
        p->put("%02d:%02d:%06.3f ", p->std_, p->min, p->sek);
        p->put(" lat: %.5f ", p->lat);
        p->put(" lon: %.5f ", p->lon);
        p->put(" alt: %.2fm ", p->alt);
        {                                                                     // get_GPSvel24
            const double vx = vel24(fb + pos_GPSvO) / 1e3, vy = vel24(fb + pos_GPSvN) / 1e3, vz = vel24(fb + pos_GPSvV) / 1e3;
            p->vH = std::sqrt(vx * vx + vy * vy);
            double dir = std::atan2(vx, vy) * 180 / M_PI;
            if (dir < 0) dir += 360;
            p->vD = dir;
            p->vV = vz;
        }
        p->put("  vH: %.1fm/s  D: %.1f  vV: %.1fm/s ", p->vH, p->vD, p->vV);
        if (o.crc) p->put(crc_err == 0 ? " [OK]" : " [NO]");
        p->put("\n");
        if (o.json && crc_err == 0 && (p->id & 0xFFFF0000) && p->prev_frnr != p->frnr) {
            p->put("{ \"type\": \"%s\"", "LMS");
            p->put(", \"frame\": %d, \"id\": \"LMS6-%d\", \"datetime\": \"%02d:%02d:%06.3fZ\", \"lat\": %.5f, \"lon\": %.5f, \"alt\": %.5f, \"vel_h\": %.5f, \"heading\": %.5f, \"vel_v\": %.5f",
                   p->frnr, (int)p->id, p->std_, p->min, p->sek, p->lat, p->lon, p->alt, p->vH, p->vD, p->vV);
            p->put(", \"subtype\": \"%s\"", "MK2A");
            if (o.jsn_freq_khz > 0) p->put(", \"freq\": %d", o.jsn_freq_khz);
            p->put(", \"ref_datetime\": \"%s\"", "GPS");
            p->put(", \"ref_position\": \"%s\"", "GPS");
            if (o.version[0]) p->put(", \"version\": \"%s\"", o.version);
            p->put(" }\n");
            p->put("\n");
            p->prev_frnr = p->frnr;
        }
    }
    if (p->out.size() + 1 > outlen) return SONDE_E_RANGE;
    memcpy(outbuf, p->out.data(), p->out.size());
    outbuf[p->out.size()] = 0;
    return (int)p->out.size();
}
