// iMet-4 / iMet-1-RS printer (include/sonde_imet4.h): host code, no GPU.  Mirrors imet4iq.c print_frame :1206-1315 with bits2byte /
// bits2bytes :873-897, print_rawbits :899-906, crc16 :911-928, print_ePTU :973-1017, print_eGPS :1048-1118, print_xdata :1143-1200.
// State that the reference keeps in globals lives in the printer object: byteframe (bytes behind the end of the byte frame keep what
// earlier frames left there, the packet readers can reach them) and gpx (last valid values).
#include <cmath>
#include <new>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/sonde_hip.h"
#include "../../include/sonde_imet4.h"

namespace {

constexpr int BITS = 10;
constexpr int LEN_BYTEFRAME = 1200 / BITS;
constexpr int PKT_PTU = 0x01, PKT_GPS = 0x02, PKT_XDATA = 0x03, PKT_ePTU = 0x04, PKT_eGPS = 0x05;
constexpr int pos_PCKnum = 0x02, pos_PTUprs = 0x04, pos_PTUtem = 0x07, pos_PTUhum = 0x09, pos_PTUbat = 0x0B, pos_PTUcrc = 0x0C,
              pos_ePTUcrc = 0x12;
constexpr int pos_GPSlat = 0x02, pos_GPSlon = 0x06, pos_GPSalt = 0x0A, pos_GPSsats = 0x0C, pos_GPStim = 0x0D, pos_GPScrc = 0x10;
constexpr int pos_eGPSvE = 0x0D, pos_eGPSvN = 0x11, pos_eGPSvU = 0x15, pos_eGPStim = 0x19, pos_eGPScrc = 0x1C;
#define DEG "\xC2\xB0"

struct Gpx {
    int hour, min, sec;
    float lat, lon;
    int alt, sats;
    float vH, vD, vV;
    int frame;
    float temp, pressure, humidity, batt;
    char xdata[2 * LEN_BYTEFRAME + 1];
    char *paux;
    int gps_valid, ptu_valid;
};

}  // namespace

struct sonde_imet4_printer {
    sonde_imet4_opts_t o;
    uint8_t bytes[LEN_BYTEFRAME + 40];   // a packet starting near the end of a 100-byte frame is read up to 29 bytes on (zeros here)
    Gpx gpx;
    std::string out;

    void put(const char *fmt, ...) __attribute__((format(printf, 2, 3))) {
        char tmp[512];
        va_list ap;
        va_start(ap, fmt);
        const int n = vsnprintf(tmp, sizeof tmp, fmt, ap);
        va_end(ap);
        out.append(tmp, n < (int)sizeof tmp ? n : (int)sizeof tmp - 1);
    }
    int print_eptu(int pos, int id);
    int print_egps(int pos, int id);
    int print_xdata(int pos, int N);
};

extern "C" int sonde_imet4_crc16(const uint8_t *b, int32_t len) {
    int rem = 0x1D0F;
    for (int i = 0; i < len; i++) {
        rem ^= b[i] << 8;
        for (int j = 0; j < 8; j++) {
            rem = (rem & 0x8000) ? (rem << 1) ^ 0x1021 : rem << 1;
            rem &= 0xFFFF;
        }
    }
    return rem;
}

int sonde_imet4_printer::print_eptu(int pos, int id) {
    const uint8_t *f = bytes + pos;
    const int pcrc = id == PKT_ePTU ? pos_ePTUcrc : pos_PTUcrc;
    const int crc_val = (f[pcrc] << 8) | f[pcrc + 1];
    const int crc = sonde_imet4_crc16(f, pcrc);
    const int P = f[pos_PTUprs] | (f[pos_PTUprs + 1] << 8) | (f[pos_PTUprs + 2] << 16);
    const short T = (short)(f[pos_PTUtem] | (f[pos_PTUtem + 1] << 8));
    const int U = f[pos_PTUhum] | (f[pos_PTUhum + 1] << 8);
    const int bat = f[pos_PTUbat];
    const int pcknum = f[pos_PCKnum] | (f[pos_PCKnum + 1] << 8);
    put("[%d] ", pcknum);
    put(" P:%.2fmb ", P / 100.0);
    put(" T:%.2f" DEG "C ", T / 100.0);
    put(" U:%.2f%% ", U / 100.0);
    put(" bat:%.1fV ", bat / 10.0);
    put(" # ");
    put(" CRC: %04X ", crc_val);
    put("- %04X ", crc);
    if (crc_val == crc) {
        put("[OK]");
        gpx.ptu_valid = id;
        gpx.frame = pcknum;
        gpx.pressure = (float)(P / 100.0);
        gpx.temp = (float)(T / 100.0);
        gpx.humidity = (float)(U / 100.0);
        gpx.batt = (float)(bat / 10.0);
    } else {
        put("[NO]");
        gpx.ptu_valid = 0;
    }
    put("\n");
    return crc_val != crc;
}

int sonde_imet4_printer::print_egps(int pos, int id) {
    const uint8_t *f = bytes + pos;
    const int ptim = id == PKT_GPS ? pos_GPStim : pos_eGPStim;
    // the CRC is read at the GPS packet's offset for eGPS too (imet4iq.c:1058-1059)
    const int crc_val = (f[pos_GPScrc] << 8) | f[pos_GPScrc + 1];
    const int crc = sonde_imet4_crc16(f, pos_GPScrc);
    float lat, lon, vE, vN, vU, vH = 0, vD = 0;
    memcpy(&lat, f + pos_GPSlat, 4);
    memcpy(&lon, f + pos_GPSlon, 4);
    const int alt = (f[pos_GPSalt + 1] << 8) + f[pos_GPSalt] - 5000;
    const int sats = f[pos_GPSsats];
    const int std_ = f[ptim], min = f[ptim + 1], sek = f[ptim + 2];
    put("(%02d:%02d:%02d) ", std_, min, sek);
    put(" lat: %.6f" DEG " ", lat);
    put(" lon: %.6f" DEG " ", lon);
    put(" alt: %dm ", alt);
    put(" sats: %d ", sats);
    gpx.vH = gpx.vD = gpx.vV = 0;
    if (id == PKT_eGPS) {
        memcpy(&vE, f + pos_eGPSvE, 4);
        memcpy(&vN, f + pos_eGPSvN, 4);
        memcpy(&vU, f + pos_eGPSvU, 4);
        vH = sqrtf(vE * vE + vN * vN);
        vD = (float)(atan2((double)vE, (double)vN) * 180.0 / M_PI);
        if (vD < 0) vD = (float)(vD + 360.0);
        put("  vH: %.1fm/s  D: %.1f" DEG "  vV: %.1fm/s ", vH, vD, vU);
    }
    put(" # ");
    put(" CRC: %04X ", crc_val);
    put("- %04X ", crc);
    if (crc_val == crc) {
        put("[OK]");
        gpx.gps_valid = id;
        gpx.lat = lat; gpx.lon = lon; gpx.alt = alt; gpx.sats = sats;
        gpx.hour = std_; gpx.min = min; gpx.sec = sek;
        if (id == PKT_eGPS) { gpx.vH = vH; gpx.vD = vD; gpx.vV = vU; }
    } else {
        put("[NO]");
        gpx.gps_valid = 0;
    }
    put("\n");
    return crc_val != crc;
}

int sonde_imet4_printer::print_xdata(int pos, int N) {
    const uint8_t *f = bytes + pos;
    const int crc_len = 3 + N;
    const int crc_val = (f[crc_len] << 8) | f[crc_len + 1];
    const int crc = sonde_imet4_crc16(f, crc_len);
    put(" XDATA ");
    if (N == 8 && f[3] == 0x01) {                       // ozonesonde, big-endian fields
        const unsigned short Icell = (unsigned short)(f[6] | (f[5] << 8));
        const short Tpump = (short)(f[8] | (f[7] << 8));
        put(" Icell:%.3fuA ", Icell / 1000.0);
        put(" Tpump:%.2f" DEG "C ", Tpump / 100.0);
        put(" Ipump:%dmA ", (int)f[9]);
        put(" Vbat:%.1fV ", f[10] / 10.0);
    } else {
        put(" (N=0x%02X)", N);
        for (int j = 0; j < N; j++) put(" %02X", f[3 + j]);
    }
    if (crc_val == crc && (gpx.paux - gpx.xdata) + 2 * (N + 1) < 2 * LEN_BYTEFRAME) {
        if (gpx.paux > gpx.xdata) { *gpx.paux = '#'; gpx.paux += 1; }
        for (int j = 0; j < N; j++) { snprintf(gpx.paux, 3, "%02X", f[3 + j]); gpx.paux += 2; }
        *gpx.paux = '\0';
    }
    put(" # ");
    put(" CRC: %04X ", crc_val);
    put("- %04X ", crc);
    put(crc_val == crc ? "[OK]" : "[NO]");
    put("\n");
    return crc_val != crc;
}

extern "C" int sonde_imet4_printer_create(const sonde_imet4_opts_t *opts, sonde_imet4_printer_t **out) {
    if (!opts || !out) return SONDE_E_ARG;
    auto *p = new (std::nothrow) sonde_imet4_printer();
    if (!p) return SONDE_E_NOMEM;
    p->o = *opts;
    p->o.version[sizeof p->o.version - 1] = '\0';
    memset(p->bytes, 0, sizeof p->bytes);
    memset(&p->gpx, 0, sizeof p->gpx);
    p->gpx.paux = p->gpx.xdata;
    *out = p;
    return 0;
}

extern "C" void sonde_imet4_printer_destroy(sonde_imet4_printer_t *p) { delete p; }

extern "C" int sonde_imet4_print_frame(sonde_imet4_printer_t *p, const uint8_t *bits, int32_t nbits, char *outbuf, size_t outlen) {
    if (!p || !bits || !outbuf || nbits < 0 || nbits > 1200) return SONDE_E_ARG;
    p->out.clear();
    const int len = nbits / BITS;
    if (len >= 2 && len <= LEN_BYTEFRAME) {
        Gpx &g = p->gpx;
        for (int i = len; i < LEN_BYTEFRAME; i++) p->bytes[i] = 0;
        g.gps_valid = 0;
        g.ptu_valid = 0;
        int framelen;
        for (framelen = 0; framelen < len; framelen++) {          // bits2bytes: 8N1, LSB first; ten ones end the byte frame
            const uint8_t *b = bits + BITS * framelen;
            int s = 0, byte = 0;
            for (int i = 0; i < BITS; i++) s += b[i];
            if (s == 10) byte = 0xFFFF;
            else for (int i = 1, d = 1; i < BITS - 1; i++, d <<= 1) if (b[i] == 1) byte += d;
            p->bytes[framelen] = byte & 0xFF;
            if (byte == 0xFFFF) break;
        }
        if (p->o.rawbits) {
            for (int i = 0; i < framelen * BITS; i++) {
                if (i % BITS == 1 || i % BITS == BITS - 1) p->out += ' ';
                p->put("%d", bits[i]);
            }
            p->out += '\n';
        } else {
            int out = 0;
            if (p->o.raw) {
                for (int i = 0; i < framelen; i++) p->put("%02X ", p->bytes[i]);
                p->out += '\n';
                out |= 8;
            }
            int ofs = 0;
            g.xdata[0] = '\0';
            g.paux = g.xdata;
            while (ofs < framelen && p->bytes[ofs] == 0x01) {
                const int id = p->bytes[ofs + 1];
                if (id == PKT_GPS || id == PKT_eGPS) {
                    p->print_egps(ofs, id);
                    ofs += (id == PKT_GPS ? pos_GPScrc : pos_eGPScrc) + 2;
                    out |= 1;
                } else if (id == PKT_ePTU || id == PKT_PTU) {
                    p->print_eptu(ofs, id);
                    ofs += (id == PKT_ePTU ? pos_ePTUcrc : pos_PTUcrc) + 2;
                    out |= 2;
                } else if (id == PKT_XDATA) {
                    const int N = p->bytes[ofs + 2];
                    if (N > 0 && ofs + 2 + N + 2 < framelen) {
                        p->print_xdata(ofs, N);
                        ofs += N + 3 + 2;
                        out |= 4;
                    } else break;
                } else break;
            }
            if (p->o.json && g.gps_valid && g.ptu_valid) {
                p->put("{ \"type\": \"%s\"", "IMET");
                p->put(", \"frame\": %d, \"id\": \"iMet\", \"datetime\": \"%02d:%02d:%02dZ\", \"lat\": %.5f, \"lon\": %.5f, \"alt\": %d, \"sats\": %d, "
                       "\"temp\": %.2f, \"humidity\": %.2f, \"pressure\": %.2f, \"batt\": %.1f",
                       g.frame, g.hour, g.min, g.sec, g.lat, g.lon, g.alt, g.sats, g.temp, g.humidity, g.pressure, g.batt);
                if (g.xdata[0]) p->put(", \"aux\": \"%s\"", g.xdata);
                if (p->o.jsn_freq_khz > 0) p->put(", \"freq\": %d", p->o.jsn_freq_khz);
                p->put(", \"ref_datetime\": \"%s\"", "GPS");
                p->put(", \"ref_position\": \"%s\"", "MSL");
                if (p->o.version[0]) p->put(", \"version\": \"%s\"", p->o.version);
                p->put(" }\n");
            }
            if (out) p->out += '\n';
        }
    }
    if (p->out.size() + 1 > outlen) return SONDE_E_RANGE;
    memcpy(outbuf, p->out.data(), p->out.size());
    outbuf[p->out.size()] = '\0';
    return (int)p->out.size();
}
