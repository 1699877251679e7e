// sonde_drop_fields.cpp — host-only part of include/sonde_drop.h: the printer (print_frame of the reference's dropsonde/rd94rd41drop.c
// :1013-1251 with the getBlock_* / get_* readers in front of it), the check words, the --softin bit loop of its main (:1357-1386) and the
// --rawhex line reader (:1450-1458).  No GPU.
#include "../../include/sonde_hip.h"
#include "../../include/sonde_drop.h"
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <deque>
#include <new>
#include <string>

namespace {

constexpr int FRAME_LEN = SONDE_DROP_FRAME_LEN, RAWBITS = SONDE_DROP_RAWBITS, HEADLEN = 40, BITS = 10;
constexpr int RD41 = 41, RD94 = 94;
// FC 1D as Manchester-coded 8N1: header[HEADOFS..] of the reference
const char HDR40[] = "10101001010101010101" "10011001010110101001";

// byte positions (the reference's pos_* with OFS = 2)
constexpr int OFS = 2;
constexpr int pos_FrameNb = OFS + 0x01, pos_sensorP = OFS + 0x05, pos_sensorT = OFS + 0x09, pos_sensorU1 = OFS + 0x0D, pos_sensorU2 = OFS + 0x11;
constexpr int pos_GPSTOW = OFS + 0x18, pos_GPSweek = OFS + 0x20, pos_GPSecefX = OFS + 0x24, pos_GPSpAcc = OFS + 0x30, pos_GPSecefV1 = OFS + 0x34;
constexpr int pos_GPSsAcc1 = OFS + 0x40, pos_GPSsats1 = OFS + 0x46, pos_GPSecefV2 = OFS + 0x4A, pos_GPSsAcc2 = OFS + 0x56, pos_GPSsats2 = OFS + 0x5A;
constexpr int pos94_ID = OFS + 0x5D, pos94_bat = OFS + 0x66, pos94_sensorTi = OFS + 0x68;
constexpr int pos_chkFrNb = pos_FrameNb - 1 + 3, pos_chkPTU = pos_sensorP + 17, pos_chkGPS1 = pos_GPSTOW + 47, pos_chkGPS2 = pos_GPSecefV2 - 1 + 18;
constexpr int pos_chkInt = pos94_ID + 21;
constexpr int pos_pckFrm = OFS + 0x00, pos_pckPTU = OFS + 0x05, pos_CCC = OFS + 0x17, pos_DDD = OFS + 0x2A, pos_EEE = OFS + 0x38, pos_FFF = OFS + 0x47;
constexpr int pos_pckIDint = OFS + 0x64;
constexpr int pos41_ID = pos_pckIDint, pos41_bat = pos_pckIDint + 0x6, pos41_sensorTi = pos_pckIDint + 0x8;

void put(std::string &s, const char *fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    const int n = vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (n > 0) s.append(buf, (size_t)n);
}

unsigned chksum16(const uint8_t *bytes, int len) {
    unsigned sum1 = 0, sum2 = 0;
    for (int i = 0; i < len; i++) {
        sum1 = (sum1 + bytes[i]) % 0x100;
        sum2 = (sum2 + sum1) % 0x100;
    }
    return sum2 | (sum1 << 8);
}

unsigned crc16(const uint8_t *bytes, int len) {
    int rem = 0;
    for (int i = 0; i < len; i++) {
        rem ^= bytes[i] << 8;
        for (int j = 0; j < 8; j++) {
            rem = (rem & 0x8000) ? (rem << 1) ^ 0x1021 : rem << 1;
            rem &= 0xFFFF;
        }
    }
    return (unsigned)rem;
}

unsigned word_at(const uint8_t *b, int pos) { return ((unsigned)b[pos] << 8) | b[pos + 1]; }

// block tables: start, length of the checked bytes; the check word follows them, high byte first
const int BLK94[5][2] = { { pos_chkFrNb - 3, 3 }, { pos_chkPTU - 17, 17 }, { pos_chkGPS1 - 47, 47 }, { pos_chkGPS2 - 18, 18 }, { pos_chkInt - 21, 21 } };
const int BLK41[7][2] = { { pos_pckFrm, 3 }, { pos_pckPTU, 16 }, { pos_CCC, 17 }, { pos_DDD, 12 }, { pos_EEE, 13 }, { pos_FFF, 27 }, { pos_pckIDint, 14 } };

unsigned geterr_rd94(const uint8_t *b) {
    unsigned err = 0;
    for (int i = 0; i < 5; i++) if (word_at(b, BLK94[i][0] + BLK94[i][1]) != chksum16(b + BLK94[i][0], BLK94[i][1])) err |= 1u << i;
    return err;
}

unsigned geterr_rd41(const uint8_t *b) {
    unsigned err = 0;
    for (int i = 0; i < 7; i++) if (word_at(b, BLK41[i][0] + BLK41[i][1]) != crc16(b + BLK41[i][0], BLK41[i][1])) err |= 1u << i;
    return err;
}

float float32_rd94(const uint8_t *b) {
    unsigned num = 0, val;
    float f;
    for (int i = 0; i < 4; i++) num |= (unsigned)b[i] << (24 - 8 * i);
    val = (num & 0x800000) << 8;
    val |= (num >> 1) & 0x7F800000;
    val |= num & 0x7FFFFF;
    memcpy(&f, &val, 4);
    return f;
}

float float32_le(const uint8_t *b) {
    unsigned num = 0;
    float f;
    for (int i = 0; i < 4; i++) num |= (unsigned)b[i] << (8 * i);
    memcpy(&f, &num, 4);
    return f;
}

int i32_le(const uint8_t *b) { int v; memcpy(&v, b, 4); return v; }

const double EARTH_a = 6378137.0, EARTH_b = 6356752.31424518;
const double EARTH_a2_b2 = EARTH_a * EARTH_a - EARTH_b * EARTH_b;
const double e2 = EARTH_a2_b2 / (EARTH_a * EARTH_a), ee2 = EARTH_a2_b2 / (EARTH_b * EARTH_b);

void ecef2elli(const double X[], double *lat, double *lon, double *alt) {
    const double a = EARTH_a, b = EARTH_b;
    const double lam = atan2(X[1], X[0]);
    const double p = sqrt(X[0] * X[0] + X[1] * X[1]);
    const double t = atan2(X[2] * a, p * b);
    const double phi = atan2(X[2] + ee2 * b * sin(t) * sin(t) * sin(t), p - e2 * a * cos(t) * cos(t) * cos(t));
    const double R = a / sqrt(1 - e2 * sin(phi) * sin(phi));
    *alt = p / cos(phi) - R;
    *lat = phi * 180 / M_PI;
    *lon = lam * 180 / M_PI;
}

const char weekday[7][4] = { "Sun", "Mon", "Tue", "Wed", "Thu", "Fri", "Sat" };

// gpx_t: everything print_frame reads; it outlives a frame (a field that a frame does not set keeps its value)
struct Gpx {
    int frnr = 0;
    unsigned id = 0;
    int week = 0, gpstow = 0, gpssec = 0, jahr = 0, monat = 0, tag = 0, wday = 0, std = 0, min = 0, sek = 0, ms = 0, cs = 0;
    double lat = 0, lon = 0, alt = 0, X = 0, Y = 0, Z = 0, pAcc = 0, vX1 = 0, vY1 = 0, vZ1 = 0, sAcc1 = 0;
    int sats = 0;
    double vN = 0, vE = 0, vU = 0, vH = 0, vD = 0, vV = 0, vX2 = 0, vY2 = 0, vZ2 = 0, sAcc2 = 0;
    int sats2 = 0;
    double alt2 = 0, vH2 = 0, vD2 = 0, vV2 = 0, P = 0, T = 0, U1 = 0, U2 = 0, bat = 0, iT = 0;
    int type = RD41;
};

void Gps2Date(Gpx &g) {
    long GpsDays, Mjd, J, C, Y, M;
    GpsDays = g.week * 7 + (g.gpssec / 86400);
    Mjd = 44244 + GpsDays;
    J = Mjd + 2468570;
    C = 4 * J / 146097;
    J = J - (146097 * C + 3) / 4;
    Y = 4000 * (J + 1) / 1461001;
    J = J - 1461 * Y / 4 + 31;
    M = 80 * J / 2447;
    g.tag = J - 2447 * M / 80;
    J = M / 11;
    g.monat = M + 2 - (12 * J);
    g.jahr = 100 * (C - 49) + Y + J;
}

void getBlock_GPS_rd94(Gpx &g, const uint8_t *fb) {
    g.week = fb[pos_GPSweek] + (fb[pos_GPSweek + 1] << 8);
    {   // get_GPStime_rd94
        int gpstime = i32_le(fb + pos_GPSTOW);
        g.gpstow = gpstime;
        g.ms = gpstime % 1000;
        gpstime /= 1000;
        g.gpssec = g.gpstow / 1000;
        g.cs = g.ms / 10;
        const int day = gpstime / (24 * 3600);
        gpstime %= (24 * 3600);
        if (!(day < 0 || day > 6)) {
            g.wday = day;
            g.std = gpstime / 3600;
            g.min = (gpstime % 3600) / 60;
            g.sek = gpstime % 60;
        }
    }
    double X[3], V[3], lat, lon, alt;
    for (int k = 0; k < 3; k++) X[k] = i32_le(fb + pos_GPSecefX + 4 * k) / 100.0;
    ecef2elli(X, &lat, &lon, &alt);
    g.lat = lat; g.lon = lon; g.alt = alt;
    g.pAcc = i32_le(fb + pos_GPSpAcc) / 100.0;
    g.X = X[0]; g.Y = X[1]; g.Z = X[2];
    // get_GPSvel_rd94
    for (int k = 0; k < 3; k++) V[k] = i32_le(fb + pos_GPSecefV1 + 4 * k) / 100.0;
    g.vX1 = V[0]; g.vY1 = V[1]; g.vZ1 = V[2];
    g.sats = fb[pos_GPSsats1];
    const double phi = g.lat * M_PI / 180.0, lam = g.lon * M_PI / 180.0;
    g.vN = -V[0] * sin(phi) * cos(lam) - V[1] * sin(phi) * sin(lam) + V[2] * cos(phi);
    g.vE = -V[0] * sin(lam) + V[1] * cos(lam);
    g.vU = V[0] * cos(phi) * cos(lam) + V[1] * cos(phi) * sin(lam) + V[2] * sin(phi);
    g.vH = sqrt(g.vN * g.vN + g.vE * g.vE);
    double dir = atan2(g.vE, g.vN) * 180 / M_PI;
    if (dir < 0) dir += 360;
    g.vD = dir;
    g.vV = g.vU;
    g.sAcc1 = i32_le(fb + pos_GPSsAcc1) / 100.0;
    for (int k = 0; k < 3; k++) V[k] = i32_le(fb + pos_GPSecefV2 + 4 * k) / 100.0;
    g.vX2 = V[0]; g.vY2 = V[1]; g.vZ2 = V[2];
    g.sats2 = fb[pos_GPSsats2];
    g.sAcc2 = i32_le(fb + pos_GPSsAcc2) / 100.0;
}

void getBlock_GPS_rd41(Gpx &g, const uint8_t *fb) {
    g.std = fb[pos_CCC + 9] & 0x1F;
    g.min = fb[pos_CCC + 10];
    g.sek = fb[pos_CCC + 11];
    g.cs = fb[pos_CCC + 12];
    g.ms = g.cs * 10;
    const int lat_i4 = (int)(((unsigned)fb[pos_DDD] << 24) | (fb[pos_DDD + 1] << 16) | (fb[pos_DDD + 2] << 8) | fb[pos_DDD + 3]);
    const int lon_i4 = (int)(((unsigned)fb[pos_DDD + 4] << 24) | (fb[pos_DDD + 5] << 16) | (fb[pos_DDD + 6] << 8) | fb[pos_DDD + 7]);
    g.lat = lat_i4 / 1e7;
    g.lon = lon_i4 / 1e7;
    const short vH1 = (short)((fb[pos_CCC + 0] << 8) | fb[pos_CCC + 1]);
    const short D1 = (short)((fb[pos_CCC + 2] << 8) | fb[pos_CCC + 3]);
    const short V1 = (short)((fb[pos_CCC + 4] << 8) | fb[pos_CCC + 5]);
    int alt1 = (fb[pos_CCC + 6] << 16) | (fb[pos_CCC + 7] << 8) | fb[pos_CCC + 8];
    if (alt1 & 0x800000) alt1 -= 0x1000000;
    g.sats = fb[pos_CCC + 13];
    const short vH2 = (short)((fb[pos_EEE + 0] << 8) | fb[pos_EEE + 1]);
    const short D2 = (short)((fb[pos_EEE + 2] << 8) | fb[pos_EEE + 3]);
    const short V2 = (short)((fb[pos_EEE + 4] << 8) | fb[pos_EEE + 5]);
    int alt2 = (fb[pos_EEE + 6] << 16) | (fb[pos_EEE + 7] << 8) | fb[pos_EEE + 8];
    if (alt2 & 0x800000) alt2 -= 0x1000000;
    g.sats2 = fb[pos_EEE + 9];
    g.vH = vH1 / 100.0; g.vD = D1 / 100.0; g.vV = -V1 / 100.0; g.alt = alt1 / 100.0;
    g.vH2 = vH2 / 100.0; g.vD2 = D2 / 100.0; g.vV2 = -V2 / 100.0; g.alt2 = alt2 / 100.0;
}

// -R: where the RD94 line gets a blank behind byte i (print_frame :1049-1068)
bool r94_blank(int i) {
    static const int at[] = { -1, 0, 2, 4, 8, 12, 16, 20, 21, 23, 27, 31, 33, 35, 39, 43, 47, 51, 55, 59, 63, 67, 69, 70, 72, 73, 77, 81, 85, 89, 90,
                              92, 96, 98, 101, 103, 107, 113, 115 };
    for (int v : at) if (i == OFS + v) return true;
    return false;
}

}  // namespace

struct sonde_drop_printer {
    sonde_drop_opts_t o{};
    Gpx g;
    int auto_type = 1, last_json = 0;
};

extern "C" uint32_t sonde_drop_chksum16(const uint8_t *bytes, int32_t len) { return bytes && len >= 0 ? chksum16(bytes, len) : 0; }
extern "C" uint32_t sonde_drop_crc16(const uint8_t *bytes, int32_t len) { return bytes && len >= 0 ? crc16(bytes, len) : 0; }

extern "C" int sonde_drop_errs(const uint8_t *bytes, int32_t *err94, int32_t *err41) {
    if (!bytes) return SONDE_E_ARG;
    if (err94) *err94 = (int32_t)geterr_rd94(bytes);
    if (err41) *err41 = (int32_t)geterr_rd41(bytes);
    return 0;
}

extern "C" int sonde_drop_rawhex(const char *line, uint8_t *bytes) {
    if (!line || !bytes) return SONDE_E_ARG;
    char buf[2 * FRAME_LEN + 4];
    strncpy(buf, line, sizeof buf - 1);
    buf[sizeof buf - 1] = 0;
    buf[2 * FRAME_LEN + 1] = 0;
    const int len = (int)(strlen(buf) / 2);
    int i;
    for (i = 0; i < len; i++) sscanf(buf + 2 * i, "%2hhx", bytes + i);        // a pair that is no hex number leaves the byte as it was
    for (i = len; i < FRAME_LEN; i++) bytes[i] = 0;
    return bytes[0] == 0xFC && bytes[1] == 0x1D;
}

extern "C" int sonde_drop_printer_create(const sonde_drop_opts_t *opts, sonde_drop_printer_t **out) {
    if (!opts || !out || (opts->type != 0 && opts->type != RD41 && opts->type != RD94)) return SONDE_E_ARG;
    auto *p = new (std::nothrow) sonde_drop_printer();
    if (!p) return SONDE_E_NOMEM;
    p->o = *opts;
    p->o.version[sizeof p->o.version - 1] = 0;
    p->auto_type = opts->type == 0;
    p->g.type = opts->type ? opts->type : RD41;
    *out = p;
    return 0;
}

extern "C" void sonde_drop_printer_destroy(sonde_drop_printer_t *p) { delete p; }

extern "C" int sonde_drop_printer_last(const sonde_drop_printer_t *p, int32_t *type, int32_t *json_printed) {
    if (!p) return SONDE_E_ARG;
    if (type) *type = p->g.type;
    if (json_printed) *json_printed = p->last_json;
    return 0;
}

extern "C" int sonde_drop_print_frame(sonde_drop_printer_t *p, const uint8_t *fb, char *out, size_t outlen) {
    if (!p || !fb || !out) return SONDE_E_ARG;
    const sonde_drop_opts_t &o = p->o;
    Gpx &g = p->g;
    std::string s;
    p->last_json = 0;

    unsigned err_rd94 = ~0u, err_rd41 = ~0u;
    if (g.type == RD94 || p->auto_type) err_rd94 = geterr_rd94(fb);
    if (g.type == RD41 || p->auto_type) err_rd41 = geterr_rd41(fb);
    if (p->auto_type) {
        // the reference counts the RD94 failures into num_errs41 (:1034), so num_errs94 stays 0: more than two failing RD41 blocks = RD94
        int num_errs41 = 0;
        g.type = RD41;
        for (int i = 0; i < 7; i++) num_errs41 += (err_rd41 >> i) & 1;
        if (num_errs41 > 2) g.type = RD94;
    }

    if (o.raw) {
        for (int i = 0; i < FRAME_LEN; i++) {
            put(s, "%02x", fb[i]);
            if (o.raw != 2) continue;
            if (g.type == RD94) {
                if (r94_blank(i)) s += " ";
                for (int k = 0; k < 5; k++) {
                    const int chk = BLK94[k][0] + BLK94[k][1];
                    if (i == chk - BLK94[k][1] - 1) s += " ";
                    if (i == chk + 1) put(s, "[%04X] ", chksum16(fb + BLK94[k][0], BLK94[k][1]));
                }
                if (i == pos_chkInt + 1) s += " ";
            } else if (g.type == RD41) {
                if (i == OFS - 1) s += "  ";
                for (int k = 0; k < 7; k++) {
                    if (i == BLK41[k][0] + BLK41[k][1] - 1) s += " ";
                    if (i == BLK41[k][0] + BLK41[k][1] + 1) put(s, " [%04X]  ", crc16(fb + BLK41[k][0], BLK41[k][1]));
                }
            }
        }
        if (o.raw == 2) {
            s += "  # chk: ";
            if (g.type == RD94) for (int i = 0; i < 5; i++) put(s, "%d", (err_rd94 >> i) & 1);
            else if (g.type == RD41) for (int i = 0; i < 7; i++) put(s, "%d", (err_rd41 >> i) & 1);
        }
        s += "\n";
    } else {
        const bool is41 = g.type == RD41;
        // getBlock_FrNb, getBlock_PTU, getBlock_GPS, getBlock_Int: the fields are read whatever the checks say
        g.frnr = is41 ? fb[pos_FrameNb + 1] + (fb[pos_FrameNb] << 8) : fb[pos_FrameNb] + (fb[pos_FrameNb + 1] << 8);
        float (*f32p)(const uint8_t *) = is41 ? float32_le : float32_rd94;
        g.P = f32p(fb + pos_sensorP); g.T = f32p(fb + pos_sensorT); g.U1 = f32p(fb + pos_sensorU1); g.U2 = f32p(fb + pos_sensorU2);
        if (is41) getBlock_GPS_rd41(g, fb); else getBlock_GPS_rd94(g, fb);
        const int pos_ID = is41 ? pos41_ID : pos94_ID;
        g.id = 0;
        for (int i = 0; i < 4; i++) g.id |= (unsigned)fb[pos_ID + i] << (24 - 8 * i);
        g.iT = f32p(fb + (is41 ? pos41_sensorTi : pos94_sensorTi));
        const int pos_bat = is41 ? pos41_bat : pos94_bat;
        g.bat = (is41 ? (fb[pos_bat] << 8) | fb[pos_bat + 1] : fb[pos_bat] | (fb[pos_bat + 1] << 8)) / 1e3;

        if (g.type == RD94 && !(err_rd94 & 0x17)) {
            Gps2Date(g);
            put(s, "[%5d] ", g.frnr);
            put(s, "%s", weekday[g.wday]);
            put(s, " %04d-%02d-%02d", g.jahr, g.monat, g.tag);
            put(s, " %02d:%02d:%02d.%03d", g.std, g.min, g.sek, g.ms);
            if (o.vbs) put(s, " (W %d)", g.week);
            s += "  ";
            put(s, " lat: %.5f° ", g.lat);
            put(s, " lon: %.5f° ", g.lon);
            put(s, " alt: %.2fm ", g.alt);
            if (o.vbs == 2) put(s, " (E:%.2fm) ", g.pAcc);
            if (o.vbs) put(s, " sats: %2d ", g.sats);
            if (o.vbs == 2) {
                put(s, " V1: (%5.2f,%5.2f,%5.2f) ", g.vX1, g.vY1, g.vZ1);
                put(s, "(E:%.2fm/s) ", g.sAcc1);
            }
            put(s, " vH: %.2fm/s  D: %.1f°  vV: %.2fm/s ", g.vH, g.vD, g.vV);
            if (o.vbs == 2 && !(err_rd94 & 0x08)) {
                put(s, " ENU=(%.2f,%.2f,%.2f) ", g.vE, g.vN, g.vU);
                put(s, " V2: (%5.2f,%5.2f,%5.2f) ", g.vX2, g.vY2, g.vZ2);
                put(s, "(E:%.2fm/s) ", g.sAcc2);
                put(s, " sats2: %2d ", g.sats2);
            }
            s += "  ";
            put(s, " P=%.2fhPa ", g.P);
            put(s, " T=%.2f°C ", g.T);
            put(s, " H1=%.2f%% ", g.U1);
            put(s, " H2=%.2f%% ", g.U2);
            s += " ";
            put(s, " (%09d) ", (int)g.id);
            if (o.vbs == 2) {
                s += " ";
                put(s, " Ti=%.2f°C ", g.iT);
                put(s, " Bat=%.2fV ", g.bat);
            }
            s += "  # chk: ";
            for (int i = 0; i < 5; i++) put(s, "%d", (err_rd94 >> i) & 1);
            s += "\n";
        } else if (g.type == RD41 && !(err_rd41 & 0x4F)) {
            put(s, "[%5d] ", g.frnr);
            put(s, " %02d:%02d:%02d.%02d", g.std, g.min, g.sek, g.cs);
            s += "  ";
            put(s, " lat: %.5f° ", g.lat);
            put(s, " lon: %.5f° ", g.lon);
            put(s, " alt: %.2fm ", g.alt);
            put(s, " vH: %.2fm/s  D: %.1f°  vV: %.2fm/s ", g.vH, g.vD, g.vV);
            if (o.vbs) put(s, " sats: %2d ", g.sats);
            if (o.vbs && !(err_rd41 & 0x10)) {
                put(s, " alt2: %.2fm ", g.alt2);
                put(s, " vH2: %.2fm/s  D2: %.1f°  vV2: %.2fm/s ", g.vH2, g.vD2, g.vV2);
                put(s, " sats2: %2d ", g.sats2);
            }
            s += "  ";
            put(s, " P=%.2fhPa ", g.P);
            put(s, " T=%.2f°C ", g.T);
            put(s, " H1=%.2f%% ", g.U1);
            put(s, " H2=%.2f%% ", g.U2);
            s += " ";
            put(s, " (%09d) ", (int)g.id);
            if (o.vbs == 2) {
                s += " ";
                put(s, " Ti=%.2f°C ", g.iT);
                put(s, " Bat=%.2fV ", g.bat);
            }
            s += "  # chk: ";
            for (int i = 0; i < 7; i++) put(s, "%d", (err_rd41 >> i) & 1);
            s += "\n";
        }

        const bool frm_ok = g.type == RD41 ? (err_rd41 & 0x7F) == 0 : (err_rd94 & 0x1F) == 0;
        if (o.json && frm_ok) {
            put(s, "{ \"type\": \"%s\"", g.type == RD94 ? "RD94" : "RD41");
            put(s, ", \"frame\": %d, \"id\": \"%09d\"", g.frnr, (int)g.id);
            if (g.type == RD94) put(s, ", \"datetime\": \"%04d-%02d-%02dT%02d:%02d:%02d.%03dZ\"", g.jahr, g.monat, g.tag, g.std, g.min, g.sek, g.ms);
            else put(s, ", \"datetime\": \"%02d:%02d:%02d.%02dZ\"", g.std, g.min, g.sek, g.cs);
            put(s, ", \"lat\": %.5f, \"lon\": %.5f, \"alt\": %.5f, \"vel_h\": %.5f, \"heading\": %.5f, \"vel_v\": %.5f, \"sats\": %d", g.lat, g.lon, g.alt,
                g.vH, g.vD, g.vV, g.sats);
            if (g.T > -273.0) put(s, ", \"temp\": %.1f", g.T);
            if (g.U1 > -0.5) put(s, ", \"humidity\": %.1f", g.U1);
            if (g.P > 0.0) put(s, ", \"pressure\": %.2f", g.P);
            if (o.jsn_freq_khz > 0) put(s, ", \"freq\": %d", o.jsn_freq_khz);
            put(s, ", \"ref_datetime\": \"%s\"", g.type == RD94 ? "GPS" : "UTC");
            put(s, ", \"ref_position\": \"%s\"", g.type == RD94 ? "GPS" : "MSL");
            if (o.version[0]) put(s, ", \"version\": \"%s\"", o.version);
            s += " }\n";
            s += "\n";
            p->last_json = 1;
        }
    }
    if (s.size() + 1 > outlen) return SONDE_E_RANGE;
    memcpy(out, s.data(), s.size());
    out[s.size()] = 0;
    return (int)s.size();
}

// ------------------------------------------------------------------ print_bitframe's way from raw bits to bytes (:332-374, :1253-1259)
extern "C" int sonde_drop_frame_from_rawbits(const uint8_t *rawbits, int32_t nraw, sonde_drop_frame_t *f) {
    if (!rawbits || !f || nraw < 0 || nraw > RAWBITS) return SONDE_E_ARG;
    for (int j = 0; j < FRAME_LEN; j++) {
        int v = 0;
        for (int i = 1; i < BITS - 1; i++) {
            const int p = 2 * (BITS * j + i);
            const int b0 = p < nraw ? rawbits[p] : 0, b1 = p + 1 < nraw ? rawbits[p + 1] : 0;
            if (b0 == 0 && b1 == 1) v |= 1 << (i - 1);                          // manchester2: 01 -> 1; 10 -> 0; the rest 'x' = 0
        }
        f->bytes[j] = (uint8_t)v;
    }
    f->nraw = nraw;
    f->err94 = (int32_t)geterr_rd94(f->bytes);
    f->err41 = (int32_t)geterr_rd41(f->bytes);
    return 0;
}

// ------------------------------------------------------------------ --softin / --softinv (main :1357-1386)
struct sonde_drop_softin {
    int inv = 0, found = 0, pos = HEADLEN;
    uint64_t hist = 0, valid = 0, hdr = 0, count = 0, t_hdr = 0;     // buf[40] as values and "holds a bit" masks (it starts as "x" and NULs)
    uint8_t frame[RAWBITS];
    std::deque<sonde_drop_frame_t> done;
};

extern "C" int sonde_drop_softin_create(int32_t invert, sonde_drop_softin_t **out) {
    if (!out) return SONDE_E_ARG;
    auto *s = new (std::nothrow) sonde_drop_softin();
    if (!s) return SONDE_E_NOMEM;
    s->inv = invert ? 1 : 0;
    for (int i = 0; i < HEADLEN; i++) { s->hdr = (s->hdr << 1) | (uint64_t)(HDR40[i] == '1'); s->frame[i] = (uint8_t)(HDR40[i] == '1'); }
    *out = s;
    return 0;
}

extern "C" void sonde_drop_softin_destroy(sonde_drop_softin_t *s) { delete s; }

extern "C" int sonde_drop_softin_push(sonde_drop_softin_t *s, const float *soft, int32_t n, sonde_drop_frame_t *out, int32_t max) {
    if (!s || (!soft && n > 0) || n < 0 || (!out && max > 0) || max < 0) return SONDE_E_ARG;
    const uint64_t mask = (1ULL << HEADLEN) - 1;
    for (int i = 0; i < n; i++) {
        const int bit = s->inv ? (soft[i] <= 0.0f) : (soft[i] >= 0.0f);
        s->count++;
        s->hist = ((s->hist << 1) | (uint64_t)bit) & mask;
        s->valid = ((s->valid << 1) | 1) & mask;
        if (!s->found) {
            if (s->valid == mask && s->hist == s->hdr) { s->found = 1; s->t_hdr = s->count; }
        } else {
            s->frame[s->pos++] = (uint8_t)bit;
            if (s->pos == RAWBITS) {
                sonde_drop_frame_t f;
                memset(&f, 0, sizeof f);
                sonde_drop_frame_from_rawbits(s->frame, RAWBITS, &f);
                f.complete = 1; f.sample = s->t_hdr;
                s->done.push_back(f);
                s->found = 0; s->pos = HEADLEN;
            }
        }
    }
    int k = 0;
    while (k < max && !s->done.empty()) { out[k++] = s->done.front(); s->done.pop_front(); }
    return k;
}
