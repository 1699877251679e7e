// sonde_host.h — internal host-side declarations of libsonde_hip (design math, RS41 framing/ECC).
#ifndef SONDE_HOST_H
#define SONDE_HOST_H
#include <complex>
#include <cstdint>
#include <string>
#include <vector>

struct sonde_engine;

namespace sonde {

struct Decimator { int if_sr = 0, decM = 1; std::vector<float> taps; };

std::vector<float> design_lowpass(float f, int taps);
std::vector<float> dup_taps(const std::vector<float> &w);
Decimator design_decimator(int sr_base, bool if_min);
Decimator design_decimator_scan(int sr_base, bool if_min, float set_lpIQ);
Decimator design_decimator_if(int sr_base, int if_target, bool narrow);
struct Imet4Design { int if_sr = 0, decM = 1; std::vector<float> lp_iq0, lp_iq1, lp_fm, lp_dec; };
Imet4Design design_imet4(int sr_base, bool iq, bool if_min, bool imet1, float lpiq_bw);
// mk2a1680mod's L-band design (init_buffers_Lband and the option handling of its main)
struct Mk2aDesign {
    int if_sr = 0, decM = 1, decFM = 1, fmdec = 0, lp = 0;        // lp: 1 IF low-pass, 2 FM low-pass, 4 IQFM low-pass
    float sps = 0, bl = -1, tone_sps = 0, h = 10.4f;
    int L = 0, M = 0, K = 0, N = 0, delay = 0, bitofs = 0, mp_ofs = 0;
    std::vector<float> lp_dec, lp_iq0, lp_iq1, lp_fm, lp_iqfm, match;
    std::vector<int> tone_n;                                       // sample lags of the --IQ tone correlator, in the reference's order
    double f1 = 0;                                                 // its lower tone (Hz); the upper one is -f1
};
Mk2aDesign design_mk2a(int sr_base, int opt_iq, bool lp_iq, float lpiq_bw, bool lp_fm, int opt_decFM, bool dc, bool if_min, float baud, int shift);
int engine_fm_tap_device(sonde_engine *e, const float **base, int *ring_len);
struct Mixer { double f0 = 0; int lut_len = 1; };
Mixer design_mixer(double xlt_fq, int sr_base);
std::vector<float> design_match(const std::string &hdr, float sps, float bt);
void bit_window(int pos, int half, int symlen, float sps, uint32_t &q0, uint32_t &q1, double &mid);
void slice_range(uint32_t q0, uint32_t q1, double mid, float l, uint32_t &qa, uint32_t &qb);

// GF(2^8)/0x11D, alpha = 2
const uint8_t *gf_exp_table();   // 512 entries
const uint8_t *gf_log_table();   // 256 entries
int  rs255_syndromes(const uint8_t cw[255], uint8_t S[24]);     // returns 1 if any non-zero
int  rs255_decode_syn(uint8_t cw[255], const uint8_t S[24]);    // errors-only, Euclid; <0 on failure
int  rs255_decode(uint8_t cw[255]);
void rs255_encode(uint8_t cw[255]);
int  crc16(const uint8_t *p, int len);

// the reference's 8192-point transform (dft_raw with its float twiddle recurrence; sonde_scan.cpp): in place on 8192 (re, im) pairs,
// and the stage twiddle table the device kernels use (stage t at 2^t - 1 + j, (re, im) pairs)
void ref_dft_8192(std::vector<float> &re_im);
std::vector<float> ref_twiddle_table();

extern const char    kRs41Header[65];
extern const uint8_t kRs41HeaderBytes[8];
extern const uint8_t kRs41Mask[64];
int  rs41_frametype(const uint8_t *frame);
// rs41_ecc() of the reference for ecc levels 1/2; synd = device syndromes of the first pass or nullptr
int  rs41_ecc(uint8_t frame[518], int frmlen, int level, const uint8_t *synd);

extern const char kDfmRawHeader[33];
extern const char kM10RawHeader[33];
int  m10_checksum(const uint8_t *msg, int len);          // checkM10 (m10mod.c:594-628)
int  dfm_block(int level, const uint8_t *hb, const float *sb, int L, uint8_t *nib);

}  // namespace sonde
#endif
