// fm_front_emu.cpp — test infrastructure: the device front end of the FM slicers (csrc/sonde_fm_front_dev.h: iq_dec's IQ-dc removal, table mixer,
// discriminator and FM low-pass at decM = 1 on float32 IQ) compiled for the CPU under wave_emu.h, driven the way the engine drives k_fm_front: one wave per call,
// the channel's record and its unfiltered ring in memory between the calls, LDS that does not survive a launch.  The design (mixer frequency, table period,
// taps) is the product's own: csrc/sonde_design.cpp is compiled into this file.
//   emu_fm_front_run(iq, n, calls, n_calls, fq, sr, out)
//       n float32 IQ samples through one channel created at --iq fq, in calls of calls[0], calls[1], .. samples (the last length repeats until the stream is
//       consumed); the FM stream through iq_dec's 16-bit conversion (fwrite_fm_blk, --bo 16) -> out[n].  Returns the tap count, or a negative number.
//   emu_fm_front_lds_bytes()
#include "wave_emu.h"
#include "../../radiosonde_auto_rx_amd/csrc/sonde_fm_front_dev.h"
#include "../../radiosonde_auto_rx_amd/csrc/sonde_design.cpp"
#include <algorithm>
#include <cstring>
#include <vector>

extern "C" int emu_fm_front_run(const float *iq, int n, const int *calls, int n_calls, double fq, int sr, int16_t *out) {
    if (!iq || n < 0 || !calls || n_calls < 1 || !out || sr < 32 || !(fq >= -0.5 && fq <= 0.5)) return -1;
    int longest = 64;
    for (int i = 0; i < n_calls; i++) { if (calls[i] < 1) return -1; longest = std::max(longest, calls[i]); }
    if (sonde::design_decimator_if(sr, 48000, false).decM != 1) return -1;
    int taps = (int)(4 * sr / 2e3); if (taps % 2 == 0) taps++;                                // iq_dec.c: --lpFM
    const std::vector<float> w = sonde::design_lowpass(6e3f / (float)sr, taps), ws2 = sonde::dup_taps(w);
    taps = (int)w.size();
    int ring = 1, rring = 1;
    while (ring < longest) ring <<= 1;
    while (rring < taps + 128) rring <<= 1;
    if (taps > FMF_TAPS_MAX || rring > FMF_RING_MAX) return -1;
    FmFrontChan st;                                                                          // as FmSliceEngine::fresh_front builds it
    memset(&st, 0, sizeof st);
    st.maxlim = (uint32_t)sr; st.maxcnt = st.maxlim / 32;
    const sonde::Mixer m = sonde::design_mixer(-fq, sr);
    st.f0 = m.f0; st.lut_len = (uint32_t)m.lut_len;
    std::vector<float> fm((size_t)ring, 0.f), raw((size_t)rring, 0.f);
    std::vector<FmFrontLds> lds(1);
    uint64_t m_done = 0;
    int k = 0;
    for (int at = 0; at < n; k++) {
        const int want = calls[k < n_calls ? k : n_calls - 1], nb = n - at < want ? n - at : want;
        std::vector<FmfIQ> call((size_t)nb);                                                 // a buffer of exactly the call's length: a read beyond it is the sanitizer's to find
        memcpy((void *)call.data(), iq + 2 * (size_t)at, (size_t)nb * sizeof(FmfIQ));
        memset((void *)lds.data(), 0xA5, sizeof(FmFrontLds));
        const uint32_t first = (uint32_t)(m_done & (uint64_t)(ring - 1));
        emu::run_workgroup(64, [&](int tid) {
            fm_front_channel(&st, call.data(), nb, fm.data(), first, (uint32_t)ring - 1, raw.data(), rring, ws2.data(), taps, lds.data(), tid);
        });
        for (int i = 0; i < nb; i++) {
            float x = fm[(size_t)((first + (uint32_t)i) & (uint32_t)(ring - 1))] * 128.0f;
            x *= 256.0f;
            out[at + i] = (int16_t)(int)x;
        }
        m_done += (uint64_t)nb;
        at += nb;
    }
    return taps;
}

extern "C" int emu_fm_front_lds_bytes() { return (int)sizeof(FmFrontLds); }
