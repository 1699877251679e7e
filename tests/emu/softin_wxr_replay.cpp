// softin_wxr_replay.cpp — test infrastructure: a stand-alone program around emu_wxr_run (softin_wxr_emu.cpp) for sanitizer builds of the emulated WxR-301D wave
// function, outside any interpreter:
//   softin_wxr_replay <float32 soft-bit file> <invert_stream> <invert> <pn9> <cap> <call length> [<call length> ..]  -> the `weathex301d -r -v` line of every frame
// The last call length repeats until the stream is consumed.  Frames, dropped frames and the end state go to stderr.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct SoftinWxrRec { int32_t channel, pad; unsigned long long hdr_bit; uint8_t raw[69], x[69], pad2[2]; uint32_t chkval, chkdat; uint8_t chk_ok, frid, pad3[2]; uint32_t sn, cnt; };
struct EmuWxrState { int mode, pos; unsigned long long hist, valid, bits_in, hdr_bit; uint32_t w[18]; };
extern "C" int emu_wxr_run(const float *soft, int n, const int *calls, int n_calls, int invert_stream, int invert, int pn9, int cap, SoftinWxrRec *recs, int max_recs,
                           int *n_dropped, EmuWxrState *end);

int main(int argc, char **argv) {
    if (argc < 7) { fprintf(stderr, "usage: %s soft.f32 invert_stream invert pn9 cap call [call ..]\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<float> s;
    float buf[4096]; size_t n;
    while ((n = fread(buf, sizeof(float), 4096, f)) > 0) s.insert(s.end(), buf, buf + n);
    fclose(f);
    std::vector<int> calls;
    for (int i = 6; i < argc; i++) calls.push_back(atoi(argv[i]));
    std::vector<SoftinWxrRec> recs(s.size() / 552 + 2);
    int dropped = 0; EmuWxrState end{};
    const int got = emu_wxr_run(s.data(), (int)s.size(), calls.data(), (int)calls.size(), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), recs.data(),
                                (int)recs.size(), &dropped, &end);
    if (got < 0) { fprintf(stderr, "emu_wxr_run: %d\n", got); return 1; }
    for (int i = 0; i < got && i < (int)recs.size(); i++) {
        const SoftinWxrRec &r = recs[i];
        for (int k = 0; k < 69; k++) printf("%02X ", r.x[k]);
        printf(" #  %s # [%04X:%04X]\n", r.chk_ok ? "[OK]" : "[NO]", (unsigned)r.chkdat, (unsigned)r.chkval);
    }
    fprintf(stderr, "%d frames, %d dropped, mode %d pos %d bits_in %llu\n", got, dropped, end.mode, end.pos, end.bits_in);
    return 0;
}
