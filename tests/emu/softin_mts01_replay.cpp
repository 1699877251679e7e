// softin_mts01_replay.cpp — test infrastructure: a stand-alone program around emu_mts01_run (softin_mts01_emu.cpp) for sanitizer builds of the emulated MTS01 wave
// function, outside any interpreter:
//   softin_mts01_replay <float32 symbol file> <invert> <cap> <call length> [<call length> ..]     -> the `mts01mod -r` line of every frame on stdout
// The last call length repeats until the stream is consumed.  Frames, dropped frames and the end state go to stderr.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct SoftinMts01Rec { int32_t channel; float mv; unsigned long long hdr_bit; uint16_t crcval, crcdat; uint8_t crc_ok; uint8_t bytes[131]; };
struct EmuMts01State { int mode, done; float mv; int pad; unsigned long long bits_in, hdr_bit; float hist[32]; uint32_t w[33]; int pad2; };
extern "C" int emu_mts01_run(const float *soft, int n, const int *calls, int n_calls, int invert, int cap, SoftinMts01Rec *recs, int max_recs, int *n_dropped,
                             EmuMts01State *end);

int main(int argc, char **argv) {
    if (argc < 5) { fprintf(stderr, "usage: %s symbols.f32 invert cap call [call ..]\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<float> s;
    float buf[4096]; size_t n;
    while ((n = fread(buf, sizeof(float), 4096, f)) > 0) s.insert(s.end(), buf, buf + n);
    fclose(f);
    std::vector<int> calls;
    for (int i = 4; i < argc; i++) calls.push_back(atoi(argv[i]));
    std::vector<SoftinMts01Rec> recs(s.size() / 1048 + 2);
    int dropped = 0; EmuMts01State end{};
    const int got = emu_mts01_run(s.data(), (int)s.size(), calls.data(), (int)calls.size(), atoi(argv[2]), atoi(argv[3]), recs.data(), (int)recs.size(), &dropped, &end);
    if (got < 0) { fprintf(stderr, "emu_mts01_run: %d\n", got); return 1; }
    for (int i = 0; i < got && i < (int)recs.size(); i++) {
        const SoftinMts01Rec &r = recs[i];
        for (int k = 0; k < 131; k++) printf("%02X ", r.bytes[k]);
        printf(" # [%04X:%04X] # [%s]\n", (unsigned)r.crcdat, (unsigned)r.crcval, r.crc_ok ? "OK" : "NO");
    }
    fprintf(stderr, "%d frames, %d dropped, mode %d done %d bits_in %llu\n", got, dropped, end.mode, end.done, end.bits_in);
    return 0;
}
