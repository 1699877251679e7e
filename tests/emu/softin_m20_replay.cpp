// softin_m20_replay.cpp — test infrastructure: a stand-alone program around emu_m20_run (softin_m20_emu.cpp) for sanitizer builds of the emulated M20 wave function
// and the host entry points behind its records (sonde_m20_rawline), outside any interpreter:
//   softin_m20_replay <float32 symbol file> <skip> <invert> <cap> <call length> [<call length> ..]     -> the `m20mod -r -v` line of every frame on stdout
// The last call length repeats until the stream is consumed.  Frames, dropped frames and the end state go to stderr.
#include "../../include/sonde_hip.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

struct EmuM20State { int mode, inv, mpos, mhalf, mbit0, mskip; float ms1, mv; unsigned long long bits_in, hdr_bit; };
extern "C" int emu_m20_run(const float *soft, int n, const int *calls, int n_calls, int invert, int doskip, int cap, sonde_m20_frame_t *recs, int max_recs, int *n_dropped,
                           EmuM20State *end);

int main(int argc, char **argv) {
    if (argc < 6) { fprintf(stderr, "usage: %s symbols.f32 skip invert cap call [call ..]\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<float> s;
    float buf[4096]; size_t n;
    while ((n = fread(buf, sizeof(float), 4096, f)) > 0) s.insert(s.end(), buf, buf + n);
    fclose(f);
    std::vector<int> calls;
    for (int i = 5; i < argc; i++) calls.push_back(atoi(argv[i]));
    std::vector<sonde_m20_frame_t> recs(s.size() / 2672 + 2);
    int dropped = 0; EmuM20State end{};
    const int got = emu_m20_run(s.data(), (int)s.size(), calls.data(), (int)calls.size(), atoi(argv[3]), atoi(argv[2]), atoi(argv[4]), recs.data(), (int)recs.size(), &dropped, &end);
    if (got < 0) { fprintf(stderr, "emu_m20_run: %d\n", got); return 1; }
    char line[400];
    for (int i = 0; i < got && i < (int)recs.size(); i++) {
        if (sonde_m20_rawline(&recs[i], 1, line, sizeof line) < 0) { fprintf(stderr, "sonde_m20_rawline failed on frame %d\n", i); return 1; }
        printf("%s\n", line);
    }
    fprintf(stderr, "%d frames, %d dropped, mode %d mpos %d mskip %d bits_in %llu\n", got, dropped, end.mode, end.mpos, end.mskip, end.bits_in);
    return 0;
}
