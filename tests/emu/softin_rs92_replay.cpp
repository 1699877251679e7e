// softin_rs92_replay.cpp — test infrastructure: a stand-alone program around emu_rs92_run (softin_rs92_emu.cpp) for sanitizer builds of the emulated RS92 wave function,
// outside any interpreter:
//   softin_rs92_replay <float32 symbol file> <invert> <inv> <cap> <call length> [<call length> ..]     -> the `rs92mod -r -v` line of every frame on stdout
// The last call length repeats until the stream is consumed.  Frames, dropped frames and the end state go to stderr.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct SoftinRs92Rec { int32_t channel, ec; float mv; int32_t pad; unsigned long long hdr_bit; uint8_t frame[240]; };
struct EmuRs92State { int mode, done, carry_n; float mv; unsigned long long bits_in, hdr_bit; float carry[20]; float hist[60]; };
extern "C" int emu_rs92_run(const float *soft, int n, const int *calls, int n_calls, int invert, int inv, int cap, SoftinRs92Rec *recs, int max_recs, int *n_dropped,
                            EmuRs92State *end);

int main(int argc, char **argv) {
    if (argc < 6) { fprintf(stderr, "usage: %s symbols.f32 invert inv cap call [call ..]\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<float> s;
    float buf[4096]; size_t n;
    while ((n = fread(buf, sizeof(float), 4096, f)) > 0) s.insert(s.end(), buf, buf + n);
    fclose(f);
    std::vector<int> calls;
    for (int i = 5; i < argc; i++) calls.push_back(atoi(argv[i]));
    std::vector<SoftinRs92Rec> recs(s.size() / 4680 + 2);
    int dropped = 0; EmuRs92State end{};
    const int got = emu_rs92_run(s.data(), (int)s.size(), calls.data(), (int)calls.size(), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), recs.data(), (int)recs.size(), &dropped, &end);
    if (got < 0) { fprintf(stderr, "emu_rs92_run: %d\n", got); return 1; }
    for (int i = 0; i < got && i < (int)recs.size(); i++) {
        const SoftinRs92Rec &r = recs[i];
        for (int k = 0; k < 240; k++) printf("%02x", r.frame[k]);
        printf(" %s", r.ec >= 0 ? " [OK]" : " [NO]");
        if (r.ec > 0) printf(" (%d)", r.ec);
        if (r.ec < 0) printf(" (-)");
        printf("\n");
    }
    fprintf(stderr, "%d frames, %d dropped, mode %d done %d carry %d bits_in %llu\n", got, dropped, end.mode, end.done, end.carry_n, end.bits_in);
    return 0;
}
