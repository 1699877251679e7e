// softin_meisei_replay.cpp — test infrastructure: a stand-alone program around emu_meisei_run (softin_meisei_emu.cpp) for sanitizer builds of the emulated Meisei
// wave function, outside any interpreter:
//   softin_meisei_replay <float32 symbol file> <invert> <ecc> <cap> <call length> [<call length> ..]     -> the `meisei100mod -r [--ecc -v]` line of every frame on stdout
// The last call length repeats until the stream is consumed.  Frames, dropped frames and the end state go to stderr.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct SoftinMeiseiRec { int32_t channel; float mv; unsigned long long hdr_bit; uint8_t block_err[12]; uint8_t bits[75]; uint8_t pad[1]; };
struct EmuMeiseiState { int mode, done; float mv, carry; unsigned long long bits_in, hdr_bit; float hist[48]; uint32_t w[19]; int pad; };
extern "C" int emu_meisei_run(const float *soft, int n, const int *calls, int n_calls, int invert, int ecc, int cap, SoftinMeiseiRec *recs, int max_recs, int *n_dropped,
                              EmuMeiseiState *end);

static unsigned val(const uint8_t *bits, int at, int len) {
    unsigned v = 0;
    for (int j = 0; j < len; j++) v = v << 1 | ((bits[(at + j) >> 3] >> (7 - ((at + j) & 7))) & 1u);
    return v;
}

int main(int argc, char **argv) {
    if (argc < 6) { fprintf(stderr, "usage: %s symbols.f32 invert ecc cap call [call ..]\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<float> s;
    float buf[4096]; size_t n;
    while ((n = fread(buf, sizeof(float), 4096, f)) > 0) s.insert(s.end(), buf, buf + n);
    fclose(f);
    std::vector<int> calls;
    for (int i = 5; i < argc; i++) calls.push_back(atoi(argv[i]));
    const int ecc = atoi(argv[3]);
    std::vector<SoftinMeiseiRec> recs(s.size() / 1152 + 2);
    int dropped = 0; EmuMeiseiState end{};
    const int got = emu_meisei_run(s.data(), (int)s.size(), calls.data(), (int)calls.size(), atoi(argv[2]), ecc, atoi(argv[4]), recs.data(), (int)recs.size(), &dropped, &end);
    if (got < 0) { fprintf(stderr, "emu_meisei_run: %d\n", got); return 1; }
    for (int i = 0; i < got && i < (int)recs.size(); i++) {
        const SoftinMeiseiRec &r = recs[i];
        for (int sf = 0; sf < 2; sf++) {
            printf("%06X ", val(r.bits, 300 * sf, 24));
            for (int j = 0; j < 6; j++) printf("%04X %04X ", val(r.bits, 300 * sf + 24 + 46 * j, 16), val(r.bits, 300 * sf + 24 + 46 * j + 17, 16));
            if (ecc) { printf("#"); for (int b = 0; b < 6; b++) printf("%X", r.block_err[6 * sf + b]); printf("#  "); }
        }
        printf("\n");
    }
    fprintf(stderr, "%d frames, %d dropped, mode %d done %d bits_in %llu\n", got, dropped, end.mode, end.done, end.bits_in);
    return 0;
}
