// softin_mrz_replay.cpp — test infrastructure: a stand-alone program around emu_mrz_run (softin_mrz_emu.cpp) for sanitizer builds of the emulated MRZ wave
// function, outside any interpreter:
//   softin_mrz_replay <float32 symbol file> <invert> <inv> <auto> <raw2> <bits_ofs> <cap> <call length> [<call length> ..]
//       -> the `mp3h1mod -r` (raw2: `-R`) line of every frame on stdout
// The last call length repeats until the stream is consumed.  Frames, dropped frames and the end state go to stderr.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct SoftinMrzRec { int32_t channel; float mv; unsigned long long hdr_bit; int32_t nbits; uint8_t inv, crc_ok, crclen, pad; uint16_t crcval, crcdat; uint8_t bits[52]; };
struct EmuMrzState { int mode, done, inv, bitfrm_len; float mv, carry; unsigned long long bits_in, hdr_bit; float hist[44]; uint32_t w[13]; int pad; };
extern "C" int emu_mrz_run(const float *soft, int n, const int *calls, int n_calls, int invert, int inv, int aut, int raw2, int bits_ofs, int cap, SoftinMrzRec *recs,
                           int max_recs, int *n_dropped, EmuMrzState *end);

int main(int argc, char **argv) {
    if (argc < 9) { fprintf(stderr, "usage: %s symbols.f32 invert inv auto raw2 bits_ofs cap call [call ..]\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<float> s;
    float buf[4096]; size_t n;
    while ((n = fread(buf, sizeof(float), 4096, f)) > 0) s.insert(s.end(), buf, buf + n);
    fclose(f);
    std::vector<int> calls;
    for (int i = 8; i < argc; i++) calls.push_back(atoi(argv[i]));
    const int raw2 = atoi(argv[5]), ofs = atoi(argv[6]);
    std::vector<SoftinMrzRec> recs(s.size() / 700 + 2);
    int dropped = 0; EmuMrzState end{};
    const int got = emu_mrz_run(s.data(), (int)s.size(), calls.data(), (int)calls.size(), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), raw2, ofs, atoi(argv[7]), recs.data(),
                                (int)recs.size(), &dropped, &end);
    if (got < 0) { fprintf(stderr, "emu_mrz_run: %d\n", got); return 1; }
    for (int i = 0; i < got && i < (int)recs.size(); i++) {
        const SoftinMrzRec &r = recs[i];
        auto bit = [&](int p) { return (r.bits[p >> 3] >> (7 - (p & 7))) & 1; };
        if (raw2) { for (int j = 0; j < r.nbits; j++) putchar('0' + bit(j)); putchar('\n'); continue; }
        const int frmlen = (r.nbits - ofs) / 8;
        for (int k = 0; k < frmlen; k++) {
            unsigned v = 0;
            for (int j = 0; j < 8; j++) v = v << 1 | (unsigned)bit(ofs + 8 * k + j);
            printf("%02X ", v);
        }
        printf(" %s\n", r.crc_ok ? "[OK]" : "[NO]");
    }
    fprintf(stderr, "%d frames, %d dropped, mode %d done %d inv %d len %d bits_in %llu\n", got, dropped, end.mode, end.done, end.inv, end.bitfrm_len, end.bits_in);
    return 0;
}
