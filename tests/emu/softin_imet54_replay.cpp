// softin_imet54_replay.cpp — test infrastructure: a stand-alone program around emu_imet54_run (softin_imet54_emu.cpp) for sanitizer builds of the emulated iMet-54
// wave function, outside any interpreter:
//   softin_imet54_replay <float32 symbol file> <invert> <inv> <aut> <ecc> <cap> <call length> [<call length> ..]     -> the `imet54mod -r [--ecc]` line of every frame on stdout
// The last call length repeats until the stream is consumed.  Frames, dropped frames and the end state go to stderr.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct SoftinImet54Rec { int32_t channel; float mv; unsigned long long hdr_bit; int32_t inv, ecc_frm, ecc_tlm, ecc_std, crc_std, crc_cont; uint8_t frame[108]; uint8_t pad[4]; };
struct EmuImet54State { int mode, inv, done, carry_n; float mv; int pad; unsigned long long bits_in, hdr_bit; float carry[10]; float hist[40]; };
extern "C" int emu_imet54_run(const float *soft, int n, const int *calls, int n_calls, int invert, int inv, int aut, int ecc, int cap, SoftinImet54Rec *recs, int max_recs,
                              int *n_dropped, EmuImet54State *end);

int main(int argc, char **argv) {
    if (argc < 8) { fprintf(stderr, "usage: %s symbols.f32 invert inv aut ecc cap call [call ..]\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<float> s;
    float buf[4096]; size_t n;
    while ((n = fread(buf, sizeof(float), 4096, f)) > 0) s.insert(s.end(), buf, buf + n);
    fclose(f);
    std::vector<int> calls;
    for (int i = 7; i < argc; i++) calls.push_back(atoi(argv[i]));
    const int ecc = atoi(argv[5]);
    std::vector<SoftinImet54Rec> recs(s.size() / 2200 + 2);
    int dropped = 0; EmuImet54State end{};
    const int got = emu_imet54_run(s.data(), (int)s.size(), calls.data(), (int)calls.size(), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), ecc, atoi(argv[6]), recs.data(),
                                   (int)recs.size(), &dropped, &end);
    if (got < 0) { fprintf(stderr, "emu_imet54_run: %d\n", got); return 1; }
    for (int i = 0; i < got && i < (int)recs.size(); i++) {
        const SoftinImet54Rec &r = recs[i];
        for (int k = 0; k < 108; k++) printf("%02X", r.frame[k]);
        printf(" %s", r.crc_std ? "[OK]" : r.crc_cont ? "[ok]" : r.ecc_std == 0 ? "[oo]" : r.frame[0x52] == 0xF8 ? "[NO]" : "[no]");
        if (ecc && r.ecc_frm != 0) printf(" # (%d) [%d]", r.ecc_frm, r.ecc_tlm);
        printf("\n");
    }
    fprintf(stderr, "%d frames, %d dropped, mode %d inv %d done %d carry %d bits_in %llu\n", got, dropped, end.mode, end.inv, end.done, end.carry_n, end.bits_in);
    return 0;
}
