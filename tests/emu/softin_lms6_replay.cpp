// softin_lms6_replay.cpp — test infrastructure: a stand-alone program around emu_lms6_run_rec (softin_lms6_emu.cpp) for sanitizer builds of the host code of the LMS6
// consumer (sonde_lms6_dec_block_bytes and the emulated wave function), outside any interpreter:
//   softin_lms6_replay <float32 soft-bit file> <soft bits per call> <vit> <typ> <ecc> <raw> <json> <invert>     -> the text of all blocks on stdout
// The record buffer holds 8 blocks per launch: a call that completes more takes the kernel's dropped-record path (decoded into the tail of the wave's LDS), and
// the count of those goes to stderr.
#include "../../include/sonde_lms6.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" int emu_lms6_run_rec(const float *soft, int n, int call, int invert, const sonde_lms6_opts_t *opts, int cap, char *out, size_t outlen, int *n_blocks, int *n_launches,
                                void *recs, int max_recs, int *n_dropped);

int main(int argc, char **argv) {
    if (argc != 9) { fprintf(stderr, "usage: %s soft.f32 call vit typ ecc raw json invert\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<float> s;
    float buf[4096]; size_t n;
    while ((n = fread(buf, sizeof(float), 4096, f)) > 0) s.insert(s.end(), buf, buf + n);
    fclose(f);
    sonde_lms6_opts_t o; memset(&o, 0, sizeof o);
    o.vit = atoi(argv[3]); o.typ = atoi(argv[4]); o.ecc = atoi(argv[5]); o.raw = atoi(argv[6]); o.json = atoi(argv[7]);
    std::vector<char> out(1 << 18);
    int blocks = 0, launches = 0, dropped = 0;
    const int rc = emu_lms6_run_rec(s.data(), (int)s.size(), atoi(argv[2]), atoi(argv[8]), &o, 8, out.data(), out.size(), &blocks, &launches, nullptr, 0, &dropped);
    if (rc < 0) { fprintf(stderr, "emu_lms6_run_rec: %d\n", rc); return 1; }
    fwrite(out.data(), 1, (size_t)rc, stdout);
    fprintf(stderr, "%d blocks, %d launches, %d dropped\n", blocks, launches, dropped);
    return 0;
}
