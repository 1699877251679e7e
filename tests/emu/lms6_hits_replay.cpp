// lms6_hits_replay.cpp — test infrastructure: a stand-alone program around emu_lms6_hits_run (lms6_hits_emu.cpp) for sanitizer builds of the emulated per-hit
// LMS6 / LMS-X decoder, outside any interpreter:
//   lms6_hits_replay <float32 file: n hits of `nb` soft bits> <vit> <nb> <grid> <max_frames> <start> <nbits mv> [<nbits mv> ..]
// One `nbits mv` pair per ring slot (max_frames of them; the file holds the hits by slot, nb = 4096 or 4720 values each); the records of the counter values
// [start, start + max_frames) go to stdout, one line each in slot order: channel kind nbits decoded len blen err vit bytes (hex).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/sonde_hip.h"

extern "C" int emu_lms6_hits_run(int vit, int nb, const float *soft, long long stride, const int *nbits, const float *mv, int max_frames, unsigned start, unsigned end,
                                 int grid, sonde_lms6_hit_t *out, unsigned *done);

int main(int argc, char **argv) {
    if (argc < 9 || (argc - 7) % 2) { fprintf(stderr, "usage: %s hits.f32 vit nb grid max_frames start nbits mv [nbits mv ..]\n", argv[0]); return 2; }
    const int vit = atoi(argv[2]), nb = atoi(argv[3]), grid = atoi(argv[4]), max_frames = atoi(argv[5]);
    const unsigned start = (unsigned)strtoul(argv[6], nullptr, 10);
    if (max_frames != (argc - 7) / 2 || nb < 1) { fprintf(stderr, "one nbits mv pair per slot\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<float> s((size_t)max_frames * (size_t)nb);                 // exactly what the kernel may index: a read beyond it is the sanitizer's to report
    const size_t got = fread(s.data(), sizeof(float), s.size(), f);
    fclose(f);
    if (got != s.size()) { fprintf(stderr, "%s: %zu of %zu soft bits\n", argv[1], got, s.size()); return 2; }
    std::vector<int> nbits((size_t)max_frames); std::vector<float> mv((size_t)max_frames);
    for (int i = 0; i < max_frames; i++) { nbits[(size_t)i] = atoi(argv[7 + 2 * i]); mv[(size_t)i] = (float)atof(argv[8 + 2 * i]); }
    std::vector<sonde_lms6_hit_t> out((size_t)max_frames);
    memset((void *)out.data(), 0xEE, out.size() * sizeof(sonde_lms6_hit_t));
    unsigned done[2] = { start, 0u };
    const int rc = emu_lms6_hits_run(vit, nb, s.data(), nb, nbits.data(), mv.data(), max_frames, start, start + (unsigned)max_frames, grid, out.data(), done);
    if (rc < 0) { fprintf(stderr, "emu_lms6_hits_run: %d\n", rc); return 1; }
    for (const sonde_lms6_hit_t &r : out) {
        printf("%d %d %d %d %d %d %d %d ", r.channel, r.kind, r.nbits, r.decoded, r.len, r.blen, r.err, r.vit);
        for (int k = 0; k < 308; k++) printf("%02x", r.bytes[k]);
        printf("\n");
    }
    fprintf(stderr, "%d records, done %u ticket %u\n", max_frames, done[0], done[1]);
    return 0;
}
