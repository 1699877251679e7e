// m20_hits_replay.cpp — test infrastructure: a stand-alone program around emu_m20_hits_run (m20_hits_emu.cpp) for sanitizer builds of the emulated per-hit M20
// decoder, outside any interpreter:
//   m20_hits_replay <file: n hits of 165 bytes, hard bits 8 a byte, LSB first> <grid> <n_channels> <nbits channel mv> [<nbits channel mv> ..]
// One `nbits channel mv` triple per hit, in the order of the file (one launch, a ring of n slots).  The records go to stdout, one line each:
// channel nbits len cs_ok cs_calc blk_ok fw mv_pos mv(bits, hex) frame (hex), then one line per channel with its characters (hex).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/sonde_hip.h"

extern "C" int emu_m20_hits_run(const uint8_t *bits, const int *nbits, const int *channel, const float *mv, int n_channels, int max_frames, unsigned end, int grid,
                                char *chars, sonde_m20_frame_t *out, unsigned *done);
extern "C" int emu_m20_chan_chars();

int main(int argc, char **argv) {
    if (argc < 7 || (argc - 4) % 3) { fprintf(stderr, "usage: %s hits.bin grid n_channels nbits channel mv [nbits channel mv ..]\n", argv[0]); return 2; }
    const int grid = atoi(argv[2]), n_channels = atoi(argv[3]), n = (argc - 4) / 3;
    if (n_channels < 1 || grid < 1) { fprintf(stderr, "grid and n_channels from 1\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> bits((size_t)n * 165);                           // exactly what the kernel may index: a read beyond it is the sanitizer's to report
    const size_t got = fread(bits.data(), 1, bits.size(), f);
    fclose(f);
    if (got != bits.size()) { fprintf(stderr, "%s: %zu of %zu bytes\n", argv[1], got, bits.size()); return 2; }
    std::vector<int> nbits((size_t)n), channel((size_t)n); std::vector<float> mv((size_t)n);
    for (int i = 0; i < n; i++) { nbits[(size_t)i] = atoi(argv[4 + 3 * i]); channel[(size_t)i] = atoi(argv[5 + 3 * i]); mv[(size_t)i] = (float)atof(argv[6 + 3 * i]); }
    const size_t per = (size_t)emu_m20_chan_chars();
    std::vector<char> chars((size_t)n_channels * per, 0);
    std::vector<sonde_m20_frame_t> out((size_t)n);
    memset((void *)out.data(), 0xEE, out.size() * sizeof(sonde_m20_frame_t));
    unsigned done[2] = { 0u, 0u };
    const int rc = emu_m20_hits_run(bits.data(), nbits.data(), channel.data(), mv.data(), n_channels, n, (unsigned)n, grid, chars.data(), out.data(), done);
    if (rc < 0) { fprintf(stderr, "emu_m20_hits_run: %d\n", rc); return 1; }
    for (const sonde_m20_frame_t &r : out) {
        uint32_t mvb; memcpy(&mvb, &r.mv, 4);
        printf("%d %d %d %d %u %d %d %u %08x ", r.channel, r.nbits, r.len, r.cs_ok, r.cs_calc, r.blk_ok, r.fw, r.mv_pos, mvb);
        for (int k = 0; k < 172; k++) printf("%02x", r.frame[k]);
        printf("\n");
    }
    for (int c = 0; c < n_channels; c++) {
        for (size_t k = 0; k < per; k++) printf("%02x", (unsigned char)chars[(size_t)c * per + k]);
        printf("\n");
    }
    fprintf(stderr, "%d records, done %u ticket %u\n", n, done[0], done[1]);
    return 0;
}
