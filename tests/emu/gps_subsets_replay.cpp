// gps_subsets_replay.cpp — test infrastructure: a stand-alone program around emu_gps_solve (gps_subsets_emu.cpp) for sanitizer builds of the emulated subset search,
// outside any interpreter:
//   gps_subsets_replay <file of sonde_gps_job_t>      -> one line per job on stdout: num best doubt n and the 16 hex digits of gdop
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/sonde_rs92.h"

extern "C" int emu_gps_solve(void *ctx, const sonde_gps_job_t *jobs, int32_t n, sonde_gps_pick_t *picks);

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s jobs.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<sonde_gps_job_t> jobs;
    sonde_gps_job_t j;
    while (fread(&j, sizeof j, 1, f) == 1) jobs.push_back(j);
    fclose(f);
    std::vector<sonde_gps_pick_t> picks(jobs.size());
    int64_t count = 0;
    const int rc = emu_gps_solve(&count, jobs.data(), (int32_t)jobs.size(), picks.data());
    if (rc != 0 || count != (int64_t)jobs.size()) { fprintf(stderr, "emu_gps_solve: %d\n", rc); return 1; }
    for (const sonde_gps_pick_t &p : picks) {
        uint64_t bits;
        memcpy(&bits, &p.gdop, 8);
        printf("%d %d %d %d %016llx\n", p.num, p.best, p.doubt, p.n, (unsigned long long)bits);
    }
    return 0;
}
