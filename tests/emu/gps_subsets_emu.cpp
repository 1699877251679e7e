// gps_subsets_emu.cpp — test infrastructure: the device RS92 subset search (csrc/sonde_gps_dev.h: closed form and GDOP of every 4-satellite subset on one wave, the
// arg-min by ballots) compiled for the CPU under wave_emu.h, driven the way sonde_gps_dev_solve drives k_gps_subsets: one wave per job, the job copied to a buffer of
// its own (LDS does not survive a launch), lane 0's pick.  Built with -ffp-contract=off; the libm is the host's, so every pick, `doubt` included, is what the device
// gives wherever the two libms decide alike.
//   emu_gps_solve(ctx, jobs, n, picks)      the signature of sonde_gps_solve_fn (include/sonde_rs92.h); ctx: NULL or an int64_t that counts the jobs
//   emu_gps_unrank(n, at, ix4)              the subset the wave takes for index `at`
#include "wave_emu.h"
#include "../../radiosonde_auto_rx_amd/csrc/sonde_gps_dev.h"
#include <cstring>

extern "C" int emu_gps_solve(void *ctx, const sonde_gps_job_t *jobs, int32_t n, sonde_gps_pick_t *picks) {
    if (n < 0 || (n > 0 && (!jobs || !picks))) return -1;
    for (int i = 0; i < n; i++) if (jobs[i].n < 4 || jobs[i].n > SONDE_GPS_MAX_SATS) return -1;
    for (int i = 0; i < n; i++) {
        sonde_gps_job_t lds;
        memcpy(&lds, jobs + i, sizeof lds);
        memset((void *)(picks + i), 0xEE, sizeof *picks);
        emu::run_workgroup(64, [&](int tid) { gps_wave_solve(&lds, tid, picks + i); });
    }
    if (ctx) *(int64_t *)ctx += n;
    return 0;
}

extern "C" int emu_gps_unrank(int n, int at, int *ix4) {
    if (!ix4 || n < 4 || n > SONDE_GPS_MAX_SATS || at < 0 || at >= n * (n - 1) * (n - 2) * (n - 3) / 24) return -1;
    gpsd_unrank4(n, at, ix4, ix4 + 1, ix4 + 2, ix4 + 3);
    return 0;
}
