// sonde_gps.hip — the RS92 position solve's 4-satellite subset search on the device (include/sonde_gps.h).
//
// k_gps_subsets: one wavefront per workgroup, one workgroup per job.  The job (680 bytes) is staged in LDS; lane l takes subsets l, l + 64, .. of the C(n,4) <= 495
//   in the order of the decoder's nested loops (at most 8 rounds), each the closed-form solution and the GDOP in FP64 with the host's order of operations and
//   no fused multiply-add (sonde_gps_dev.h); the wave counts the solutions, finds the first smallest GDOP and writes one 24-byte pick.  Nothing else: what is
//   printed is computed by the host from the winning subset.
// The host object below owns the buffers for max_jobs jobs, a stream of its own, and the counts.
#include <hip/hip_runtime.h>
#include "sonde_gps_dev.h"
#include "../../include/sonde_gps.h"
#include "../../include/sonde_hip.h"
#include "sonde_devmem.h"
#include "sonde_pinned.h"
#include <cmath>
#include <cstring>
#include <memory>

static_assert(sizeof(sonde_gps_job_t) == 680 && sizeof(sonde_gps_job_t) % 8 == 0, "a job is copied to LDS as 64-bit words");
static_assert(sizeof(sonde_gps_pick_t) == 24, "sonde_gps_pick_t is part of the ABI");

__global__ __launch_bounds__(64) void k_gps_subsets(const sonde_gps_job_t *__restrict__ jobs, sonde_gps_pick_t *__restrict__ picks, const int n_jobs) {
    __shared__ sonde_gps_job_t job;
    const int lane = threadIdx.x, j = blockIdx.x;
    if (j >= n_jobs) return;
    const unsigned long long *src = (const unsigned long long *)(jobs + j);
    unsigned long long *dst = (unsigned long long *)&job;
    for (int i = lane; i < (int)(sizeof(sonde_gps_job_t) / 8); i += 64) dst[i] = src[i];
    __syncthreads();
    if (job.n < 4 || job.n > SONDE_GPS_MAX_SATS) {                  // (the host has refused such a job; a pick all the same, never an index out of the job)
        if (lane == 0) { sonde_gps_pick_t p; p.num = 0; p.best = -1; p.doubt = 0; p.n = job.n; p.gdop = 0.0; picks[j] = p; }
        return;
    }
    gps_wave_solve(&job, lane, picks + j);
}

struct sonde_gps_dev {
    DevMem mem;
    ~sonde_gps_dev() { if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); } }
    int max_jobs = 0;
    hipStream_t stream = nullptr;
    sonde_gps_job_t *d_jobs = nullptr; Pinned<sonde_gps_job_t> h_jobs;
    sonde_gps_pick_t *d_picks = nullptr; Pinned<sonde_gps_pick_t> h_picks;
    sonde_gps_stats_t st{};
};

static int gps_solve_cb(void *ctx, const sonde_gps_job_t *jobs, int32_t n, sonde_gps_pick_t *picks) { return sonde_gps_dev_solve((sonde_gps_dev *)ctx, jobs, n, picks); }

extern "C" {

int sonde_gps_dev_create(int32_t max_jobs, sonde_gps_dev_t **out) {
    if (!out || max_jobs < 1 || max_jobs > 65536) return SONDE_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); return SONDE_E_NOGPU; }
    std::unique_ptr<sonde_gps_dev> g(new sonde_gps_dev());
    g->max_jobs = max_jobs;
    TRY(g->mem.dalloc(&g->d_jobs, (size_t)max_jobs));
    TRY(g->mem.dalloc(&g->d_picks, (size_t)max_jobs));
    if (!g->h_jobs.alloc((size_t)max_jobs) || !g->h_picks.alloc((size_t)max_jobs)) return SONDE_E_NOMEM;
    HIPCHK(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    *out = g.release();
    return 0;
}

void sonde_gps_dev_destroy(sonde_gps_dev_t *g) { delete g; }

int sonde_gps_dev_solve(sonde_gps_dev_t *g, const sonde_gps_job_t *jobs, int32_t n, sonde_gps_pick_t *picks) {
    if (!g || n < 0 || (n > 0 && (!jobs || !picks))) return SONDE_E_ARG;
    for (int i = 0; i < n; i++) {
        const sonde_gps_job_t &j = jobs[i];
        if (j.n < 4 || j.n > SONDE_GPS_MAX_SATS) return SONDE_E_ARG;
        for (int k = 0; k < j.n; k++) {
            const sonde_gps_sat_t &s = j.sat[k];
            if (!(std::isfinite(s.X) && std::isfinite(s.Y) && std::isfinite(s.Z) && std::isfinite(s.x) && std::isfinite(s.y) && std::isfinite(s.z) && std::isfinite(s.p)))
                return SONDE_E_ARG;
        }
    }
    for (int at = 0; at < n; at += g->max_jobs) {
        const int m = n - at < g->max_jobs ? n - at : g->max_jobs;
        memcpy(g->h_jobs.data(), jobs + at, (size_t)m * sizeof(sonde_gps_job_t));
        HIPCHK(hipMemcpyAsync(g->d_jobs, g->h_jobs.data(), (size_t)m * sizeof(sonde_gps_job_t), hipMemcpyHostToDevice, g->stream));
        hipLaunchKernelGGL(k_gps_subsets, dim3((unsigned)m), dim3(64), 0, g->stream, g->d_jobs, g->d_picks, m);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(g->h_picks.data(), g->d_picks, (size_t)m * sizeof(sonde_gps_pick_t), hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
        memcpy(picks + at, g->h_picks.data(), (size_t)m * sizeof(sonde_gps_pick_t));
        g->st.jobs += m; g->st.launches += 1;
        for (int i = 0; i < m; i++) g->st.doubts += picks[at + i].doubt != 0;
    }
    return 0;
}

int sonde_gps_dev_stats(const sonde_gps_dev_t *g, sonde_gps_stats_t *out) {
    if (!g || !out) return SONDE_E_ARG;
    *out = g->st;
    return 0;
}

int sonde_gps_rs92_text_batch(sonde_gps_dev_t *g, sonde_rs92_dec_t *const *decs, const uint8_t (*frames)[SONDE_RS92_FRAME_LEN], const int32_t *ec, int32_t n,
                              char *out, size_t stride, int32_t *len) {
    if (!g) return sonde_gps_rs92_text_batch_with(nullptr, nullptr, decs, frames, ec, n, out, stride, len, nullptr);
    int64_t via[4] = {0, 0, 0, 0};
    const int rc = sonde_gps_rs92_text_batch_with(gps_solve_cb, g, decs, frames, ec, n, out, stride, len, via);
    g->st.mismatches += via[SONDE_GPS_VIA_MISMATCH];
    g->st.picked += via[SONDE_GPS_VIA_PICK];
    return rc;
}

}  // extern "C"
