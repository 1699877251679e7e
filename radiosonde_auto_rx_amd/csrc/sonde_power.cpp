// sonde_power.cpp — host engine of the spectrum survey (include/sonde_power.h): configuration, the exact twiddle and window tables, the
// carried tail, the launch shape, fetch (un-permute, shift, crop, dB), and auto_rx's peak pick and log line as pure host functions.
#include "../../include/sonde_power.h"
#include "sonde_power_dev.h"
#include "sonde_devmem.h"
#include "sonde_pinned.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace {
struct KStat { double ms = 0; int64_t n = 0; };
}

struct sonde_power {
    DevMem mem;
    ~sonde_power() {
        if (stream) { hipStreamSynchronize(stream); hipStreamDestroy(stream); }
        if (ev0) hipEventDestroy(ev0);
        if (ev1) hipEventDestroy(ev1);
    }
    sonde_power_cfg_t cfg{};
    sonde_power_info_t info{};
    int log2n = 0, drop = 0;
    size_t unit = 4;                       // bytes per complex sample
    double scale = 1.0;                    // accumulator -> power of a full-scale sinusoid = 1: 1 / window_sum^2
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool ev_pending = false;
    float2 *d_tw = nullptr; float *d_win = nullptr, *d_partial = nullptr; double *d_acc = nullptr;
    uint8_t *d_tail = nullptr, *d_stage = nullptr;
    size_t stage_bytes = 0;
    Pinned<uint8_t> h_stage;
    Pinned<double> h_acc;
    int tail_len = 0;
    std::vector<int64_t> segments;
    std::map<std::string, KStat> stats;
};

static int settle_timing(sonde_power *s) {
    if (!s->ev_pending) return 0;
    HIPCHK(hipEventSynchronize(s->ev1));
    float ms = 0; if (hipEventElapsedTime(&ms, s->ev0, s->ev1) == hipSuccess) { auto &k = s->stats["k_power"]; k.ms += ms; k.n += 1; }
    s->ev_pending = false;
    return 0;
}

extern "C" {

int sonde_power_create(const sonde_power_cfg_t *cfg, sonde_power_t **out) {
    if (!cfg || !out || cfg->abi_version != SONDE_ABI_VERSION) return SONDE_E_ARG;
    if (cfg->n_streams < 1 || cfg->n_streams > 65535 || cfg->sample_rate < 1 || cfg->max_chunk < 1) return SONDE_E_ARG;
    if (cfg->bits != 16 && cfg->bits != 8 && cfg->bits != 32) return SONDE_E_ARG;
    if (cfg->nfft < SONDE_POWER_NFFT_MIN || cfg->nfft > SONDE_POWER_NFFT_MAX || (cfg->nfft & (cfg->nfft - 1))) return SONDE_E_ARG;
    if (cfg->window != SONDE_POWER_RECT && cfg->window != SONDE_POWER_HANN) return SONDE_E_ARG;
    if (!(cfg->crop >= 0.f) || !(cfg->crop < 1.f) || !std::isfinite(cfg->center_hz)) return SONDE_E_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || cfg->device < 0 || cfg->device >= ndev) {
        fprintf(stderr, "libsonde_hip: no usable HIP device (the survey has no CPU fallback)\n");
        return SONDE_E_NOGPU;
    }
    HIPCHK(hipSetDevice(cfg->device));
    std::unique_ptr<sonde_power> owner(new sonde_power());
    sonde_power *s = owner.get();
    s->cfg = *cfg;
    const int N = cfg->nfft, C = cfg->n_streams;
    while ((1 << s->log2n) < N) s->log2n++;
    s->unit = 2 * (size_t)(cfg->bits / 8);
    s->drop = (int)((double)cfg->crop * N / 2.0);
    s->segments.assign(C, 0);

    // exact tables: evaluated in double, rounded once
    const double PI = 3.14159265358979323846;
    std::vector<float> tw((size_t)N), win;
    for (int m = 0; m < N / 2; m++) { tw[2 * m] = (float)std::cos(2.0 * PI * m / N); tw[2 * m + 1] = (float)-std::sin(2.0 * PI * m / N); }
    double wsum = (double)N;
    if (cfg->window == SONDE_POWER_HANN) {
        win.resize(N); wsum = 0.0;
        for (int i = 0; i < N; i++) { win[i] = (float)(0.5 - 0.5 * std::cos(2.0 * PI * i / N)); wsum += (double)win[i]; }
    }
    s->scale = 1.0 / (wsum * wsum);                            // (the kernel has already divided by 32768 / 128)

    PowerKernelInfo ki{};
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) return SONDE_E_NOGPU;
    if (sonde_power_kernel_info(s->log2n, &ki) != 0) return SONDE_E_NOGPU;
    s->info.nfft = N; s->info.bins = N - 2 * s->drop;
    s->info.threads = ki.threads; s->info.lds_bytes = ki.lds_bytes; s->info.workgroups_per_cu = ki.max_per_cu;
    s->info.max_workgroups = std::max(1, prop.multiProcessorCount) * ki.max_per_cu;
    s->info.step_hz = (double)cfg->sample_rate / N; s->info.window_sum = wsum;

    HIPCHK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&s->ev0)); HIPCHK(hipEventCreate(&s->ev1));
    const size_t rows = (size_t)std::max(C, s->info.max_workgroups);        // every stream gets at least one workgroup
    { float *q = nullptr; TRY(s->mem.upload(&q, tw)); s->d_tw = (float2 *)q; }      // (re, im) pairs
    if (!win.empty()) TRY(s->mem.upload(&s->d_win, win));
    TRY(s->mem.dalloc(&s->d_partial, rows * N, false)); TRY(s->mem.dalloc(&s->d_acc, (size_t)C * N)); TRY(s->mem.dalloc(&s->d_tail, (size_t)C * N * s->unit));
    if (!s->h_acc.alloc(N)) return SONDE_E_NOMEM;
    *out = owner.release();
    return 0;
}

void sonde_power_destroy(sonde_power_t *s) { delete s; }

int sonde_power_info(const sonde_power_t *s, sonde_power_info_t *info) {
    if (!s || !info) return SONDE_E_ARG;
    *info = s->info;
    return 0;
}

int sonde_power_reset(sonde_power_t *s) {
    if (!s) return SONDE_E_ARG;
    HIPCHK(hipMemsetAsync(s->d_acc, 0, (size_t)s->cfg.n_streams * s->cfg.nfft * sizeof(double), s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    s->tail_len = 0;
    std::fill(s->segments.begin(), s->segments.end(), 0);
    return 0;
}

int sonde_power_process_device(sonde_power_t *s, const void *d_in, int64_t stream_stride, int32_t n_samples) {
    if (!s || !d_in) return SONDE_E_ARG;
    if (n_samples <= 0 || n_samples > s->cfg.max_chunk || stream_stride < n_samples) return SONDE_E_RANGE;
    const int N = s->cfg.nfft, C = s->cfg.n_streams;
    const int64_t total = (int64_t)s->tail_len + n_samples;
    const int nseg = (int)(total / N), rem = (int)(total % N);
    PowerArgs a{};
    a.in = d_in; a.tail = s->d_tail; a.tw = s->d_tw; a.win = s->d_win; a.partial = s->d_partial; a.acc = s->d_acc;
    a.stride = stream_stride; a.tail_len = s->tail_len; a.nseg = nseg; a.n_streams = C; a.bits = s->cfg.bits; a.log2n = s->log2n;
    // launch shape: what the device holds at once (compute units * occupancy) shared among the streams, never more workgroups than segments
    a.workgroups = std::max(1, std::min(nseg, s->info.max_workgroups / C));
    // behind the last whole segment: all of it lies in this call's input once a segment was completed (tail_len < nfft)
    const int src_off = nseg ? (int)((int64_t)nseg * N - s->tail_len) : 0, dst_off = nseg ? 0 : s->tail_len, count = nseg ? rem : n_samples;
    if (settle_timing(s)) return SONDE_E_NOGPU;
    HIPCHK(hipEventRecord(s->ev0, s->stream));
    const int rc = sonde_launch_power(&a, s->d_tail, src_off, dst_off, count, s->stream);
    if (rc) return rc;
    HIPCHK(hipEventRecord(s->ev1, s->stream));
    s->ev_pending = true;
    s->tail_len = rem;
    for (auto &k : s->segments) k += nseg;
    return 0;
}

int sonde_power_process_host(sonde_power_t *s, const void *h_in, int64_t stream_stride, int32_t n_samples) {
    if (!s || !h_in) return SONDE_E_ARG;
    if (n_samples <= 0 || n_samples > s->cfg.max_chunk || stream_stride < n_samples) return SONDE_E_RANGE;
    const int C = s->cfg.n_streams;
    const size_t row = (size_t)n_samples * s->unit, need = row * C;
    if (need > s->stage_bytes) {
        if (s->d_stage) { hipStreamSynchronize(s->stream); s->mem.release(s->d_stage); s->stage_bytes = 0; }
        TRY(s->mem.dalloc(&s->d_stage, need, false));
        if (!s->h_stage.alloc(need)) return SONDE_E_NOMEM;
        s->stage_bytes = need;
    }
    HIPCHK(hipStreamSynchronize(s->stream));                   // the staging buffer's last transfer and its readers are done
    for (int c = 0; c < C; c++) memcpy(s->h_stage.data() + (size_t)c * row, (const uint8_t *)h_in + (size_t)c * (size_t)stream_stride * s->unit, row);
    HIPCHK(hipMemcpyAsync(s->d_stage, s->h_stage.data(), need, hipMemcpyHostToDevice, s->stream));
    return sonde_power_process_device(s, s->d_stage, n_samples, n_samples);
}

int64_t sonde_power_segments(const sonde_power_t *s, int32_t stream) {
    if (!s || stream < 0 || stream >= s->cfg.n_streams) return SONDE_E_ARG;
    return s->segments[stream];
}

int sonde_power_fetch(sonde_power_t *s, int32_t stream, float *db, double *f_low_hz, double *f_high_hz, double *step_hz, int32_t max, int reset) {
    if (!s || stream < 0 || stream >= s->cfg.n_streams) return SONDE_E_ARG;
    const int N = s->cfg.nfft, bins = s->info.bins, L = s->log2n;
    const double step = s->info.step_hz;
    if (f_low_hz) *f_low_hz = s->cfg.center_hz + (double)(s->drop - N / 2) * step;
    if (f_high_hz) *f_high_hz = s->cfg.center_hz + (double)(s->drop + bins - 1 - N / 2) * step;
    if (step_hz) *step_hz = step;
    if (!db) return bins;
    if (max < bins) return SONDE_E_RANGE;
    double *d_row = s->d_acc + (size_t)stream * N;
    HIPCHK(hipMemcpyAsync(s->h_acc.data(), d_row, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    if (reset) HIPCHK(hipMemsetAsync(d_row, 0, (size_t)N * sizeof(double), s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    const int64_t nseg = s->segments[stream];
    const double k = nseg > 0 ? s->scale / (double)nseg : 0.0;
    for (int j = 0; j < bins; j++) {
        const unsigned b = (unsigned)(j + s->drop + N / 2) & (unsigned)(N - 1);         // ascending frequency -> transform bin
        unsigned r = 0; for (int t = 0; t < L; t++) r |= ((b >> t) & 1u) << (L - 1 - t);   // where the bit-reversed network left it
        const double p = s->h_acc[r] * k;
        double v = SONDE_POWER_FLOOR_DB;
        if (p > 0.0) { v = 10.0 * std::log10(p); if (!(v > SONDE_POWER_FLOOR_DB)) v = SONDE_POWER_FLOOR_DB; if (!(v < 400.0)) v = 400.0; }
        db[j] = (float)v;
    }
    if (reset) s->segments[stream] = 0;
    return bins;
}

int sonde_power_kernel_ms(sonde_power_t *s, const char *kernel, double *avg_ms, int64_t *launches) {
    if (!s || !kernel) return SONDE_E_ARG;
    if (settle_timing(s)) return SONDE_E_NOGPU;
    auto it = s->stats.find(kernel);
    if (it == s->stats.end() || it->second.n == 0) { if (avg_ms) *avg_ms = 0; if (launches) *launches = 0; return 0; }
    if (avg_ms) *avg_ms = it->second.ms / (double)it->second.n;
    if (launches) *launches = it->second.n;
    return 0;
}

// ---- auto_rx's peak pick (scan.py:1007-1063, utils.py detect_peaks with edge = "rising", threshold = 0, kpsh = False), operation by operation
int sonde_power_peaks(const double *db, int32_t n, double f_low_hz, double f_high_hz, double step_hz,
                      double snr_threshold_db, double min_distance_hz, double quantization_hz, double min_freq_hz, double max_freq_hz,
                      const double *never_scan_hz, int32_t n_never_scan, int32_t max_peaks,
                      double *noise_floor_db, double *peaks_hz, int32_t max_out) {
    if (n < 0 || (n > 0 && !db) || n_never_scan < 0 || (n_never_scan > 0 && !never_scan_hz) || max_out < 0 || (max_out > 0 && !peaks_hz)) return SONDE_E_ARG;
    const double NaN = std::nan("");
    // np.median: NaN if any value is one; the mean of the two middle values for an even count
    double nf = NaN;
    bool any_nan = false;
    for (int i = 0; i < n; i++) any_nan |= std::isnan(db[i]);
    if (n > 0 && !any_nan) {
        std::vector<double> v(db, db + n);
        std::sort(v.begin(), v.end());
        nf = (n & 1) ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0;
    }
    if (noise_floor_db) *noise_floor_db = nf;
    if (n < 3) return 0;
    const double mph = nf + snr_threshold_db, mpd = min_distance_hz / step_hz;

    // detect_peaks: dx before the NaNs are replaced; then x NaN -> inf, dx NaN -> inf (only if x had a NaN)
    std::vector<double> x(db, db + n), dx(n - 1);
    for (int i = 0; i + 1 < n; i++) dx[i] = x[i + 1] - x[i];
    if (any_nan) {
        for (int i = 0; i < n; i++) if (std::isnan(x[i])) x[i] = INFINITY;
        for (auto &d : dx) if (std::isnan(d)) d = INFINITY;
    }
    std::vector<int> ind;
    for (int i = 1; i < n - 1; i++) {                        // (index 0 has no rise before it; the last value cannot be a peak)
        if (!(dx[i] <= 0 && dx[i - 1] > 0)) continue;
        if (any_nan && (std::isnan(db[i]) || std::isnan(db[i - 1]) || std::isnan(db[i + 1]))) continue;
        if (x[i] >= mph) ind.push_back(i);
    }
    if (!ind.empty() && mpd > 1) {
        std::vector<int> ord(ind);
        std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return x[a] < x[b]; });
        std::reverse(ord.begin(), ord.end());                // by height, descending
        std::vector<char> del(ord.size(), 0);
        for (size_t i = 0; i < ord.size(); i++) {
            if (del[i]) continue;
            for (size_t j = 0; j < ord.size(); j++) if ((double)ord[j] >= (double)ord[i] - mpd && (double)ord[j] <= (double)ord[i] + mpd) del[j] = 1;
            del[i] = 0;
        }
        ind.clear();
        for (size_t i = 0; i < ord.size(); i++) if (!del[i]) ind.push_back(ord[i]);
        std::sort(ind.begin(), ind.end());
    }
    if (ind.empty()) return 0;

    // freq = np.linspace(f_low, f_high, n)
    const double delta = f_high_hz - f_low_hz, lstep = delta / (double)(n - 1);
    auto freq = [&](int i) { return i == n - 1 ? f_high_hz : (lstep == 0 ? ((double)i / (double)(n - 1)) * delta : (double)i * lstep) + f_low_hz; };
    // by power, descending; quantise (np.round: half to even, the default rounding mode of nearbyint)
    std::stable_sort(ind.begin(), ind.end(), [&](int a, int b) { return db[a] < db[b]; });
    std::reverse(ind.begin(), ind.end());
    std::vector<double> pk;
    for (int i : ind) {
        const double f = std::nearbyint(freq(i) / quantization_hz) * quantization_hz;
        if (std::find(pk.begin(), pk.end(), f) == pk.end()) pk.push_back(f);           // duplicates out, first kept
    }
    const double hq = quantization_hz / 2.0;
    const double lo = min_freq_hz - hq, hi = max_freq_hz + hq;
    pk.erase(std::remove_if(pk.begin(), pk.end(), [&](double f) { return f < lo || f > hi; }), pk.end());
    for (int k = 0; k < n_never_scan; k++) {
        const double nv = never_scan_hz[k];
        pk.erase(std::remove_if(pk.begin(), pk.end(), [&](double f) { return std::fabs(f - nv) < hq; }), pk.end());
    }
    if (max_peaks >= 0 && (int)pk.size() > max_peaks) pk.resize(max_peaks);
    for (size_t i = 0; i < pk.size() && (int)i < max_out; i++) peaks_hz[i] = pk[i];
    return (int)pk.size();
}

int sonde_power_csv_line(int64_t unix_time, double f_low_hz, double f_high_hz, double step_hz, int64_t samples,
                         const float *db, int32_t n, char *buf, size_t buflen) {
    if (n < 0 || (n > 0 && !db) || (!buf && buflen)) return SONDE_E_ARG;
    auto exact = [](double v) {                               // the fewest digits that read back to the same double
        char t[40];
        for (int p = 15; p <= 17; p++) { snprintf(t, sizeof t, "%.*g", p, v); if (strtod(t, nullptr) == v) break; }
        return std::string(t);
    };
    std::string o;
    char t[64];
    const time_t tt = (time_t)unix_time;
    struct tm tmv;
    gmtime_r(&tt, &tmv);
    strftime(t, sizeof t, "%Y-%m-%d, %H:%M:%S", &tmv); o += t;
    o += ", " + exact(f_low_hz) + ", " + exact(f_high_hz);
    o += ", " + exact(step_hz);
    snprintf(t, sizeof t, ", %lld", (long long)samples); o += t;
    for (int i = 0; i < n; i++) { snprintf(t, sizeof t, ", %.2f", (double)db[i]); o += t; }
    o += "\n";
    if (o.size() + 1 <= buflen) memcpy(buf, o.c_str(), o.size() + 1);
    else if (buflen) buf[0] = 0;
    return (int)o.size();
}

}  // extern "C"
