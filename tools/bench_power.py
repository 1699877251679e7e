"""Throughput of the spectrum survey (k_power_seg + k_power_fold + k_power_tail): GPU time by HIP events (sonde_power_kernel_ms) in ms per second of
stream and in Gsamples/s, for nfft 4096 and 16384 at 1 and 8 streams of 2.4 and 10 Msps cs16.  Input already on the device (process_device), one
call per 0.25 s of stream as the receiver makes them, at least --seconds of stream per configuration after a warm-up call.  Beside each figure:
the plain read rate of the same buffer on this box (sonde_probe_read_gbps) and the time that rate would need for the same bytes.
Prints one JSON line per configuration.

    python tools/bench_power.py [--seconds 1]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--nfft", default="4096,16384")
    ap.add_argument("--streams", default="1,8")
    ap.add_argument("--rates", default="2400000,10000000")
    a = ap.parse_args()
    import torch
    from radiosonde_auto_rx_amd.engine import lib
    from radiosonde_auto_rx_amd.power import HANN, PowerSurvey
    L = lib()
    L.sonde_probe_read_gbps.argtypes = [C.c_void_p, C.c_size_t, C.c_int32, C.POINTER(C.c_double)]
    rng = np.random.default_rng(1)
    for sr in [int(v) for v in a.rates.split(",")]:
        chunk = sr // 4
        calls = max(1, int(np.ceil(a.seconds * sr / chunk)))
        for ns in [int(v) for v in a.streams.split(",")]:
            x = torch.from_numpy(rng.integers(-3000, 3000, size=(ns, 2 * chunk), dtype=np.int16)).to("cuda")
            torch.cuda.synchronize()
            g = C.c_double(0)
            rc = L.sonde_probe_read_gbps(C.c_void_p(x.data_ptr()), C.c_size_t(x.numel() * 2), 5, C.byref(g))
            gbps = float(g.value) if rc == 0 and g.value > 0 else None
            for nfft in [int(v) for v in a.nfft.split(",")]:
                ps = PowerSurvey(sr, nfft, n_streams=ns, window=HANN, crop=0.25, max_chunk=chunk)
                ps.process_device(x.data_ptr(), chunk, chunk)                 # warm-up (first call: module load)
                ps.kernel_ms()
                ms0, n0 = ps.kernel_ms()
                for _ in range(calls):
                    ps.process_device(x.data_ptr(), chunk, chunk)
                ms1, n1 = ps.kernel_ms()
                gpu_ms = ms1 * n1 - ms0 * n0
                sig = calls * chunk / sr
                segs = ps.segments(0)
                info = ps.info
                ps.close()
                print(json.dumps({"sr": sr, "streams": ns, "nfft": nfft, "stream_s": sig, "calls": calls, "segments_per_stream": segs,
                                  "gpu_ms_per_stream_s": round(gpu_ms / sig, 4), "gpu_ms_per_stream_s_per_stream": round(gpu_ms / sig / ns, 4),
                                  "gsamples_per_s": round(ns * calls * chunk / (gpu_ms * 1e-3) / 1e9, 3),
                                  "read_gbps_same_buffer": None if gbps is None else round(gbps, 1),
                                  "read_ms_same_bytes": None if gbps is None else round(ns * calls * chunk * 4 / (gbps * 1e9) * 1e3 / sig, 4),
                                  "threads": info["threads"], "lds_bytes": info["lds_bytes"], "workgroups_per_cu": info["workgroups_per_cu"],
                                  "max_workgroups": info["max_workgroups"]}), flush=True)


if __name__ == "__main__":
    main()
