"""Throughput of the Weathex WxR-301D engine (the iq_dec front end + k_wxr_slice) on auto_rx's form (iq_dec --FM --IFbw 64 --lpFM --iq 0.0 |
weathex301d -b) at 96 kHz:
per second of signal, the call wall time (input already on the device, process_device; one call per 0.25 s of signal, as the CLI makes them;
each call waits for its kernels and the frame-count copy, so this is an upper bound of the GPU time).  The kernel time alone comes from a run
under `rocprofv3 --kernel-trace --stats -- python tools/bench_wxr.py --channels 1024 --repeat 1`.  A warm-up call precedes the timed ones; the
timed region is repeated --repeat times with a fresh engine, and the median and the spread are reported.  Prints one JSON line per channel count and writes them to --out.

The single-core time of the reference's `iq_dec | weathex301d` on such a capture is measured where the goldens are made (tools/make_golden_wxr.py prints it); it is
passed in with --ref-seconds-per-signal-s only to be quoted next to the result.

    python tools/bench_wxr.py [--seconds 2] [--channels 1,64,1024] [--out profiles/wxr_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--channels", default="1,64,1024")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--ref-seconds-per-signal-s", type=float, default=0.0)
    a = ap.parse_args()
    import torch
    from radiosonde_auto_rx_amd.wxr import WxrEngine
    from tools import synth
    sr = 96000
    chunk = sr // 4
    calls = int(a.seconds * sr) // chunk
    one = synth.wxr_capture(sr, n_frames=int((calls + 1) * chunk / sr / 0.135) + 2, f_offset_hz=3000.0, noise=15.0, seed=3, lead_s=0.05)
    rows = []
    for nch in [int(c) for c in a.channels.split(",")]:
        x = torch.from_numpy(np.ascontiguousarray(one[:2 * chunk * (calls + 1)])).to("cuda")
        blocks = [x[2 * chunk * k:2 * chunk * (k + 1)].repeat(nch).contiguous() for k in range(calls + 1)]
        torch.cuda.synchronize()
        walls, nf = [], 0
        for _ in range(a.repeat):
            eng = WxrEngine([0.0] * nch, sr, if_bw_khz=64, opt_b=True, max_chunk=chunk)
            eng.process_device(blocks[0].data_ptr(), chunk)                  # warm-up (first call: module load)
            t0 = time.perf_counter()
            for k in range(1, calls + 1):
                eng.process_device(blocks[k].data_ptr(), chunk)
            walls.append((time.perf_counter() - t0) * 1e3)
            nf = len(eng.fetch_frames())
            eng.close()
        sig = calls * chunk / sr
        wall = statistics.median(walls)
        row = {"sr": sr, "channels": nch, "signal_s": sig, "call_ms_per_signal_s": round(wall / sig, 3),
               "min_ms_per_signal_s": round(min(walls) / sig, 3), "max_ms_per_signal_s": round(max(walls) / sig, 3), "repeat": a.repeat,
               "x_realtime_all_channels": round(sig * 1e3 / wall, 2), "channel_seconds_per_second": round(nch * sig * 1e3 / wall, 1),
               "frames": nf}
        if a.ref_seconds_per_signal_s > 0:
            row["reference_one_core_channels_realtime"] = round(1.0 / a.ref_seconds_per_signal_s, 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
