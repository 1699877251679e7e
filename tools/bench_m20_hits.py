"""What the M20 hits of a base-rate engine cost the host, both ways: ONE M20 engine of --channels channels at 48 kHz (the `--IQ 0.0` form), every
channel carrying the same capture, fed one second a call, the capture repeated.

    device path   the default: k_m20_hits behind the frame sync; timed: fetch_m20_raw (596 + 208 bytes a hit) + the raw text line per frame
    host path     set_device_ecc(False), the path as it was: the fetch copies every hit's 1320 float soft bits and runs the differential code, bits2bytes and both
                  checksums on one host thread; then the same text line per frame

Both paths run on the same samples in the same process, on the SAME engine, alternating pass by pass (a pass = the capture once through; the switch of
set_device_ecc needs everything queued fetched, which the end of a call is).  A call's samples are processed and the stream synchronised (Engine.sync) before the
timed region starts, so `fetch_decode_ms` is host time per second of signal with the device idle; `call_ms` is the whole call — process_host, the kernels (the device
path's k_m20_hits among them), fetch and text — under one clock.  Two warm-up passes, then passes until both paths have at least --seconds of timed fetch + decode
(and no fewer than --calls calls each).  One JSON line with medians, minima and maxima per call, the frames and good checksums of both paths (they must agree), the
bytes copied per hit both ways and the device's clocks.

    python tools/bench_m20_hits.py [--channels 256] [--seconds 1.0] [--calls 12] [--out profiles/m20_hits_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR = 48_000


def capture():
    """int16 IQ of six whole seconds: an M20 frame a second, firmware 6 and 8, every fifth checksum bad"""
    from tools import synth
    return synth.m10_capture(sr=SR, seconds=6.0, baud=9600.0, noise_sigma=0.05, seed=20, t_first=0.3,
                             frame_fn=lambda k: synth.m20_frame(k, fw=(6, 8)[k % 2], rng=np.random.default_rng(2000 + k), good_checksum=k % 5 != 4))


def run(a):
    import torch                                                                 # noqa: F401  (PyTorch's HIP runtime first)
    from bench import _device_clocks
    from radiosonde_auto_rx_amd.engine import Engine, lib
    x = capture()
    secs = len(x) // 2 // SR
    nch = a.channels
    blocks = [np.ascontiguousarray(np.broadcast_to(x[2 * SR * k:2 * SR * (k + 1)], (nch, 2 * SR))) for k in range(secs)]
    eng = Engine([0.0] * nch, SR, sonde="m20", ecc=0, lp_iq=True, max_chunk=SR, max_frames=8 * nch)
    stat = {p: dict(fd=[], call=[], frames=0, good=0) for p in ("device", "host")}
    line = C.create_string_buffer(420)
    rawline = lib().sonde_m20_rawline

    def one_call(p, k, timed):
        s = stat[p]
        t0 = time.perf_counter()
        eng.process_host(blocks[k % secs])
        eng.sync()
        t1 = time.perf_counter()
        buf, n = eng.fetch_m20_raw()
        good = 0
        for i in range(n):
            rawline(C.byref(buf[i]), 1, line, 420)
            good += buf[i].cs_ok
        t2 = time.perf_counter()
        if timed:
            s["fd"].append((t2 - t1) * 1e3); s["call"].append((t2 - t0) * 1e3); s["frames"] += n; s["good"] += good

    def one_pass(p, timed):
        eng.set_device_ecc(p == "device")                                        # (nothing is queued: every call ends with its fetch)
        for k in range(secs):
            one_call(p, k, timed)

    for _ in range(2):                                                           # warm-up: code objects, the first frames, both paths
        for p in stat:
            one_pass(p, False)
    clocks0 = _device_clocks()
    passes = 0
    while passes < 400 and (passes * secs < a.calls or min(sum(stat[p]["fd"]) for p in stat) < 1e3 * a.seconds):
        for p in (list(stat) if passes & 1 else list(stat)[::-1]):               # alternating: other people's work shares the box
            one_pass(p, True)
        passes += 1
    clocks1 = _device_clocks()
    ovf = eng.overflowed()
    eng.close()
    row = {"kind": "M20", "channels": nch, "calls": len(stat["device"]["fd"]), "signal_s_per_call": 1.0, "overflowed": bool(ovf)}
    for p, s in stat.items():
        row[p] = {"fetch_decode_ms": round(statistics.median(s["fd"]), 3), "fetch_decode_min_ms": round(min(s["fd"]), 3), "fetch_decode_max_ms": round(max(s["fd"]), 3),
                  "fetch_decode_timed_s": round(sum(s["fd"]) / 1e3, 3), "call_ms": round(statistics.median(s["call"]), 3), "call_min_ms": round(min(s["call"]), 3),
                  "call_max_ms": round(max(s["call"]), 3), "frames": s["frames"], "good": s["good"]}
    row["bytes_per_hit"] = {"device": 596 + 208, "host": 596 + 4 * 1320,
                            "note": "596 = the engine's hit record, which both paths copy; device: + sonde_m20_frame_t (208); host: + 1320 float soft bits"}
    row["clocks_before"], row["clocks_after"] = clocks0, clocks1
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=1.0, help="least timed fetch + decode time per path")
    ap.add_argument("--calls", type=int, default=12, help="least timed calls per path")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    row = run(a)
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump([row], f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
