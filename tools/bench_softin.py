"""Wall time of the LMS6 soft-bit consumer on the device (SoftinDev(kind="lms6"): k_softin_lms6 — header search, block assembly, wave Viterbi — plus the
per-channel host decoder behind block_bytes) per second of soft bits, beside the host tier (sonde_lms6_dec_push_soft: everything on one CPU thread) on the
same streams on the same machine.

N channels x one second (4800 soft bits) per push, the soft bits already in device memory: a 13 s stream of 15 LMS6 blocks (15 x 4160 = 13 x 4800 bits) at
sigma 0.3, repeated, so that every push continues the stream of the one before.  One warm-up round of 13 pushes (module load, the first blocks), then
--pushes timed pushes (>= 30), each waiting for its kernels, the copies of its blocks and the host decoders: median, min and max per push.  The kernel time
alone comes from a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/bench_softin.py --channels 1024`.  The host tier is timed on
--host-channels channels of the same stream (one thread; the figure is per channel and second, and scales linearly).  One JSON line per channel count.

    python tools/bench_softin.py [--channels 1,64,341,1024] [--pushes 39] [--vit 2] [--typ 0] [--out profiles/softin_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def lms6_stream(sigma=0.3, seed=1):
    from tools import synth
    bits = synth.lms6_onair_bits(15)
    assert len(bits) == 13 * 4800
    rng = np.random.default_rng(seed)
    return (2.0 * bits.astype(np.float64) - 1.0 + rng.normal(0.0, sigma, len(bits))).astype(np.float32)


def host_tier(s, pushes, nch, vit, typ):
    """ms per push of one channel through sonde_lms6_dec_push_soft (median over the timed pushes), [OK] frames of one channel"""
    from radiosonde_auto_rx_amd.engine import lib
    from radiosonde_auto_rx_amd.fsk import Lms6Opts
    L = lib()
    L.sonde_lms6_dec_create.argtypes = [C.POINTER(Lms6Opts), C.POINTER(C.c_void_p)]
    L.sonde_lms6_dec_destroy.argtypes = [C.c_void_p]
    L.sonde_lms6_dec_push_soft.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]
    o = Lms6Opts(json=1, vit=vit, typ=typ)
    decs = []
    for _ in range(nch):
        d = C.c_void_p()
        assert L.sonde_lms6_dec_create(C.byref(o), C.byref(d)) == 0
        decs.append(d)
    out = C.create_string_buffer(1 << 16)
    walls, ok = [], 0
    for k in range(13 + pushes):
        p = s.ctypes.data + (k % 13) * 4800 * 4
        t0 = time.perf_counter()
        for d in decs:
            n = L.sonde_lms6_dec_push_soft(d, p, 4800, 0, 0, out, len(out))
            assert n >= 0
        dt = (time.perf_counter() - t0) * 1e3
        if k >= 13:
            walls.append(dt / nch)
            ok += out.value.count(b"[OK]")
    for d in decs:
        L.sonde_lms6_dec_destroy(d)
    return walls, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="1,64,341,1024")
    ap.add_argument("--pushes", type=int, default=39)
    ap.add_argument("--vit", type=int, default=2)
    ap.add_argument("--typ", type=int, default=0)
    ap.add_argument("--host-channels", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.pushes >= 30
    import torch
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    s = lms6_stream()
    hw, hok = host_tier(s, a.pushes, a.host_channels, a.vit, a.typ)
    host_ms = statistics.median(hw)
    rows = []
    for nch in [int(c) for c in a.channels.split(",")]:
        d = torch.from_numpy(s).to("cuda").repeat(nch, 1).contiguous()
        torch.cuda.synchronize()
        sf = SoftinDev(nch, kind="lms6", json=True, vit=a.vit, typ=a.typ, ecc=0)
        walls, ok, blocks = [], 0, 0
        for k in range(13 + a.pushes):
            p = d.data_ptr() + (k % 13) * 4800 * 4
            t0 = time.perf_counter()
            sf.push_device(p, d.shape[1], 4800)
            dt = (time.perf_counter() - t0) * 1e3
            recs = sf.fetch_lms6(2 * nch + 16)
            if k >= 13:
                walls.append(dt)
                blocks += len(recs)
                ok += sum(r["text"].count("[OK]") for r in recs if r["channel"] == 0)
        cnt = sf.counts()
        sf.close()
        wall = statistics.median(walls)
        row = {"kind": "lms6", "vit": a.vit, "typ": a.typ, "channels": nch, "pushes": a.pushes, "push_ms": round(wall, 3), "min_ms": round(min(walls), 3),
               "max_ms": round(max(walls), 3), "channel_seconds_per_second": round(nch * 1e3 / wall, 1), "blocks": blocks, "ok_channel0": ok, "dropped": cnt["dropped"],
               "host_tier_ms_per_channel_second": round(host_ms, 3), "host_tier_min_ms": round(min(hw), 3), "host_tier_max_ms": round(max(hw), 3),
               "host_tier_ms_for_these_channels": round(host_ms * nch, 1), "host_tier_ok_one_channel": hok}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
