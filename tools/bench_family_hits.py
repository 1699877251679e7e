"""What the block codes of a generic engine's hits cost the host, both ways: per kind — Meisei, iMet-54, MTS01, RS92 — a generic engine of
--channels channels at 48 kHz (the `--IQ 0.0` form), every channel carrying the same capture of that kind, fed one second a call, the capture repeated.

    device path   Engine.set_family: k_family_hits behind the frame sync; timed: fetch_family (300 bytes a hit) + FamilyDecoder.decoded per hit
    host path     the path as it was: timed: fetch_hits + fetch_soft (the hit's float soft bits) + FamilyDecoder.hit -> sonde_<kind>_dec_frame per hit

Both engines get the same samples in the same run, alternating call by call.  A call's samples are processed and the stream synchronised (Engine.sync) before the
timed region starts, so `fetch_decode_ms` is host time per second of signal with the device idle; `call_ms` is the whole call — process_host, the kernels (the
device path's k_family_hits among them), fetch and decode — under one clock.  Two warm-up passes over the capture, then calls until both paths have at least
--seconds of timed fetch + decode (and no fewer than --calls).  One decoder object per channel, the receivers' JSON options.  One JSON line per kind with medians,
minima and maxima per call, the hits and good frames of both paths (they must agree), the bytes copied per hit both ways and the device's clocks.

--gps-device (RS92 only): a third engine on the device path whose records go through family.rs92_text_batch with a gps.GpsSolver — the position solve's
4-satellite subset search of a call's hits in one launch; one row of kind "RS92_GPS" with all three paths, appended to --out (the stored rows stay).

    python tools/bench_family_hits.py [--gps-device] [--kinds MEISEI,IMET5,MTS01,RS92] [--channels 256] [--seconds 1.0] [--calls 12] [--out profiles/family_hits_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR = 48_000


def capture(kind, tmp):
    """-> (int16 IQ of a whole number of seconds, decoder keywords)"""
    from tools import synth, synth_rs92 as R
    if kind == "MEISEI":
        return synth.meisei_capture(sr=SR, seconds=6.0, noise_sigma=0.05, seed=1), {}
    if kind == "IMET5":
        return synth.imet54_capture(sr=SR, seconds=6.0, noise_sigma=0.05, seed=2), {}
    if kind == "MTS01":
        return synth.mts01_capture(sr=SR, seconds=6.0, noise_sigma=0.05, seed=3), {}
    eph = R.constellation()
    p = os.path.join(tmp, "brdc.nav")
    with open(p, "wb") as f:
        f.write(R.rinex_nav(eph))
    x = R.rs92_capture(R.flight(6, eph), sr=SR, noise_sigma=0.02, seed=4)
    return x[:2 * SR * (len(x) // 2 // SR)], dict(ephemeris=p)


def run_kind(kind, a, tmp, gps_path=False):
    import torch                                                                 # noqa: F401  (PyTorch's HIP runtime first)
    from bench import _device_clocks
    from radiosonde_auto_rx_amd.engine import Engine
    from radiosonde_auto_rx_amd.family import FAMILY, FamilyDecoder, rs92_text_batch
    f = FAMILY[kind]
    x, dkw = capture(kind, tmp)
    secs = len(x) // 2 // SR
    nch = a.channels
    blocks = [np.ascontiguousarray(np.broadcast_to(x[2 * SR * k:2 * SR * (k + 1)], (nch, 2 * SR))) for k in range(secs)]

    def engine(dev):
        e = Engine([0.0] * nch, SR, sonde="generic", generic=f["generic"], thres=f["thres"], auto=f["auto"], keep_soft=True, lp_iq=True, max_chunk=SR, max_frames=8 * nch)
        if dev:
            e.set_family(kind, ecc=f["kw"].get("ecc", 1))
        return e
    eng = {"device": engine(True), "host": engine(False)}
    solver = None
    if gps_path:
        from radiosonde_auto_rx_amd.gps import GpsSolver
        eng["device_gps"] = engine(True)
        solver = GpsSolver(max_jobs=max(nch, 64))
    dec = {p: [FamilyDecoder(kind, version="bench", **dkw) for _ in range(nch)] for p in eng}
    stat = {p: dict(fd=[], call=[], hits=0, json=0, undecoded=0) for p in eng}

    def one_call(p, k, timed):
        e, d, s = eng[p], dec[p], stat[p]
        t0 = time.perf_counter()
        e.process_host(blocks[k % secs])
        e.sync()
        t1 = time.perf_counter()
        recs = e.fetch_hits() if p == "host" else e.fetch_family()
        nj = 0
        texts = rs92_text_batch(d, recs, solver) if p == "device_gps" else [d[r["channel"]].decoded(r) if p == "device" else d[r["channel"]].hit(r) for r in recs]
        for text in texts:
            nj += text.count("\n{")  + text.startswith("{")
        t2 = time.perf_counter()
        if timed:
            s["fd"].append((t2 - t1) * 1e3); s["call"].append((t2 - t0) * 1e3); s["hits"] += len(recs); s["json"] += nj
            s["undecoded"] += sum(1 for r in recs if p == "device" and not r["decoded"])

    k = 0
    for _ in range(2 * secs):                                                    # warm-up: code objects, the first frames, the decoders' configuration cycles
        for p in eng:
            one_call(p, k, False)
        k += 1
    clocks0 = _device_clocks()
    while k < 2 * secs + 2000 and (k < 2 * secs + a.calls or min(sum(stat[p]["fd"]) for p in eng) < 1e3 * a.seconds):
        for p in (list(eng) if k & 1 else list(eng)[::-1]):                     # alternating: other people's work shares the box
            one_call(p, k, True)
        k += 1
    clocks1 = _device_clocks()
    ovf = {p: eng[p].overflowed() for p in eng}
    for p in eng:
        eng[p].close()
        for d in dec[p]:
            d.close()
    nb = f["generic"]["nbits"]
    row = {"kind": kind + "_GPS" if gps_path else kind, "channels": nch, "calls": len(stat["device"]["fd"]), "signal_s_per_call": 1.0}
    if solver is not None:
        row["gps"] = solver.stats()
        solver.close()
    for p in eng:
        s = stat[p]
        row[p] = {"fetch_decode_ms": round(statistics.median(s["fd"]), 3), "fetch_decode_min_ms": round(min(s["fd"]), 3), "fetch_decode_max_ms": round(max(s["fd"]), 3),
                  "fetch_decode_timed_s": round(sum(s["fd"]) / 1e3, 3), "call_ms": round(statistics.median(s["call"]), 3), "call_min_ms": round(min(s["call"]), 3),
                  "call_max_ms": round(max(s["call"]), 3), "hits": s["hits"], "json": s["json"], "overflowed": bool(ovf[p])}
    row["device"]["undecoded"] = stat["device"]["undecoded"]
    row["bytes_per_hit"] = {"device": 596 + 300, "host": 596 + 4 * nb,
                            "note": "596 = the engine's hit record, which both paths copy; device: + sonde_family_hit_t (300); host: + nbits float soft bits"}
    row["clocks_before"], row["clocks_after"] = clocks0, clocks1
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="MEISEI,IMET5,MTS01,RS92")
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=1.0, help="least timed fetch + decode time per path")
    ap.add_argument("--calls", type=int, default=12, help="least timed calls")
    ap.add_argument("--out", default="")
    ap.add_argument("--gps-device", action="store_true", help="RS92 alone, with a third path: rs92_text_batch and the device subset search")
    a = ap.parse_args()
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for kind in (["RS92"] if a.gps_device else a.kinds.split(",")):
            row = run_kind(kind, a, tmp, a.gps_device)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        if a.gps_device and os.path.exists(a.out):
            with open(a.out) as f:
                rows = [r for r in json.load(f) if r.get("kind") != "RS92_GPS"] + rows
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
