"""What RS(255,223) of the LMS6 / LMS-X hits of a generic engine costs the host, with the decoder on the host and on the device (third addendum):
two generic engines of --channels channels at 48 kHz with the LMS6 description (--lmsx: the LMS-X one), both with Engine.set_family (k_lms6_hits behind the frame
sync), every channel carrying the same capture (continuous blocks, one every 0.87 s; LMS-X: 1.0 s), fed one second a call, the capture repeated.

    rs_off   the path as it was: timed: fetch_family (348 bytes a hit) + FamilyDecoder.decoded per hit -> sonde_lms6_dec_block_bytes (RS(255,223) on the host,
             frame sync, CRC, text)
    rs_on    Engine.set_family(.., rs=True): k_lms6_rs behind k_lms6_hits; timed: fetch_family (348 + 120 bytes a hit) + FamilyDecoder.decoded per hit ->
             sonde_lms6_dec_block_rs (the RS result from the record; frame sync, CRC, text)

Both engines get the same samples in the same run, alternating call by call.  A call's samples are processed and the stream synchronised (Engine.sync) before the
timed region starts, so `fetch_text_ms` is host time per second of signal with the device idle; `call_ms` is the whole call — process_host, the kernels (rs_on:
k_lms6_rs among them), fetch and text — under one clock.  Two warm-up passes over the capture, then calls until both paths have at least --seconds of timed fetch +
text (and no fewer than --calls).  One decoder object per channel, the receivers' JSON options (--vit2).  One JSON line per channel count with medians, minima and
maxima per call, the hits and JSON objects of both paths (they must agree), the RS results taken from records and decoded on the host instead (the fallback: 0
expected) and the device's clocks.  No threshold: the numbers are what was measured.

    python tools/bench_lms6_rs.py [--channels 256,1024] [--seconds 1.0] [--calls 12] [--lmsx] [--out profiles/lms6_rs_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR = 48_000


def run(a, nch):
    import torch                                                                 # noqa: F401  (PyTorch's HIP runtime first)
    from bench import _device_clocks
    from tools import synth
    from radiosonde_auto_rx_amd.engine import Engine
    from radiosonde_auto_rx_amd.family import FAMILY, FamilyDecoder
    typ = "LMSX" if a.lmsx else "LMS6"
    f = FAMILY[typ]
    x = synth.lms6_capture(sr=SR, seconds=6.0, noise_sigma=0.05, seed=1, **(dict(lmsx=True, baud=4797.8) if a.lmsx else {}))
    secs = len(x) // 2 // SR
    blocks = [np.ascontiguousarray(np.broadcast_to(x[2 * SR * k:2 * SR * (k + 1)], (nch, 2 * SR))) for k in range(secs)]

    def engine(rs):
        e = Engine([0.0] * nch, SR, sonde="generic", generic=f["generic"], thres=f["thres"], auto=f["auto"], keep_soft=True, lp_iq=True, max_chunk=SR, max_frames=8 * nch)
        e.set_family(typ, vit=f["kw"]["vit"], rs=rs)
        return e
    eng = {"rs_on": engine(True), "rs_off": engine(False)}
    dec = {p: [FamilyDecoder("LMS6", version="bench", typ=10 if a.lmsx else 6) for _ in range(nch)] for p in eng}
    stat = {p: dict(ft=[], call=[], hits=0, ok=0, json=0, undecoded=0) for p in eng}

    def one_call(p, k, timed):
        e, d, s = eng[p], dec[p], stat[p]
        t0 = time.perf_counter()
        e.process_host(blocks[k % secs])
        e.sync()
        t1 = time.perf_counter()
        recs = e.fetch_family()
        nj = nok = 0
        for r in recs:
            text = d[r["channel"]].decoded(r)                                    # (a record of the rs_on engine carries its "rs")
            nj += text.count("\n{") + text.startswith("{")
            nok += "[OK]" in text
        t2 = time.perf_counter()
        if timed:
            s["ft"].append((t2 - t1) * 1e3); s["call"].append((t2 - t0) * 1e3); s["hits"] += len(recs); s["json"] += nj; s["ok"] += nok
            s["undecoded"] += sum(1 for r in recs if not r["decoded"])

    k = 0
    for _ in range(2 * secs):                                                    # warm-up: code objects, the first frames, the decoders' configuration cycles
        for p in eng:
            one_call(p, k, False)
        k += 1
    clocks0 = _device_clocks()
    while k < 2 * secs + 2000 and (k < 2 * secs + a.calls or min(sum(stat[p]["ft"]) for p in eng) < 1e3 * a.seconds):
        for p in (list(eng) if k & 1 else list(eng)[::-1]):                     # alternating: other people's work shares the box
            one_call(p, k, True)
        k += 1
    clocks1 = _device_clocks()
    ovf = {p: eng[p].overflowed() for p in eng}
    rs_stats = {p: [sum(v) for v in zip(*(d.lms_rs_stats() for d in dec[p]))] for p in eng}
    for p in eng:
        eng[p].close()
        for d in dec[p]:
            d.close()
    row = {"kind": typ, "channels": nch, "calls": len(stat["rs_on"]["ft"]), "signal_s_per_call": 1.0}
    for p in eng:
        s = stat[p]
        row[p] = {"fetch_text_ms": round(statistics.median(s["ft"]), 3), "fetch_text_min_ms": round(min(s["ft"]), 3), "fetch_text_max_ms": round(max(s["ft"]), 3),
                  "fetch_text_timed_s": round(sum(s["ft"]) / 1e3, 3), "call_ms": round(statistics.median(s["call"]), 3), "call_min_ms": round(min(s["call"]), 3),
                  "call_max_ms": round(max(s["call"]), 3), "hits": s["hits"], "ok": s["ok"], "json": s["json"], "undecoded": s["undecoded"], "overflowed": bool(ovf[p]),
                  "rs_used": rs_stats[p][0], "rs_missed": rs_stats[p][1]}
    u, m = rs_stats["rs_on"]
    row["host_fallback_share"] = round(m / (u + m), 6) if u + m else None         # (warm-up calls included: the decoders count from creation)
    row["bytes_per_hit"] = {"rs_on": 596 + 348 + 120, "rs_off": 596 + 348, "note": "596 = the engine's hit record; 348 = sonde_lms6_hit_t; 120 = sonde_lms6_rs_t"}
    row["clocks_before"], row["clocks_after"] = clocks0, clocks1
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="256,1024", help="channel counts, one row each")
    ap.add_argument("--seconds", type=float, default=1.0, help="least timed fetch + text time per path")
    ap.add_argument("--calls", type=int, default=12, help="least timed calls")
    ap.add_argument("--lmsx", action="store_true", help="the LMS-X description and capture: 4720 bits a hit at 4797.8 Bd")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    for nch in [int(c) for c in a.channels.split(",")]:
        row = run(a, nch)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        keep = []
        if os.path.exists(a.out):                                                # a row per type and channel count: the others stay
            with open(a.out) as f:
                keep = [r for r in json.load(f) if not any(r.get("kind") == n["kind"] and r.get("channels") == n["channels"] for n in rows)]
        with open(a.out, "w") as f:
            json.dump(keep + rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
