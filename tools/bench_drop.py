"""Throughput of the two GPU forms of the RD94 / RD41 dropsonde decoder at 48 kHz:
 - "iq":   the engine's IQ form (the iq_dec front end + k_drop_slice: iq_dec --FM --lpFM --wav --bo 16 --iq 0.0 | rd94rd41drop -b);
 - "soft": auto_rx's production pipe on the device (the 2-FSK modem at 4800 Bd + k_softin_drop: fsk_demod ... | rd94rd41drop --softinv).
Per second of signal, the call wall time (input already on the device; one call per 0.25 s of signal; each call waits for its kernels and
the frame-count copy, so this is an upper bound of the GPU time).  The kernel time alone comes from a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/bench_drop.py --channels 1024 --repeat 1`.  A warm-up call precedes the timed ones; the
timed region is repeated --repeat times with fresh engines, and the median and the spread are reported.  Prints one JSON line per form and
channel count and writes them to --out.

The single-core time of the reference's `iq_dec | rd94rd41drop` on such a capture is measured where the goldens are made
(tools/make_golden_drop.py prints it: one run, not a benchmark); it is passed in with --ref-seconds-per-signal-s only to be quoted next to
the result.

--bits 32 times the IQ form on float32 (the int16 capture / 32768: k_fm_front + k_drop_slice_rt, the engine of the channelized receiver);
--idle-slots K releases the last K channels of that engine before the first call, as a pool with free slots runs.

    python tools/bench_drop.py [--seconds 2] [--channels 1,64,1024] [--forms iq,soft] [--bits 16|32] [--idle-slots K] [--out profiles/drop_bench.json]"""
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
    ap.add_argument("--forms", default="iq,soft")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--bits", type=int, default=16, choices=(16, 32), help="IQ form: int16, or float32 (the engine with run-time channels)")
    ap.add_argument("--idle-slots", type=int, default=0, help="with --bits 32: that many channels are released before the first call")
    ap.add_argument("--ref-seconds-per-signal-s", type=float, default=0.0)
    a = ap.parse_args()
    if a.idle_slots and a.bits != 32:
        ap.error("--idle-slots needs --bits 32 (the engine whose channels are handed out at run time)")
    import torch
    from radiosonde_auto_rx_amd.drop import DropEngine
    from radiosonde_auto_rx_amd.fsk import FskModem, SoftinDev
    from tools import synth
    sr = 48000
    chunk = sr // 4
    calls = int(a.seconds * sr) // chunk
    one = synth.drop_capture(sr, n_frames=int((calls + 1) * chunk / sr / 0.5) + 2, kind=41, f_offset_hz=500.0, noise=15.0, seed=3, lead_s=0.05)
    rows = []
    for form in a.forms.split(","):
        for nch in [int(c) for c in a.channels.split(",")]:
            if form == "iq" and a.bits == 32:
                x = torch.from_numpy(np.ascontiguousarray(one[:2 * chunk * (calls + 1)]).astype(np.float32) / np.float32(32768.0)).to("cuda")
            else:
                x = torch.from_numpy(np.ascontiguousarray(one[:2 * chunk * (calls + 1)])).to("cuda")
            blocks = [x[2 * chunk * k:2 * chunk * (k + 1)].repeat(nch).contiguous() for k in range(calls + 1)]
            torch.cuda.synchronize()
            walls, nf = [], 0
            for _ in range(a.repeat):
                if form == "iq":
                    eng = DropEngine([0.0] * nch, sr, bits=a.bits, opt_b=True, max_chunk=chunk)
                    for c in range(max(0, nch - a.idle_slots), nch if a.idle_slots else 0):
                        eng.release_channel(c)
                    step = lambda k: eng.process_device(blocks[k].data_ptr(), chunk)
                else:
                    md = FskModem(sr, 4800, n_channels=nch, P=10, nsym=50, lower=-20000, upper=20000, max_chunk=chunk)
                    sf = SoftinDev(nch, kind="drop", softinv=True, inv=False)

                    def step(k):
                        md.process_device(blocks[k].data_ptr(), chunk, chunk)
                        sf.push_fsk(md)
                step(0)                                                          # warm-up (first call: module load)
                t0 = time.perf_counter()
                for k in range(1, calls + 1):
                    step(k)
                walls.append((time.perf_counter() - t0) * 1e3)
                if form == "iq":
                    nf = len(eng.fetch_frames())
                    eng.close()
                else:
                    nf = len(sf.fetch_drop(4 * nch * (calls + 1) + 16))
                    md.close(); sf.close()
            sig = calls * chunk / sr
            wall = statistics.median(walls)
            f32 = {"bits": a.bits, "idle_slots": min(a.idle_slots, nch)} if form == "iq" and a.bits == 32 else {}     # (the default run's rows keep their keys)
            row = {"form": form, "sr": sr, "channels": nch, **f32, "signal_s": sig, "call_ms_per_signal_s": round(wall / sig, 3),
                   "min_ms_per_signal_s": round(min(walls) / sig, 3), "max_ms_per_signal_s": round(max(walls) / sig, 3), "repeat": a.repeat,
                   "x_realtime_all_channels": round(sig * 1e3 / wall, 2), "channel_seconds_per_second": round(nch * sig * 1e3 / wall, 1),
                   "frames": nf}
            if a.ref_seconds_per_signal_s > 0 and form == "iq":
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
