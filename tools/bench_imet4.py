"""Throughput of the iMet-4 / iMet-1-RS engine (k_imet4_afsk): call wall time in ms per second of signal for 1, 64 and 1024 channels at 48 kHz
(the auto_rx IMET form: --iq 0.0 --lpIQ --dc) and at 96 kHz with --imet1.  Input already on the device (process_device); one call per 0.25 s
of signal, as the CLI makes them; each call waits for its kernel and the frame-count copy, so this is an upper bound of the GPU time.
Kernel times alone: run it under `rocprofv3 --kernel-trace --stats`.  Prints one JSON line per configuration.
--bits 32 feeds the same samples as float32; --idle-slots K releases K of the channels (sonde_imet4_release_channel), as a receiver's pool of
mostly unused slots has them.

    python tools/bench_imet4.py [--seconds 2] [--channels 1,64,1024] [--bits 32] [--idle-slots K]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--channels", default="1,64,1024")
    ap.add_argument("--bits", type=int, default=16, choices=(16, 32), help="32: the same samples as float32 (x / 32768)")
    ap.add_argument("--idle-slots", type=int, default=0, metavar="K", help="release the last K channels of every engine before the first call")
    a = ap.parse_args()
    import torch
    from radiosonde_auto_rx_amd.imet4 import Imet4Engine
    from tools import synth
    for sr, imet1 in ((48000, False), (96000, True)):
        one = synth.imet4_capture(sr, a.seconds + 0.5, imet1=imet1, f_offset_hz=1200.0, dev_hz=12000.0 if imet1 else 4000.0, seed=3)
        chunk = sr // 4
        for nch in [int(c) for c in a.channels.split(",")]:
            eng = Imet4Engine([0.0] * nch, sr, bits=a.bits, imet1=imet1, max_chunk=chunk)
            idle = min(a.idle_slots, nch)
            for c in range(nch - idle, nch):
                eng.release_channel(c)
            calls = int(a.seconds * sr) // chunk
            x = torch.from_numpy(np.ascontiguousarray(one[:2 * chunk * (calls + 1)])).to("cuda")
            if a.bits == 32:
                x = x.to(torch.float32) / 32768.0
            blocks = [x[2 * chunk * k:2 * chunk * (k + 1)].repeat(nch).contiguous() for k in range(calls + 1)]
            torch.cuda.synchronize()
            eng.process_device(blocks[0].data_ptr(), chunk)                  # warm-up (first call: module load)
            t0 = time.perf_counter()
            for k in range(1, calls + 1):
                eng.process_device(blocks[k].data_ptr(), chunk)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            nf = len(eng.fetch_frames())
            eng.close()
            sig = calls * chunk / sr
            wall = (t1 - t0) * 1e3
            print(json.dumps({"sr": sr, "imet1": imet1, "bits": a.bits, "channels": nch, "idle_slots": idle, "signal_s": sig, "call_ms_per_signal_s": round(wall / sig, 3),
                              "x_realtime_all_channels": round(nch * sig * 1e3 / wall, 1), "frames": nf}), flush=True)


if __name__ == "__main__":
    main()
