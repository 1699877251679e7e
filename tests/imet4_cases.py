"""The iMet-4 / iMet-1-RS captures of the goldens tests/golden/imet4_*.npz (tools/make_golden_imet4.py) and how to rebuild them.

Each case: gen = keyword arguments of tools.synth.imet4_capture (plus "form": "cs16" | "cu8" | "wav"), argv = the imet4iq argument lists
whose stdout the golden holds ("{wav}" stands for the WAV file of the capture)."""
from __future__ import annotations

import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
IMET = ["--iq", "0.0", "--lpIQ", "--dc", "-", "48000", "16"]          # auto_rx, decode.py:546-606

CASES = {
    # GPS / ePTU every second, an eGPS packet (frame 3), ozone XDATA on odd frames and a generic one on frame 4, a wrong GPS CRC (frame 5)
    "48k_off1500": dict(gen=dict(sr=48000, seconds=8.0, f_offset_hz=1500.0, seed=11, egps=[3], corrupt=[5], xdata="ozone+generic"),
                        argv=[IMET + ["--json"], IMET + ["--json", "--jsn_cfq", "402500000"], IMET + ["-r"], IMET + ["--rawbits"], IMET]),
    # the first AFC step is above 2 kHz: acquisition taps, then the nominal set
    "48k_offm2600": dict(gen=dict(sr=48000, seconds=7.0, f_offset_hz=-2600.0, seed=12),
                         argv=[IMET + ["--json"]]),
    # iMet-1-RS: 96 kHz IF, two packets per second, plain PTU.  A frame is 1000 bit decisions long and the packets are 600 bits apart, so
    # the reference's window swallows every second header: the golden holds every other frame (12:34:00, :02, ...), as the reference decodes it
    "96k_imet1": dict(gen=dict(sr=96000, seconds=6.0, imet1=True, dev_hz=12000.0, f_offset_hz=900.0, seed=13),
                      argv=[["--iq", "0.0", "--lpIQ", "--dc", "--imet1", "-", "96000", "16", "--json"]]),
    # carrier off centre: the mixer table
    "48k_fq": dict(gen=dict(sr=48000, seconds=5.0, fq=0.2, seed=14),
                   argv=[["--iq", "0.2", "--lpIQ", "--dc", "-", "48000", "16", "--json"], ["--iq", "0.2", "--lpIQ", "--lpFM", "-", "48000", "16"]]),
    "48k_u8": dict(gen=dict(sr=48000, seconds=5.0, f_offset_hz=700.0, seed=15, form="cu8"),
                   argv=[["--iq", "0.0", "--lpIQ", "--dc", "-", "48000", "8", "--json"]]),
    "48k_noisy": dict(gen=dict(sr=48000, seconds=6.0, f_offset_hz=-400.0, seed=16, noise_sigma=0.06, corrupt=[1, 2]),
                      argv=[IMET + ["--json"]]),
    # the stream ends inside a frame
    "48k_cut": dict(gen=dict(sr=48000, seconds=4.62, seed=17),
                    argv=[IMET + ["--json"]]),
    # decimating front end: 2.4 Msps, decM 50 (the decimator's own taps, IQ-dc blocks of base-rate samples, the mixer table at the base rate)
    "2400k_dec50": dict(gen=dict(sr=2400000, seconds=5.0, fq=0.1, f_offset_hz=-900.0, seed=19),
                        argv=[["--iq", "0.1", "--lpIQ", "--dc", "-", "2400000", "16", "--json"]]),
    # FM audio above 48 kHz: the FM low-pass is designed at the WAV rate (193 taps at 96 kHz)
    "audio_96k": dict(gen=dict(sr=96000, seconds=5.0, seed=20, audio=True, audio_dc=-0.03, form="wav"),
                      argv=[["--lpFM", "--dc", "--json", "{wav}"], ["--json", "{wav}"]]),
    # one 2.4 Msps stream with an iMet-4 at +300 kHz and an RS41 at -400 kHz (the one-stream receiver's test, tests/test_gpu_imet4.py)
    "wide_2400k": dict(gen=dict(sr=2400000, seconds=8.0, fq=0.125, seed=21, amp=0.3, form="wide"),
                       argv=[["--iq", "0.125", "--lpIQ", "--dc", "-", "2400000", "16", "--json", "--jsn_cfq", "403000000"]]),
    "audio_48k": dict(gen=dict(sr=48000, seconds=6.0, seed=18, audio=True, audio_dc=0.04, form="wav"),
                      argv=[["--json", "{wav}"], ["--dc", "--json", "{wav}"], ["--lpFM", "--dc", "{wav}"]]),
}


def _xdata(kind):
    if kind != "ozone+generic":
        return None
    return lambda k: ([bytes([0x01, 0x07, 0x00, 0x7B, 0x09, 0x60, 0x5A, 0x70])] if k % 2 else []) + \
                     ([bytes([0x19, 0x02, 0x33, 0x44])] if k in (1, 4) else [])


def capture(case):
    """-> (stdin bytes or None, WAV bytes or None) of a case"""
    from tools import synth
    g = dict(case["gen"])
    form = g.pop("form", "cs16")
    g["xdata"] = _xdata(g.get("xdata"))
    g["egps"] = set(g.get("egps", ()))
    g["corrupt"] = set(g.get("corrupt", ()))
    x = synth.imet4_capture(**g)
    if form == "wide":
        r = synth.rs41_capture(sr=g["sr"], seconds=g["seconds"], fq=-400000 / g["sr"], amp=0.3, seed=g["seed"] + 1, sonde_id="W1234567")
        x = np.clip(x.astype(np.int32) + r[:len(x)].astype(np.int32), -32768, 32767).astype(np.int16)
    if form == "wav":
        return None, synth.wav_bytes(x, g["sr"])
    if form == "cu8":
        return synth.to_u8(x).tobytes(), None
    return x.astype("<i2").tobytes(), None


def load(name):
    z = np.load(os.path.join(GOLDEN, "imet4_%s.npz" % name))
    raw, ends = z["stdout"].tobytes(), np.cumsum(z["lengths"])
    return {"params": json.loads(str(z["params"])), "argv": [json.loads(str(a)) for a in z["argv"]],
            "stdout": [raw[e - n:e] for e, n in zip(ends, z["lengths"])]}
