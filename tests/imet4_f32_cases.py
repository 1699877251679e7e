"""The float32 iMet-4 captures of the goldens tests/golden/imet4f32_*.npz (tools/make_golden_imet4_f32.py) and how to rebuild them.

Each case: gen = keyword arguments of tools.synth.imet4_capture (plus "form": "cf32" | "wav"), eng = the Imet4Engine keywords that are the
argv's front-end options, argv = the imet4iq argument lists whose stdout the golden holds ("{wav}" stands for the WAV file of the capture).
Every capture goes through synth.to_f32: int16 samples times 0.73 / 32768, values an int16 stream cannot carry."""
from __future__ import annotations

import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _iq(fq, sr):
    return ["--iq", repr(fq), "--lpIQ", "--dc", "-", str(sr), "32"]


IQ_ENG = dict(iq=True, lp_iq=True, dc=True)

CASES = {
    # the auto_rx IMET form on float32: text, JSON, -r, --rawbits; an eGPS packet, XDATA, a wrong GPS CRC
    "48k_off1500": dict(gen=dict(sr=48000, seconds=6.0, f_offset_hz=1500.0, seed=31, egps=[3], corrupt=[4], xdata="ozone+generic"),
                        eng=dict(IQ_ENG, fq=0.0), argv=[_iq(0.0, 48000) + ["--json"], _iq(0.0, 48000) + ["-r"], _iq(0.0, 48000) + ["--rawbits"]]),
    # the channelizer's rate: 48000 does not divide it, so the IF rate is 50000 and decM 1
    "50k_fq014": dict(gen=dict(sr=50000, seconds=5.0, fq=0.14, f_offset_hz=800.0, seed=32),
                      eng=dict(IQ_ENG, fq=0.14), argv=[_iq(0.14, 50000) + ["--json"]]),
    # a second one at that rate (the run-time channel test hands a used slot to it)
    "50k_fqm010": dict(gen=dict(sr=50000, seconds=4.4, fq=-0.1, f_offset_hz=-500.0, seed=36),
                       eng=dict(IQ_ENG, fq=-0.1), argv=[_iq(-0.1, 50000) + ["--json"]]),
    # IF 50000, decM 2: the decimating front end on float32
    "100k_fqm007": dict(gen=dict(sr=100000, seconds=5.0, fq=-0.07, f_offset_hz=-900.0, seed=33),
                        eng=dict(IQ_ENG, fq=-0.07), argv=[_iq(-0.07, 100000) + ["--json"]]),
    "48k_noisy": dict(gen=dict(sr=48000, seconds=6.0, f_offset_hz=-400.0, seed=34, noise_sigma=0.06, corrupt=[1, 2]),
                      eng=dict(IQ_ENG, fq=0.0), argv=[_iq(0.0, 48000) + ["--json"]]),
    # the stream ends inside a frame
    "48k_cut": dict(gen=dict(sr=48000, seconds=4.62, seed=35),
                    eng=dict(IQ_ENG, fq=0.0), argv=[_iq(0.0, 48000) + ["--json"]]),
    # float32 mono WAV of FM audio
    "audio_48k": dict(gen=dict(sr=48000, seconds=6.0, seed=38, audio=True, audio_dc=0.04, form="wav"),
                      eng=dict(iq=False, lp_iq=False, dc=True, lp_fm=True, fq=0.0), argv=[["--dc", "--lpFM", "--json", "{wav}"]]),
}

# two more 50 kHz captures without a golden: the neighbours of the slot that is handed out in the run-time channel test
NEIGHBOURS = [dict(sr=50000, seconds=11.0, fq=0.05, f_offset_hz=300.0, seed=41), dict(sr=50000, seconds=11.0, fq=-0.2, f_offset_hz=-1100.0, seed=42)]


def _xdata(kind):
    if kind != "ozone+generic":
        return None
    return lambda k: ([bytes([0x01, 0x07, 0x00, 0x7B, 0x09, 0x60, 0x5A, 0x70])] if k % 2 else []) + \
                     ([bytes([0x19, 0x02, 0x33, 0x44])] if k in (1, 4) else [])


def samples(gen) -> np.ndarray:
    """the float32 samples of a gen record (interleaved IQ, or mono FM audio)"""
    from tools import synth
    g = dict(gen)
    g.pop("form", None)
    g["xdata"] = _xdata(g.get("xdata"))
    g["egps"] = set(g.get("egps", ()))
    g["corrupt"] = set(g.get("corrupt", ()))
    return synth.to_f32(synth.imet4_capture(**g))


def capture(case):
    """-> (float32 samples, stdin bytes or None, WAV bytes or None) of a case"""
    from tools import synth
    x = samples(case["gen"])
    if case["gen"].get("form") == "wav":
        return x, None, synth.wav_bytes(x, case["gen"]["sr"], bits=32)
    return x, x.astype("<f4").tobytes(), None


def printer_kw(argv):
    return dict(json="--json" in argv, raw="-r" in argv, rawbits="--rawbits" in argv)


def load(name):
    z = np.load(os.path.join(GOLDEN, "imet4f32_%s.npz" % name))
    raw, ends = z["stdout"].tobytes(), np.cumsum(z["lengths"])
    return {"params": json.loads(str(z["params"])), "argv": [json.loads(str(a)) for a in z["argv"]],
            "stdout": [raw[e - n:e] for e, n in zip(ends, z["lengths"])]}
