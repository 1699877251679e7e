"""The float32 dropsonde captures of the goldens tests/golden/dropf32_*.npz (tools/make_golden_drop_f32.py) and how to rebuild them.

Each case: gen = keyword arguments of tools.synth.drop_capture plus
    "scale": the factor of synth.to_f32 (int16 / 32768 times it; 0.73 when absent: values an int16 stream cannot carry),
    "dc": (re, im) added to every float32 sample, "cut": IQ samples kept;
fq = iq_dec's --iq; argv = the rd94rd41drop argument lists whose stdout and stderr the golden holds.  The pipeline of a case is
    iq_dec --FM --lpFM --wav --bo 16 --iq <fq> - <sr> 32 | rd94rd41drop <argv>
Every capture is at 48 or 50 kHz and at most 2 s long (three frames of half a second and 0.2 s of noise at either end)."""
from __future__ import annotations

import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

B = ["-b", "--json"]
BI = ["-b", "--json", "-i"]
G = dict(n_frames=3, lead_s=0.2)
BAD41 = {1: [4], 2: [0, 1, 2]}                                # text only; a mistyped RD94: no text
BAD94 = {0: [3], 2: [2, 4]}                                   # text only; no text

CASES = {
    "50k_94_fq014": dict(gen=dict(G, sr=50000, seed=71, kind=94, fq=0.014), fq=0.014, argv=[B]),
    "50k_41_fqm010": dict(gen=dict(G, sr=50000, seed=72, kind=41, fq=-0.010, f_offset_hz=300.0), fq=-0.010, argv=[B, ["-b", "-r"]]),
    "48k_41": dict(gen=dict(G, sr=48000, seed=73, kind=41), fq=0.0, argv=[B]),
    "48k_94": dict(gen=dict(G, sr=48000, seed=74, kind=94, f_offset_hz=-400.0), fq=0.0, argv=[B]),
    # inverted deviation: nothing without -i
    "50k_inv41": dict(gen=dict(G, sr=50000, seed=75, kind=41, invert=True, fq=0.014), fq=0.014, argv=[B, BI]),
    "48k_inv94": dict(gen=dict(G, sr=48000, seed=76, kind=94, invert=True), fq=0.0, argv=[B, BI]),
    # 8 dB in the 48 kHz band
    "50k_noisy41": dict(gen=dict(G, sr=50000, seed=77, kind=41, noise=8.0, fq=-0.010), fq=-0.010, argv=[B, ["-b", "-R"]]),
    "48k_noisy94": dict(gen=dict(G, sr=48000, seed=78, kind=94, noise=8.0), fq=0.0, argv=[B]),
    # flipped raw bits and frames with chosen blocks bad: text without JSON, no text
    "50k_flips41": dict(gen=dict(G, sr=50000, seed=79, kind=41, flips=4, corrupt=BAD41, fq=0.014), fq=0.014, argv=[["-b", "-v", "--json"], ["-b", "-r"]]),
    "48k_flips94": dict(gen=dict(G, sr=48000, seed=80, kind=94, flips=4, corrupt=BAD94), fq=0.0, argv=[["-b", "-v", "--json"], ["-b", "-r"]]),
    # the stream ends inside the third frame: -b prints it with the missing raw bits as '0'
    "50k_cut94": dict(gen=dict(G, sr=50000, seed=81, kind=94, fq=-0.010, cut=70000), fq=-0.010, argv=[["-b", "-r"], B]),
    "48k_cut41": dict(gen=dict(G, sr=48000, seed=82, kind=41, cut=66000), fq=0.0, argv=[["-b", "-r"], B]),
    # sample values above 1.0: the discriminator does not care about the amplitude, an int16 stream cannot carry them
    "50k_big41": dict(gen=dict(G, sr=50000, seed=83, kind=41, fq=0.014, amp=12000.0, scale=3.7), fq=0.014, argv=[B]),
    # a DC offset, so that every new IQ-dc average moves the samples (the wave emulator's capture: its first half second)
    "50k_dc94": dict(gen=dict(G, sr=50000, seed=84, kind=94, fq=0.013, dc=[0.05, -0.03]), fq=0.013, argv=[B]),
}

# the narrowband captures tests/test_gpu_chan_drop.py places into its wide stream (there generated at the stream's rate with the same frames): eight frames
# at 4.8 kHz of deviation, 1.5 kHz off the carrier.  Goldens like the others (dropf32_<name>.npz); not bound to 2 s
WIDE = {
    "wide94": dict(gen=dict(sr=50000, seed=85, kind=94, n_frames=8, f_offset_hz=1500.0), fq=0.0, argv=[B]),
    "wide_inv41": dict(gen=dict(sr=50000, seed=86, kind=41, n_frames=8, f_offset_hz=1500.0, invert=True), fq=0.0, argv=[BI]),
}

# the wave emulator's runs (tests/test_fm_front_emu.py): the first EMU_N samples of 50k_dc94 at two --iq; the golden dropf32_emu.npz holds iq_dec's int16 output
EMU_CASE, EMU_N, EMU_FQ = "50k_dc94", 25000, (0.013, -0.021)


def iq_dec_args(sr, fq):
    return ["--FM", "--lpFM", "--wav", "--bo", "16", "--iq", repr(float(fq)), "-", str(sr), "32"]


def samples(gen) -> np.ndarray:
    """the float32 samples of a gen record (interleaved IQ)"""
    from tools import synth
    g = dict(gen)
    scale, dc, cut = g.pop("scale", 0.73), g.pop("dc", None), g.pop("cut", None)
    if g.get("corrupt"):
        g["corrupt"] = {int(k): v for k, v in g["corrupt"].items()}
    x = synth.to_f32(synth.drop_capture(**g), scale)
    if cut:
        x = x[:2 * cut]
    if dc:
        x = (x.reshape(-1, 2) + np.array(dc, np.float32)).astype(np.float32).reshape(-1)
    return np.ascontiguousarray(x, np.float32)


def frames_in(case) -> list:
    """the frames the generator put into a case's capture (120 bytes each)"""
    from tools import synth
    g = case["gen"]
    return synth.drop_frames(g["n_frames"], g["kind"], corrupt=g.get("corrupt"))


def printer_kw(argv):
    a = list(argv)
    return dict(json="--json" in a, raw=2 if "-R" in a else 1 if "-r" in a else 0, vbs=2 if "-vv" in a else 1 if "-v" in a else 0)


def load(name):
    z = np.load(os.path.join(GOLDEN, "dropf32_%s.npz" % name))
    raw, ends = z["stdout"].tobytes(), np.cumsum(z["lengths"])
    err, eends = z["stderr"].tobytes(), np.cumsum(z["err_lengths"])
    return {"params": json.loads(str(z["params"])), "fq": float(z["fq"]), "argv": [json.loads(str(a)) for a in z["argv"]],
            "stdout": [raw[e - n:e] for e, n in zip(ends, z["lengths"])],
            "stderr": [err[e - n:e] for e, n in zip(eends, z["err_lengths"])],
            "rc": [int(v) for v in z["rc"]]}


def load_emu():
    """{fq: iq_dec's int16 FM samples on the emulator's capture}"""
    z = np.load(os.path.join(GOLDEN, "dropf32_emu.npz"))
    return {float(f): z["fm_%d" % i] for i, f in enumerate(z["fq"])}
