"""The Weathex WxR-301D captures of the goldens tests/golden/wxr_*.npz (tools/make_golden_wxr.py) and how to rebuild them.

Each case: gen = keyword arguments of tools.synth.wxr_capture plus
    "form": "cs16" | "cu8" (IQ through iq_dec), "wav16" | "wav8" | "wav32" | "wav2ch" (FM samples straight into weathex301d), "soft" (IQ
            through fsk_demod, soft bits into weathex301d --softin), "cut": IQ samples kept, and "split_runs": bit indices for split_runs();
front = the iq_dec (or fsk_demod) argument list of auto_rx in front of the decoder; argv = the weathex301d argument lists whose stdout and
stderr the golden holds."""
from __future__ import annotations

import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def iq_dec_args(sr=96000, bits=16, fq="0.0"):                # decode.py:784-834
    return ["--FM", "--IFbw", "64", "--lpFM", "--wav", "--iq", fq, "-", str(sr), str(bits)]


def fsk_args(sr=96000, baud=4800):                           # decode.py:1385-1471
    return ["--cs16", "-s", "-b", "-40000", "-u", "40000", "--mask", "50000", "--stats=5", "2", str(sr), str(baud), "-", "-"]


B = ["-b", "--json"]
PN = ["--pn9"]

CASES = {
    # auto_rx's own command lines on a clean capture, and every output form
    "clean": dict(gen=dict(seed=11), front=iq_dec_args(),
                  argv=[B, ["-b", "-r", "-v"], ["-R"], ["-b", "-t"], B + ["--jsn_cfq", "403000000"], ["--json"], ["-b", "-v", "--json"], ["-t", "-r"]]),
    "clean_pn9": dict(gen=dict(seed=12, pn9=True), front=iq_dec_args(),
                      argv=[B + PN, ["-b", "-r", "-v"] + PN, ["-R"] + PN, ["-b", "-t"] + PN, B + PN + ["--jsn_cfq", "403000000"], ["--json"] + PN, ["-v"] + PN]),
    # carrier off centre: the discriminator output sits on a DC level, the slicer's threshold does not follow
    "offm8k": dict(gen=dict(seed=13, f_offset_hz=-8000.0, noise=15.0), front=iq_dec_args(), argv=[B, ["--json"]]),
    "off12k_pn9": dict(gen=dict(seed=14, pn9=True, f_offset_hz=12000.0, noise=15.0), front=iq_dec_args(), argv=[B + PN, ["--json"] + PN]),
    # 4 dB in the 96 kHz band: frames with a wrong check, headers missed
    "noisy": dict(gen=dict(seed=15, noise=4.0), front=iq_dec_args(), argv=[["-b", "-r", "--json"], ["-r"], B]),
    "noisy_pn9": dict(gen=dict(seed=16, pn9=True, noise=4.0), front=iq_dec_args(), argv=[["-b", "-r", "--json"] + PN, ["-r"] + PN, B + PN]),
    "flips": dict(gen=dict(seed=17, noise=20.0, flips=12), front=iq_dec_args(), argv=[["-b", "-r", "-v"], B, ["--json"]]),
    "flips_pn9": dict(gen=dict(seed=18, pn9=True, noise=20.0, flips=12), front=iq_dec_args(), argv=[["-b", "-r", "-v"] + PN, B + PN]),
    # inverted deviation: nothing without -i
    "inv": dict(gen=dict(seed=19, invert=True), front=iq_dec_args(), argv=[B, B + ["-i"], ["--json", "-i"]]),
    # the stream ends inside a frame: -b prints it with the previous frame's tail, without -b only -t shows that a header was open
    "cut": dict(gen=dict(seed=20, cut=160000), front=iq_dec_args(), argv=[["-b", "-r"], ["-r"], ["-b", "-R"], ["-t", "-r"], ["-b", "-t", "--json"]]),
    "cut_pn9": dict(gen=dict(seed=21, pn9=True, cut=150000), front=iq_dec_args(), argv=[["-b", "-r"] + PN, ["-r", "-t"] + PN]),
    "u8": dict(gen=dict(seed=22, form="cu8", amp=24000.0), front=iq_dec_args(bits=8), argv=[B, ["-r"]]),
    # FM samples straight into the decoder: no float front end in between, the slicer alone
    "wav16": dict(gen=dict(seed=23, form="wav16"), front=None, argv=[B, ["-r", "-t"], ["-b", "-R"]]),
    "wav8": dict(gen=dict(seed=24, form="wav8", pn9=True), front=None, argv=[B + PN, ["-r"] + PN]),
    "wav32": dict(gen=dict(seed=25, form="wav32", noise=8.0), front=None, argv=[["-b", "-r", "-t"], ["-r"]]),
    "wav2ch": dict(gen=dict(seed=26, form="wav2ch"), front=None, argv=[B, ["--json"]]),
    # runs of 0 bits where the two FM slicers differ: three frames, and one sample of the other sign in the middle of a two-bit run (20, 1
    # and 19 samples: 1, 0 and 1 bits) in the payload of the first frame, in the header of the second (bits 28 and 29 of its 40) and in the
    # payload of the third.  weathex301d puts an 'x' into its header ring for the run of 0 bits, so the golden has frames 1 and 3 and not
    # frame 2, with and without -b; in a payload the 'x' changes nothing.
    "zero_runs": dict(gen=dict(seed=31, form="wav16", n_frames=3, lead_s=0.02, split_runs=[96 + 300, 648 + 96 + 24, 2 * 648 + 96 + 300]), front=None,
                      argv=[["-r"], ["-b", "-r"]]),
    # one 2.4 Msps stream with the signal at +240 kHz: IF 75 kHz, dec 32 (the one-stream receiver's test, tests/test_gpu_wxr.py)
    "wide_2400k": dict(gen=dict(sr=2400000, seed=27, fq=0.1, noise=15.0, n_frames=12), front=iq_dec_args(2400000, 16, "0.1"),
                       argv=[B + ["--jsn_cfq", "403240000"]]),
    "wide_2400k_pn9": dict(gen=dict(sr=2400000, seed=28, fq=0.1, noise=15.0, n_frames=12, pn9=True), front=iq_dec_args(2400000, 16, "0.1"),
                           argv=[B + PN + ["--jsn_cfq", "403240000"]]),
    # the soft-bit pipeline: the golden also holds the signs of the reference modem's soft bits
    "soft": dict(gen=dict(seed=29, form="soft", noise=20.0), front=fsk_args(96000, 4800), argv=[["--softin", "-i", "--json"], ["--softin", "--json"], ["--softin", "-i", "-r", "-t"]]),
    "soft_pn9": dict(gen=dict(sr=100000, seed=30, form="soft", noise=8.0, pn9=True), front=fsk_args(100000, 5000), argv=[["--softin", "-i", "--json", "--pn9"]]),
}

CLEAN = ["clean", "clean_pn9", "offm8k", "off12k_pn9", "u8", "wav16", "wav8", "wav2ch"]       # every frame put in comes out
BATCH = ["clean", "clean_pn9", "offm8k", "off12k_pn9", "noisy", "noisy_pn9", "flips", "flips_pn9", "inv", "cut", "cut_pn9"]     # 96 kHz cs16


def _fm(iq: np.ndarray) -> np.ndarray:
    """a plain discriminator with a 9-sample mean behind it, as float in about +-0.5: the FM samples of the WAV cases"""
    z = iq[0::2].astype(np.float64) + 1j * iq[1::2].astype(np.float64)
    s = np.concatenate([[0.0], np.angle(z[1:] * np.conj(z[:-1])) / np.pi])
    return np.convolve(s, np.ones(9) / 9.0, mode="same")


def split_runs(p: np.ndarray, bits: np.ndarray, spb: int, lead: int, at) -> np.ndarray:
    """p with one sample of the other sign in the middle of the first two-bit run of `bits` at or behind each bit index of `at` (bit k of
    the stream lies at lead + k * spb): the run falls into pieces of spb, 1 and spb - 1 samples, and the middle one rounds to 0 bits"""
    for k0 in at:
        k = next(k for k in range(k0, len(bits) - 2) if bits[k - 1] != bits[k] == bits[k + 1] != bits[k + 2])
        i = lead + (k + 1) * spb
        p[i] = -p[i] - (p[i] >= 0)
    return p


def capture(case) -> bytes:
    """stdin bytes of the first program of a case's pipeline"""
    from tools import synth
    g = dict(case["gen"])
    form, cut, splits = g.pop("form", "cs16"), g.pop("cut", None), g.pop("split_runs", None)
    g["corrupt"] = tuple(g.get("corrupt", ()))
    x = synth.wxr_capture(**g)
    sr = g.get("sr", 96000)
    if cut:
        x = x[:2 * cut]
    if form == "cu8":
        return synth.to_u8(x).tobytes()
    if form in ("cs16", "soft"):
        return x.astype("<i2").tobytes()
    s = _fm(x)
    if form == "wav16":
        p = np.round(s * 30000).astype(np.int16)
        if splits:                                                  # (4800 Bd, 12 bytes AA in front of every frame: wxr_capture's defaults)
            stream = b"".join(b"\xAA" * 12 + f for f in synth.wxr_frames(g["n_frames"])) + b"\xAA" * 12
            split_runs(p, np.unpackbits(np.frombuffer(stream, np.uint8)), sr // 4800, int(g["lead_s"] * sr), splits)
        return synth.wav_bytes(p, sr, 1, 16)
    if form == "wav8":
        return synth.wav_bytes(np.clip(np.round(s * 120) + 128, 0, 255).astype(np.uint8), sr, 1, 8)
    if form == "wav32":
        return synth.wav_bytes((s * 0.73).astype(np.float32), sr, 1, 32)
    if form == "wav2ch":                                        # the second channel carries something else: only the first is read
        p = np.round(s * 30000).astype(np.int16)
        return synth.wav_bytes(np.stack([p, -p[::-1]], axis=1).reshape(-1), sr, 2, 16)
    raise ValueError(form)


def frames_in(case) -> list:
    """the frames the generator put into a case's capture, as the bytes print_frame's -r shows (whitening removed)"""
    from tools import synth
    g = case["gen"]
    out = []
    for f in synth.wxr_frames(g.get("n_frames", 16), g.get("pn9", False)):
        b = bytearray(f)
        if g.get("pn9", False):
            for j in range(6, 69):
                b[j] ^= synth.WXR_PN9[(j - 6) % 64]
        out.append(bytes(b))
    return out


def load(name):
    z = np.load(os.path.join(GOLDEN, "wxr_%s.npz" % name))
    raw, ends = z["stdout"].tobytes(), np.cumsum(z["lengths"])
    err, eends = z["stderr"].tobytes(), np.cumsum(z["err_lengths"])
    return {"params": json.loads(str(z["params"])), "argv": [json.loads(str(a)) for a in z["argv"]],
            "front": json.loads(str(z["front"])), "front_stderr": z["front_stderr"].tobytes(),
            "stdout": [raw[e - n:e] for e, n in zip(ends, z["lengths"])],
            "stderr": [err[e - n:e] for e, n in zip(eends, z["err_lengths"])],
            "soft_sign": z["soft_sign"] if "soft_sign" in z.files else None}
