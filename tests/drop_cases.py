"""The RD94 / RD41 dropsonde captures of the goldens tests/golden/drop_*.npz (tools/make_golden_drop.py) and how to rebuild them.

Each case: gen = keyword arguments of tools.synth.drop_capture plus
    "form": "cs16" | "cu8" (IQ through iq_dec --bo 16), "wav16" | "wav8" | "wav32" | "wav2ch" (FM samples straight into rd94rd41drop),
            "soft" (IQ through fsk_demod, soft bits into rd94rd41drop --softin / --softinv), "rawhex" (the -r lines of another golden:
            "source" = its name, "index" = the argument list whose stdout is fed to --rawhex), "cut": IQ samples kept, and "split_runs": raw bit
            indices for tests/wxr_cases.py's split_runs();
front = the iq_dec (or fsk_demod) argument list in front of the decoder; argv = the rd94rd41drop argument lists whose stdout and stderr
the golden holds; rc = the exit code expected (0 when absent)."""
from __future__ import annotations

import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def iq_dec_args(sr=48000, bits=16, fq="0.0"):
    return ["--FM", "--lpFM", "--wav", "--bo", "16", "--iq", fq, "-", str(sr), str(bits)]


def fsk_args(sr=48000, baud=4800):                           # auto_rx decode.py:993-1034
    return ["--cs16", "-b", "-20000", "-u", "20000", "-s", "--stats=5", "2", str(sr), str(baud), "-", "-"]


J = ["--json"]
B = ["-b", "--json"]
FORMS = [J, B, ["-r"], ["-R"], ["-v"], ["-vv"], ["-b", "-vv", "--json"], J + ["--jsn_cfq", "403000000"]]
BAD41 = {1: [4], 2: [5], 3: [0, 1, 2], 5: [6], 6: [3]}        # text only, text only, mistyped RD94 (no text), no text, no text
BAD94 = {1: [3], 2: [0], 4: [2, 4], 6: [1]}                   # text only, no text, no text, no text

CASES = {
    # clean captures and every output form; forced to the right and to the wrong type
    "clean41": dict(gen=dict(seed=41, kind=41), front=iq_dec_args(), argv=FORMS + [["--rd41", "--json"], ["--rd94", "-v", "--json"], ["--rd94", "-R"]]),
    "clean94": dict(gen=dict(seed=42, kind=94, dev_hz=9600.0), front=iq_dec_args(), argv=FORMS + [["--rd94", "--json"], ["--rd41", "-v", "--json"], ["--rd41", "-R"]]),
    # inverted deviation: nothing without -i
    "inv41": dict(gen=dict(seed=43, kind=41, invert=True), front=iq_dec_args(), argv=[J, J + ["-i"], B + ["-i"]]),
    "inv94": dict(gen=dict(seed=44, kind=94, invert=True), front=iq_dec_args(), argv=[B, B + ["-i"]]),
    # carrier off centre: the discriminator output sits on a DC level, the slicer's threshold does not follow
    "off94": dict(gen=dict(seed=45, kind=94, f_offset_hz=1500.0, dev_hz=9600.0), front=iq_dec_args(), argv=[J, B, ["-r"]]),
    "off41": dict(gen=dict(seed=46, kind=41, f_offset_hz=-1200.0, dev_hz=9600.0), front=iq_dec_args(), argv=[J, B]),
    # 8 dB in the 48 kHz band: lost headers and bad blocks
    "noisy41": dict(gen=dict(seed=47, kind=41, noise=8.0), front=iq_dec_args(), argv=[["-b", "-R"], ["-r"], B, J, ["-vv", "--json"]]),
    "noisy94": dict(gen=dict(seed=48, kind=94, noise=8.0), front=iq_dec_args(), argv=[["-b", "-R"], ["-r"], B, J, ["-vv", "--json"]]),
    # flipped raw bits and frames with chosen blocks corrupted: text without JSON, no text, RD41 frames typed RD94
    "flips41": dict(gen=dict(seed=49, kind=41, flips=4, corrupt=BAD41), front=iq_dec_args(), argv=[["-vv", "--json"], ["-R"], ["-r"], ["-b", "-v", "--json"], ["--rd41", "-v"]]),
    "flips94": dict(gen=dict(seed=50, kind=94, flips=4, corrupt=BAD94), front=iq_dec_args(), argv=[["-vv", "--json"], ["-R"], ["-r"], ["-b", "-v", "--json"], ["--rd94", "-v"]]),
    # the stream ends inside a frame: -b prints it with the missing raw bits as '0', without -b it is not printed
    "cut41": dict(gen=dict(seed=51, kind=41, cut=100000), front=iq_dec_args(), argv=[["-b", "-r"], ["-r"], B, J, ["-b", "-R"]]),
    "cut94": dict(gen=dict(seed=52, kind=94, cut=131000), front=iq_dec_args(), argv=[["-b", "-r"], ["-r"], ["-b", "-v"]]),
    # --br: another bit length for the run lengths and the -b bit boundaries (the capture is sent at 4800, so -b drifts off the bits
    # towards the end of a frame); out of range it falls back to 4800 and still prints corr:
    "br94": dict(gen=dict(seed=53, kind=94), front=iq_dec_args(), argv=[["-b", "--br", "4798.8", "--json"], ["--br", "4798.8", "-r"], ["-b", "--br", "4790", "-r"], ["-b", "--br", "5000", "-r"]]),
    "u8": dict(gen=dict(seed=54, kind=41, form="cu8", amp=24000.0), front=iq_dec_args(bits=8), argv=[B, ["-r"]]),
    # FM samples straight into the decoder: no float front end in between, the slicer alone
    "wav16": dict(gen=dict(seed=55, kind=41, form="wav16"), front=None, argv=[B, J, ["-b", "-R"]]),
    "wav8": dict(gen=dict(seed=56, kind=94, form="wav8"), front=None, argv=[B, ["-r"]]),
    "wav2ch": dict(gen=dict(seed=57, kind=94, form="wav2ch"), front=None, argv=[B, J]),
    "wav32": dict(gen=dict(seed=58, kind=41, form="wav32"), front=None, argv=[B], rc=255),
    # runs of 0 bits where the two FM slicers differ: three frames, and one sample of the other sign in the middle of a two-bit run (10, 1
    # and 9 samples: 1, 0 and 1 raw bits) in the payload of the first frame, in the 40 header bits of the second and in the payload of the
    # third.  rd94rd41drop skips a run of 0 bits, so the golden has all three frames, with and without -b.
    "zero_runs": dict(gen=dict(seed=64, kind=41, form="wav16", n_frames=3, lead_s=0.02, split_runs=[40 + 540, 40 + 2400 + 8, 40 + 4800 + 540]), front=None,
                      argv=[["-r"], ["-b", "-r"]]),
    # one 2.4 Msps stream with the signal at +240 kHz: IF 48 kHz, dec 50 (the one-stream receiver's test; 4.8 kHz deviation, which the
    # detector's template answers with 0.98 — at 9.6 kHz the reference's dft_detect reports nothing)
    "wide41_2400k": dict(gen=dict(sr=2400000, seed=59, kind=41, fq=0.1, noise=15.0), front=iq_dec_args(2400000, 16, "0.1"),
                         argv=[B + ["--jsn_cfq", "403240000"]]),
    "wide94_2400k": dict(gen=dict(sr=2400000, seed=60, kind=94, fq=0.1, noise=15.0, invert=True), front=iq_dec_args(2400000, 16, "0.1"),
                         argv=[B + ["-i", "--jsn_cfq", "403240000"]]),
    # auto_rx's pipeline: the golden also holds the signs of the reference modem's soft bits
    "soft41": dict(gen=dict(seed=61, kind=41, form="soft"), front=fsk_args(), argv=[["--json", "--softinv"], ["--softin", "-i", "--json"], ["--softinv", "-r"], ["--softin", "--json"]]),
    "soft94": dict(gen=dict(seed=62, kind=94, form="soft", noise=8.0), front=fsk_args(), argv=[["--json", "--softinv"], ["--softinv", "-vv"]]),
    "softinv41": dict(gen=dict(seed=63, kind=41, form="soft", invert=True), front=fsk_args(), argv=[["--softinv", "-i", "--json"], ["--softin", "--json"], ["--softinv", "--json"]]),
    # the -r lines of a golden back in through --rawhex
    "rawhex": dict(gen=dict(form="rawhex", source="flips94", index=2), front=None, argv=[["--rawhex", "-vv", "--json"], ["--rawhex", "-R"], ["--rawhex", "--rd41", "-v"]]),
}

# every frame put in comes out (soft cases: all but the first, sent while the modem acquires); the argument list that shows it
CLEAN = {"clean41": 0, "clean94": 0, "off94": 0, "off41": 0, "u8": 0, "wav16": 0, "wav8": 0, "wav2ch": 0, "soft41": 0, "softinv41": 0,
         "inv41": 1, "inv94": 1, "wide41_2400k": 0, "wide94_2400k": 0}           # the inverted ones with -i / --softinv -i: the same counts
BATCH = ["clean41", "clean94", "inv41", "inv94", "off94", "off41", "noisy41", "noisy94", "flips41", "flips94", "cut41", "cut94", "br94"]     # 48 kHz cs16
N_FRAMES = 8


def _fm(iq: np.ndarray) -> np.ndarray:
    """a plain discriminator with a 5-sample mean behind it, as float in about +-0.4: the FM samples of the WAV cases"""
    z = iq[0::2].astype(np.float64) + 1j * iq[1::2].astype(np.float64)
    s = np.concatenate([[0.0], np.angle(z[1:] * np.conj(z[:-1])) / np.pi])
    return np.convolve(s, np.ones(5) / 5.0, mode="same")


def capture(case) -> bytes:
    """stdin bytes of the first program of a case's pipeline"""
    from tools import synth
    g = dict(case["gen"])
    form, cut, splits = g.pop("form", "cs16"), g.pop("cut", None), g.pop("split_runs", None)
    if form == "rawhex":
        src = load(g["source"])
        return src["stdout"][g["index"]]
    x = synth.drop_capture(**g)
    sr = g.get("sr", 48000)
    if cut:
        x = x[:2 * cut]
    if form == "cu8":
        return synth.to_u8(x).tobytes()
    if form in ("cs16", "soft"):
        return x.astype("<i2").tobytes()
    s = _fm(x)
    if form == "wav16":
        p = np.round(s * 60000).astype(np.int16)
        if splits:                                                  # (the raw bits as drop_capture sends them)
            from tests.wxr_cases import split_runs
            split_runs(p, synth.drop_rawbits([b"\x1A\xCF"] + frames_in(case)), sr // 4800, int(g["lead_s"] * sr), splits)
        return synth.wav_bytes(p, sr, 1, 16)
    if form == "wav8":
        return synth.wav_bytes(np.clip(np.round(s * 120) + 128, 0, 255).astype(np.uint8), sr, 1, 8)
    if form == "wav32":
        return synth.wav_bytes((s * 0.73).astype(np.float32), sr, 1, 32)
    if form == "wav2ch":                                        # the second channel carries something else: only the first is read
        p = np.round(s * 60000).astype(np.int16)
        return synth.wav_bytes(np.stack([p, -p[::-1]], axis=1).reshape(-1), sr, 2, 16)
    raise ValueError(form)


def frames_in(case) -> list:
    """the frames the generator put into a case's capture (120 bytes each)"""
    from tools import synth
    g = case["gen"]
    return synth.drop_frames(g.get("n_frames", N_FRAMES), g["kind"], corrupt=g.get("corrupt"))


def load(name):
    z = np.load(os.path.join(GOLDEN, "drop_%s.npz" % name))
    raw, ends = z["stdout"].tobytes(), np.cumsum(z["lengths"])
    err, eends = z["stderr"].tobytes(), np.cumsum(z["err_lengths"])
    return {"params": json.loads(str(z["params"])), "argv": [json.loads(str(a)) for a in z["argv"]],
            "front": json.loads(str(z["front"])), "front_stderr": z["front_stderr"].tobytes(),
            "stdout": [raw[e - n:e] for e, n in zip(ends, z["lengths"])],
            "stderr": [err[e - n:e] for e, n in zip(eends, z["err_lengths"])],
            "rc": [int(v) for v in z["rc"]],
            "soft_sign": z["soft_sign"] if "soft_sign" in z.files else None}
