"""iMet-4 front-end sweep: the case table, the captures, and a float64 model of the chain k_imet4_decim and the front end of k_imet4_afsk compute.

The model is the chain as its defining sums, in float64 (numpy), from the RAW samples:
  IQ-dc removal in the reference's doubling blocks (exact block sums; the mean is the float32 the reference stores) -> mixer table ->
  decimating FIR at every decM-th sample -> rotation by Df (t = sample / IF rate) -> IF low-pass with the tap set in effect ->
  0.8 arg(z conj(z_-1)) / pi -> FM low-pass;  FM audio: sample / 32768 -> FM low-pass -> v - dc 0.4;
  then the AFC's running sum over the last M samples and the sliding two-tone DFT sums over the last floor(bitlen) samples, as plain windowed
  sums at requested samples.
Every constant is an INPUT: the float32 tap tables and the mixer table come from the reference harness (oracle/ref_imet4_harness.c), and so does
the schedule, per sample: Df, the tap set and dc in effect for it (the reference's two builds disagree on Df in the last digits, DESIGN 4.14;
the sweep judges the schedule separately).  literal() evaluates the same sums term by term at single samples.

Case = the shortest capture that reaches the branch: 1.15 s, one frame starting at 0.05 s (tools/synth.py, seeded): the header re-phases the
AFC schedule (pre_pos), and the first update under the new phase falls near 0.98 s.
  id          selects
  imet48      auto_rx's IMET form, 48 k, carrier +1.5 kHz: AFC update at sample 0 (tap-set switch) and behind the header, header inside a tile
  imet1_96    --imet1 at 96 k: doubled IF rate, 80 kHz IF low-pass
  imet48_u8   imet48 from 8-bit samples
  r2400       2.4 M --iq 0.1: k_imet4_decim, decM 50
  wav48       FM-audio WAV, 48 k, no options
  wav48_dc    FM-audio WAV with an audio offset, --dc --lpFM: v - dc 0.4, the FM low-pass on audio
"""
from __future__ import annotations

import functools

import numpy as np

import mk2a_front_cases as K

SECONDS = 1.15
T_FIRST = 0.05
IMET = dict(lp_iq=True, dc=True)

CASES = [
    dict(id="imet48", gen=dict(sr=48000, f_offset_hz=1500.0, seed=3), opt=dict(IMET)),
    dict(id="imet1_96", gen=dict(sr=96000, f_offset_hz=1500.0, seed=4, imet1=True), opt=dict(IMET, imet1=True)),
    dict(id="imet48_u8", gen=dict(sr=48000, f_offset_hz=1500.0, seed=3), bits=8, opt=dict(IMET)),
    dict(id="r2400", gen=dict(sr=2400000, fq=0.1, f_offset_hz=-1200.0, seed=5), fq=0.1, opt=dict(IMET)),
    dict(id="wav48", gen=dict(sr=48000, seed=6, audio=True), wav=True, opt=dict()),
    dict(id="wav48_dc", gen=dict(sr=48000, seed=7, audio=True, audio_dc=0.05), wav=True, opt=dict(dc=True, lp_fm=True)),
]
BY_ID = {c["id"]: c for c in CASES}
figure = K.figure


def sr_of(c):
    return c["gen"]["sr"]


def bits_of(c):
    return c.get("bits", 16)


@functools.lru_cache(maxsize=None)
def capture(cid: str, seed: int | None = None) -> np.ndarray:
    """the case's raw samples: interleaved int16 (or uint8) IQ, or mono int16 FM audio; read-only"""
    from tools import synth
    c = BY_ID[cid]
    g = dict(c["gen"])
    if seed is not None:
        g["seed"] = seed
    x = synth.imet4_capture(seconds=SECONDS, t_first=T_FIRST, **g)
    if bits_of(c) == 8:
        x = synth.to_u8(x)
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return x


def cli_input(cid: str):
    """(argument list without -r, stdin bytes or None, WAV bytes or None) of the compiled CLI for the case"""
    from tools import synth
    c = BY_ID[cid]
    o = c["opt"]
    tail = (["--lpIQ"] if o.get("lp_iq") else []) + (["--lpFM"] if o.get("lp_fm") else []) + (["--dc"] if o.get("dc") else []) + (["--imet1"] if o.get("imet1") else [])
    if c.get("wav"):
        return tail, None, synth.wav_bytes(capture(cid), sr_of(c))
    return ["--iq", repr(float(c.get("fq", 0.0)))] + tail + ["-", str(sr_of(c)), str(bits_of(c))], capture(cid).tobytes(), None


def engine_kw(c) -> dict:
    """keyword arguments of Imet4Engine"""
    o = c["opt"]
    return dict(bits=bits_of(c), iq=not c.get("wav"), lp_iq=bool(o.get("lp_iq")), lp_fm=bool(o.get("lp_fm")), dc=bool(o.get("dc")), imet1=bool(o.get("imet1")))


@functools.lru_cache(maxsize=None)
def reference(cid: str, libname: str = "libref_imet4_O2.so", seed: int | None = None) -> dict:
    """the compiled reference's run of the case (oracle/_ref/<libname>), computed once and shared read-only"""
    from oracle import ref_front
    from tools import synth
    c = BY_ID[cid]
    o = c["opt"]
    x = capture(cid, seed)
    kw = dict(lp_iq=bool(o.get("lp_iq")), lp_fm=bool(o.get("lp_fm")), dc=bool(o.get("dc")), imet1=bool(o.get("imet1")), libname=libname)
    if c.get("wav"):
        r = ref_front.ref_imet4_run(synth.wav_bytes(x, sr_of(c)), sr_of(c), wav=True, **kw)
    else:
        r = ref_front.ref_imet4_run(x, sr_of(c), bits=bits_of(c), fq=c.get("fq", 0.0), **kw)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def schedule_of(ref) -> dict:
    """per sample what is in effect for it: Df, nominal tap set, dc"""
    return dict(df=ref["df"], nominal=ref["nominal"].astype(bool), dc=ref["dc_of"])


def updates_of(ref) -> list:
    """the AFC update points of a --dc run: samples p with (p + pre_pos in effect for p) % IF rate == 0 (imet4iq.c:548)"""
    if not ref["dc"]:
        return []
    p = np.arange(ref["n"], dtype=np.int64)
    return [int(v) for v in np.flatnonzero((p + ref["pre_pos"].astype(np.int64)) % ref["consts"]["if_sr"] == 0)]


def changes_of(ref) -> list:
    """the samples behind which Df, dc or the tap set in effect differ"""
    ch = (np.diff(ref["df"]) != 0) | (np.diff(ref["dc_of"]) != 0) | (np.diff(ref["nominal"].astype(int)) != 0)
    return [int(v) for v in np.flatnonzero(ch)]


def headers_of(ref) -> list:
    """the samples at which main accepted a header (mv_pos = sample + 1 from the next sample on)"""
    ch = np.flatnonzero(np.diff(ref["mv_pos"].astype(np.int64)) != 0)
    return [int(p) for p in ch]


# ----------------------------------------------------------------------------------------------- the model
def front(cid, ref):
    """the part no AFC reaches -> float64 IF samples (IQ) or audio samples"""
    c = BY_ID[cid]
    k = ref["consts"]
    raw = capture(cid)
    if c.get("wav"):
        return np.asarray(raw, np.float64) / 32768.0                 # *b / 128.0, then / 256.0: exact
    x = K.samples_of(raw, bits_of(c))
    avg, _ = K.iqdc_mean(x, k["maxcnt0"], k["maxlim"])
    lut = ref["lut"].astype(np.complex128)
    z = (x - avg) * lut[np.arange(len(x)) % len(lut)]
    D = k["decM"]
    if D > 1:
        z = K._fir(z, ref["ws"]["dec"][:k["dectaps"]], D, D - 1)
    return z[:len(x) // D]


def model(y, ref, sched, n=None):
    """the chain behind front() under the per-sample schedule -> dict of float64 streams zrot, zlp, fm (the FM low-pass input), x"""
    k = ref["consts"]
    n = ref["n"] if n is None else n
    y = np.asarray(y[:n])
    out = dict(zrot=None, zlp=None, fm=None)
    if ref["iq"]:
        u = np.arange(n)
        zrot = y * np.exp(-2j * np.pi * np.mod((u / float(k["if_sr"])) * sched["df"][:n], 1.0)) if ref["dc"] else y
        if k["iq_taps"]:
            T = k["iq_taps"]
            z1, z0 = K._fir(zrot, ref["ws"]["iq1"][:T]), K._fir(zrot, ref["ws"]["iq0"][:T])
            zlp = np.where(sched["nominal"][:n], z1, z0)
            out["zrot"] = zrot
        else:
            zlp = zrot
        zp = np.concatenate([[0.0 + 0.0j], zlp[:-1]])
        v = 0.8 * np.arctan2(zlp.imag * zp.real - zlp.real * zp.imag, zlp.real * zp.real + zlp.imag * zp.imag) / np.pi
        out["zlp"] = zlp
    else:
        v = y
    if k["fm_taps"]:
        out["fm"] = v
        v = K._fir(v, ref["ws"]["fm"][:k["fm_taps"]])
    if ref["dc"] and not ref["iq"]:
        v = v - sched["dc"][:n] * 0.4
    out["x"] = v
    return out


def sums_at(x, ref, probes):
    """at each probe sample n: the AFC sum over the last M - 1 samples, and F1, F2 = sum over the last floor(bitlen) samples of x[k] exp(-i w t_k)"""
    k = ref["consts"]
    sr, M = float(k["if_sr"]), k["M"]
    lag = int(sr / 1200.0)
    xs, F1, F2 = [], [], []
    for n in probes:
        xs.append(float(np.sum(x[max(0, n - M + 2):n + 1])))        # + x[n] - x[n + 1 - M] per sample: M - 1 terms stay
        kk = np.arange(max(0, n - lag + 1), n + 1)
        t = kk / sr
        F1.append(complex(np.sum(x[kk] * np.exp(-1j * 2 * np.pi * 2200.0 * t))))
        F2.append(complex(np.sum(x[kk] * np.exp(-1j * 2 * np.pi * 1200.0 * t))))
    return np.array(xs), np.array(F1), np.array(F2)


def literal(cid, ref, sched, probes):
    """the same sums term by term at single samples -> dict(ifin, zrot, zlp, fm, x at probes)"""
    import math
    c = BY_ID[cid]
    k = ref["consts"]
    raw = capture(cid)
    memo = {}

    def cached(f):
        def g(i):
            if i < 0:
                return 0.0
            key = (f.__name__, i)
            if key not in memo:
                memo[key] = f(i)
            return memo[key]
        return g

    half = lambda name: ref["ws"][name][:len(ref["ws"][name]) // 2].astype(np.float64)     # noqa: E731
    wdec, wiq0, wiq1, wfm = half("dec"), half("iq0"), half("iq1"), half("fm")
    if c.get("wav"):
        @cached
        def ifin(t):
            return float(raw[t]) / 32768.0
    else:
        x = K.samples_of(raw, bits_of(c))
        means = []
        for first, m in K.iqdc_blocks(len(x), k["maxcnt0"], k["maxlim"]):
            sr_, si_ = 0.0, 0.0
            for v in x[first:first + m]:
                sr_ += v.real
                si_ += v.imag
            means.append((first + m, complex(np.float32(sr_ / float(np.float32(m))), np.float32(si_ / float(np.float32(m))))))
        lut = ref["lut"].astype(np.complex128)
        D = k["decM"]

        @cached
        def base(b):
            a = 0j
            for end, m in means:
                if b >= end:
                    a = m
            return (x[b] - a) * lut[b % len(lut)]

        @cached
        def ifin(t):
            if D == 1:
                return base(t)
            s = (t + 1) * D - 1
            return sum(wdec[len(wdec) - 1 - a] * base(s - a) for a in range(len(wdec)))

    @cached
    def zrot(u):
        if not ref["dc"]:
            return ifin(u)
        ph = math.fmod((u / float(k["if_sr"])) * float(sched["df"][u]), 1.0)
        return ifin(u) * complex(math.cos(2 * math.pi * ph), -math.sin(2 * math.pi * ph))

    @cached
    def zlp(u):
        if not k["iq_taps"]:
            return zrot(u)
        w = wiq1 if sched["nominal"][u] else wiq0
        return sum(w[len(w) - 1 - a] * zrot(u - a) for a in range(len(w)))

    @cached
    def fm(u):
        if not ref["iq"]:
            return ifin(u)
        z, p = complex(zlp(u)), complex(zlp(u - 1))
        return 0.8 * math.atan2(z.imag * p.real - z.real * p.imag, z.real * p.real + z.imag * p.imag) / math.pi

    def xs(u):
        v = sum(wfm[len(wfm) - 1 - a] * fm(u - a) for a in range(len(wfm))) if k["fm_taps"] else fm(u)
        return v - float(sched["dc"][u]) * 0.4 if (ref["dc"] and not ref["iq"]) else v

    P = [int(u) for u in probes]
    return dict(ifin=np.array([ifin(u) for u in P]), zrot=np.array([zrot(u) for u in P]), zlp=np.array([zlp(u) for u in P]),
                fm=np.array([fm(u) for u in P]), x=np.array([xs(u) for u in P]))
