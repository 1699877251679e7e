"""MkIIa front-end sweep: the case table, the captures, and a float64 model of the chain k_mk2a_mix and the produce() part of k_mk2a compute.

The model is the chain as its defining sums, in float64 (numpy), from the RAW samples:
  IQ-dc removal in the reference's doubling blocks (block sums of multiples of 2^-15 / 2^-7: exact in float64; the mean is the float32 the
  reference stores) -> mixer table -> decimating FIR at every decM-th sample -> rotation by Df (t = sample / IF rate) -> IF low-pass with
  the tap set in effect -> 0.8 arg(z conj(z_-1)) / pi -> windowed two-tone correlator (--IQ) -> FM and IQFM low-pass at the decFM points.
Every constant is an INPUT: the float32 tap tables, the mixer table and the tone phasors come from the reference harness
(oracle/ref_mk2a_harness.c), and so does the schedule [(first IF sample, Df, nominal tap set)] — the reference's own two builds disagree on
Df by tenths of a hertz after three AFC steps, which would swamp everything behind a step; the sweep judges the schedule
separately.  literal() evaluates the same sums term by term at single samples; tests/test_mk2a_front_cases.py holds model() to it (1e-12),
to the compiled reference, and the table below to what each row claims, without a GPU.

Case = the shortest capture that reaches the branch: 0.45 s (at least 3 correlation windows, one complete frame), a frame starting near
0.06 s (60 fill bytes), tools/synth.py generators, seeded.
  id            selects
  auto240       auto_rx's form at 240 k, carrier +30 kHz: decM 1, acquisition tap set, unlock -> lock, an AFC step per header
  auto240_u8    the same from 8-bit samples: cu8 conversion, IQ-dc means in steps of 2^-7 / block
  r960          960 k --iq 0.02: decM 5, the base-rate ring, the mixer table off centre
  r960min       ... --min: decM 6
  r2400         2.4 M --iq 0.1: decM 12
  IQ240         --IQ 0.0 --decFM --dc: tone correlator, IQFM low-pass, FM low-pass for the dc, second correlation while unlocked
  lpfm240       --iq 0.0 --lpIQ --lpbw 160 --lpFM: decFM 1 (output rate = IF rate, K = 6866), no AFC
  decfm2        auto_rx's form with --decFM2: the other decFM
  zeros8        8-bit digital silence (0x80) for 0.02 s, then auto240_u8's signal: zero history, atan2(+-0, +-0); reference comparison only
"""
from __future__ import annotations

import functools

import numpy as np

SECONDS = 0.45
AUTO = dict(opt_iq=6, lp_iq=True, lpbw_hz=160000, dec_fm=4, dc=True)

CASES = [
    dict(id="auto240", gen=dict(sr=240000, f_offset_hz=30000.0, seed=5), opt=dict(AUTO)),
    dict(id="auto240_u8", gen=dict(sr=240000, f_offset_hz=30000.0, seed=5), bits=8, opt=dict(AUTO)),
    dict(id="r960", gen=dict(sr=960000, fq=0.02, f_offset_hz=2000.0, seed=6), fq=0.02, opt=dict(AUTO)),
    dict(id="r960min", gen=dict(sr=960000, fq=0.02, f_offset_hz=2000.0, seed=6), fq=0.02, opt=dict(AUTO, opt_min=True)),
    dict(id="r2400", gen=dict(sr=2400000, fq=0.1, f_offset_hz=-3000.0, seed=7), fq=0.1, opt=dict(AUTO)),
    dict(id="IQ240", gen=dict(sr=240000, f_offset_hz=5000.0, seed=8), opt=dict(opt_iq=5, lp_iq=False, dec_fm=4, dc=True)),
    dict(id="lpfm240", gen=dict(sr=240000, seed=9), opt=dict(opt_iq=6, lp_iq=True, lpbw_hz=160000, lp_fm=True, dec_fm=0, dc=False)),
    dict(id="decfm2", gen=dict(sr=240000, f_offset_hz=30000.0, seed=10), opt=dict(AUTO, dec_fm=2)),
    dict(id="zeros8", gen=dict(sr=240000, f_offset_hz=30000.0, seed=5), bits=8, silence=4800, opt=dict(AUTO), model=False),
]
BY_ID = {c["id"]: c for c in CASES}
DC_ROWS = [c["id"] for c in CASES if c["opt"]["dc"]]


def sr_of(c):
    return c["gen"]["sr"]


def bits_of(c):
    return c.get("bits", 16)


@functools.lru_cache(maxsize=None)
def capture(cid: str, seed: int | None = None) -> np.ndarray:
    """the case's raw samples: interleaved int16 (or uint8) IQ, read-only"""
    from tools import synth
    c = BY_ID[cid]
    g = dict(c["gen"])
    if seed is not None:
        g["seed"] = seed
    x = synth.mk2a_capture(seconds=SECONDS, **g)
    if bits_of(c) == 8:
        x = synth.to_u8(x)
        if c.get("silence"):
            x = np.concatenate([np.full(2 * c["silence"], 128, np.uint8), x[:len(x) - 2 * c["silence"]]])
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return x


def cli_argv(c) -> list:
    """the mk2a1680mod argument list of the case (without -r / -v)"""
    o = c["opt"]
    a = ["--IQ" if o["opt_iq"] == 5 else "--iq", repr(float(c.get("fq", 0.0)))]
    if o.get("lp_iq"):
        a += ["--lpIQ"]
    if o.get("lpbw_hz"):
        a += ["--lpbw", str(o["lpbw_hz"] // 1000)]
    if o.get("lp_fm"):
        a += ["--lpFM"]
    a += {0: [], 4: ["--decFM"], 2: ["--decFM2"], 1: ["--decFM1"]}[o.get("dec_fm", 0)]
    if o.get("dc"):
        a += ["--dc"]
    if o.get("opt_min"):
        a += ["--min"]
    return a + ["-", str(sr_of(c)), str(bits_of(c))]


def ref_kw(c) -> dict:
    """keyword arguments of oracle.ref_front.ref_mk2a_run"""
    return dict(bits=bits_of(c), fq=c.get("fq", 0.0), **c["opt"])


def engine_kw(c) -> dict:
    """keyword arguments of Mk2aEngine"""
    o = c["opt"]
    return dict(bits=bits_of(c), opt_iq=o["opt_iq"], lp_iq=bool(o.get("lp_iq")), lpbw_hz=o.get("lpbw_hz", 0), lp_fm=bool(o.get("lp_fm")), dec_fm=o.get("dec_fm", 0),
                dc=bool(o.get("dc")), min=bool(o.get("opt_min")))


def schedule_of(ref) -> list:
    """[(first IF sample, Df, nominal tap set)] of a harness run: the start (with --dc the acquisition set, :1263-1266), then every window
    behind which Df or the tap set is another (:1526-1543)"""
    s = [(0, 0.0, 0 if ref["dc"] else 1)]
    for w in ref["win"]:
        if (w["Df"], int(w["nominal"])) != s[-1][1:]:
            s.append((int(w["sample"]) * ref["consts"]["decFM"], w["Df"], int(w["nominal"])))
    return s


@functools.lru_cache(maxsize=None)
def reference(cid: str, libname: str = "libref_mk2a_O2.so", seed: int | None = None) -> dict:
    """the compiled reference's run of the case (oracle/_ref/<libname>), computed once and shared read-only"""
    from oracle import ref_front
    c = BY_ID[cid]
    r = ref_front.ref_mk2a_run(capture(cid, seed), sr_of(c), libname=libname, **ref_kw(c))
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def front_of(cid: str, seed: int | None = None) -> np.ndarray:
    """front() of the case, shared read-only (it depends on tables that both builds of the reference compute alike)"""
    z = front(capture(cid, seed), bits_of(BY_ID[cid]), reference(cid, seed=seed))
    z.setflags(write=False)
    return z


# ----------------------------------------------------------------------------------------------- the model
def samples_of(raw, bits) -> np.ndarray:
    """complex float64 samples as f32read_cblock converts them: int16 / 32768, (uint8 - 128) / 128 (exact)"""
    raw = np.asarray(raw)
    v = raw.astype(np.float64) / 32768.0 if bits == 16 else (raw.astype(np.float64) - 128.0) / 128.0
    return v[0::2] + 1j * v[1::2]


def iqdc_blocks(n, maxcnt0, maxlim):
    """[(first sample, length)] of the IQ-dc blocks that END inside n samples: maxcnt doubles while below maxlim"""
    out, pos, m = [], 0, maxcnt0
    while pos + m <= n:
        out.append((pos, m))
        pos += m
        if m < maxlim:
            m *= 2
    return out


def iqdc_mean(x, maxcnt0, maxlim):
    """per sample the float32 mean in effect (the block before it; 0 in the first block), and the list of (block end, mean)"""
    avg = np.zeros(len(x), np.complex128)
    ends = []
    for first, m in iqdc_blocks(len(x), maxcnt0, maxlim):
        s = x[first:first + m].sum()                                  # exact: multiples of 2^-15, fewer than 2^37 of them
        a = complex(np.float32(s.real / float(np.float32(m))), np.float32(s.imag / float(np.float32(m))))
        avg[first + m:] = a
        ends.append((first + m, a))
    return avg, ends


def _fir(x, w, stride=1, first=0):
    """y[k] = sum_a w[T-1-a] x[s-a], s = first + k stride: lowpass() / re_lowpass() of the reference (slot n holds the sample of age
    (s - n) mod T and meets ws[T - (s+1) % T + n] = w[T-1-age]); samples before the stream start are the zeroed buffer"""
    y = np.convolve(x, np.asarray(w, np.float64)[::-1])[:len(x)]
    return y[first::stride]


def front(raw, bits, ref):
    """the part that does not depend on the AFC -> float64 IF samples (k_mk2a_mix): IQ-dc, mixer table, decimator"""
    k = ref["consts"]
    x = samples_of(raw, bits)
    avg, _ = iqdc_mean(x, k["maxcnt0"], k["maxlim"])
    lut = ref["lut"].astype(np.complex128)
    z = (x - avg) * lut[np.arange(len(x)) % len(lut)]
    D = k["decM"]
    n_if = len(x) // D
    if D > 1:
        z = _fir(z, ref["ws"]["dec"][:k["dectaps"]], D, D - 1)
    return z[:n_if]


def model(ifin, ref, schedule, n_if=None):
    """the AFC-dependent chain on float64 IF samples with the given schedule -> dict of float64 streams:
    zrot, zlp (complex, per IF sample), fm, sraw (per IF sample), bufs, fmbuf (per output sample)"""
    k = ref["consts"]
    n = len(ifin) if n_if is None else n_if
    y = np.asarray(ifin[:n], np.complex128)
    u = np.arange(n)
    Df = np.zeros(n)
    nominal = np.zeros(n, bool)
    for first, df, nom in schedule:
        Df[first:] = df
        nominal[first:] = bool(nom)
    opt_dc = ref["dc"]
    zrot = y * np.exp(-2j * np.pi * np.mod((u / float(k["if_sr"])) * Df, 1.0)) if opt_dc else y
    if k["lp"] & 1:
        T = k["iq_taps"]
        z1 = _fir(zrot, ref["ws"]["iq1"][:T])
        zlp = np.where(nominal, z1, _fir(zrot, ref["ws"]["iq0"][:T])) if not nominal.all() else z1
    else:
        zlp = zrot
    zp = np.concatenate([[0.0 + 0.0j], zlp[:-1]])
    wr = zlp.real * zp.real + zlp.imag * zp.imag                     # w = z conj(z_-1), written out: sample 0 and digital silence give signed zeros
    wi = zlp.imag * zp.real - zlp.real * zp.imag
    fm = 0.8 * np.arctan2(wi, wr) / np.pi
    sraw = None
    if ref["tone"] is not None and len(ref["tone"]) and ref["sraw"] is not None:
        X1 = np.zeros(n, np.complex128)
        X2 = np.zeros(n, np.complex128)
        for lag, e1r, e1i, e2r, e2i in ref["tone"]:
            lag = int(lag)
            zz = np.concatenate([np.zeros(lag, np.complex128), zlp[:n - lag]])
            X1 += zz * complex(e1r, e1i)
            X2 += zz * complex(e2r, e2i)
        sraw = (np.abs(X2) - np.abs(X1)) / k["tone_sps"]
    d = k["decFM"]
    fmbuf = _fir(fm, ref["ws"]["fm"][:k["fm_taps"]], d, d - 1) if k["lp"] & 2 else fm[d - 1::d]
    if sraw is None:
        bufs = fmbuf
    else:
        bufs = _fir(sraw, ref["ws"]["iqfm"][:k["iqfm_taps"]], d, d - 1) if k["lp"] & 4 else sraw[d - 1::d]
    n_out = n // d
    return dict(zrot=zrot, zlp=zlp, fm=fm, sraw=sraw, bufs=bufs[:n_out], fmbuf=fmbuf[:n_out])


def literal(raw, bits, ref, schedule, probes_if, probes_out):
    """the same sums term by term at single samples -> dict(ifin, zrot, zlp, fm, sraw at probes_if; bufs, fmbuf at probes_out)"""
    import math
    k = ref["consts"]
    x = samples_of(raw, bits)
    blocks = iqdc_blocks(len(x), k["maxcnt0"], k["maxlim"])
    means = []
    for first, m in blocks:
        sr_, si_ = 0.0, 0.0
        for v in x[first:first + m]:
            sr_ += v.real
            si_ += v.imag
        means.append((first + m, complex(np.float32(sr_ / float(np.float32(m))), np.float32(si_ / float(np.float32(m))))))
    lut = ref["lut"].astype(np.complex128)
    D, d = k["decM"], k["decFM"]
    wdec, wiq0, wiq1 = (ref["ws"][n][:len(ref["ws"][n]) // 2].astype(np.float64) for n in ("dec", "iq0", "iq1"))
    wfm, wiqfm = (ref["ws"][n][:len(ref["ws"][n]) // 2].astype(np.float64) for n in ("fm", "iqfm"))
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

    def sched(u):
        cur = schedule[0]
        for e in schedule:
            if u >= e[0]:
                cur = e
        return cur

    opt_dc = ref["dc"]

    @cached
    def zrot(u):
        if not opt_dc:
            return ifin(u)
        ph = math.fmod((u / float(k["if_sr"])) * sched(u)[1], 1.0)
        return ifin(u) * complex(math.cos(2 * math.pi * ph), -math.sin(2 * math.pi * ph))

    @cached
    def zlp(u):
        if not k["lp"] & 1:
            return zrot(u)
        w = wiq1 if sched(u)[2] else wiq0
        return sum(w[len(w) - 1 - a] * zrot(u - a) for a in range(len(w)))

    @cached
    def fm(u):
        z, p = complex(zlp(u)), complex(zlp(u - 1))
        return 0.8 * math.atan2(z.imag * p.real - z.real * p.imag, z.real * p.real + z.imag * p.imag) / math.pi

    @cached
    def sraw(u):
        X1 = sum(complex(zlp(u - int(t[0]))) * complex(t[1], t[2]) for t in ref["tone"])
        X2 = sum(complex(zlp(u - int(t[0]))) * complex(t[3], t[4]) for t in ref["tone"])
        return (abs(X2) - abs(X1)) / k["tone_sps"]

    def out(n, f, w, lp):
        ul = n * d + d - 1
        return sum(w[len(w) - 1 - a] * f(ul - a) for a in range(len(w))) if lp else f(ul)

    tone = ref["sraw"] is not None
    res = dict(ifin=np.array([ifin(int(u)) for u in probes_if]), zrot=np.array([zrot(int(u)) for u in probes_if]), zlp=np.array([zlp(int(u)) for u in probes_if]),
               fm=np.array([fm(int(u)) for u in probes_if]), sraw=np.array([sraw(int(u)) for u in probes_if]) if tone else None,
               fmbuf=np.array([out(int(n), fm, wfm, k["lp"] & 2) for n in probes_out]))
    res["bufs"] = np.array([out(int(n), sraw, wiqfm, k["lp"] & 4) for n in probes_out]) if tone else res["fmbuf"]
    return res


# ----------------------------------------------------------------------------------------------- figures
STREAMS = ("ifin", "zrot", "zlp", "fm", "sraw", "bufs", "fmbuf")


def rms(a):
    a = np.asarray(a)
    return float(np.sqrt(np.mean(np.abs(a) ** 2))) if a.size else 0.0


def figure(got, want, sl=slice(None)):
    """(RMS, max-abs) of got - want on the samples sl where both are numbers (the harness marks samples it could not record with NaN);
    for the complex streams over the real and imaginary parts as separate values, like the IQ figures of the other sweeps"""
    g, w = np.asarray(got)[sl], np.asarray(want)[sl]
    n = min(len(g), len(w))
    d = g[:n].astype(np.complex128 if np.iscomplexobj(g) or np.iscomplexobj(w) else np.float64) - w[:n]
    d = d[~np.isnan(d)]
    if np.iscomplexobj(d):
        d = np.concatenate([d.real, d.imag])
    return (rms(d), float(np.abs(d).max()) if d.size else 0.0)
