"""Decimator parity sweep: the base-rate front end (mixer, IQ-DC removal, low-pass, decimation) at the input rates receivers really use,
through every kernel variant sonde_launch_mix_decimate / the engine / the scanner pick between, for every way the calls cut the stream.

Inputs are generated and seeded (tests/decim_sweep_cases.py lists the rates and what each selects; tests/test_decim_sweep_design.py
keeps that list honest without a GPU).  Per channel 0.12 s of IQ: a 4800 Bd FSK tone (+-2.4 kHz) at the channel's fq with amplitude 0.35,
an interferer at fq + 0.23 (wrapped into +-0.5) with amplitude 0.2, Gaussian noise of sigma 0.05 and an IQ-DC offset of 0.06 - 0.04j —
about 5800 IF samples, across the first two changes of the IQ-DC mean (blocks if_sr/32 and 3 if_sr/32).

Reference: the CPU oracle's streams (oracle.ora_streams; bit for bit the reference's -O2 build), the compiled reference itself
(libref_demod_O2.so) where the oracle has no switch (--min, --noLUT), and oracle/_ref/iq_dec for the front-end-only engine.

Tolerances, the project's own (tests/test_gpu_parity.py, tests/test_gpu_iqdec.py), on EVERY case and channel:
  decimated IQ, IF-filtered IQ, FM .... 1e-6 RMS
  decimated IQ, IF-filtered IQ ........ 2e-5 max-abs  (one wrong output at a tile, call or segment edge is 1e-2 or more)
  tone-correlator stream bufs ......... 1e-5 RMS
  info[if_sr, decM, dectaps, lut_len] . equal to the reference's consts
  calls cut anywhere .................. the same bits as the one-call run
  against the defining sum in float64 . RMS deviation of the GPU <= 3 x the oracle's own on the same outputs + 1e-8 (the factor
                                        test_gpu_parity.py applies to the reference's floor); the outputs are the first and last 16,
                                        +-8 around each IQ-DC segment edge and around each multiple of 64 (tile) and 232 (workgroup,
                                        4 x (64 - 6) rows) below 1000 — 350 to 370 outputs; the list as given is kept whole rather
                                        than cut to 256, a T-tap dot product each
The reference's own -Ofast build stays within 1.64e-7 RMS / 1.04e-6 max of the -O2 build on this signal at 96 k ... 10 M, so the
bounds leave it a margin of 6 x / 19 x.

Front-end-only cases: `--IFbw 8` at 48 kHz is below the 32 kHz the reference's parser accepts (iq_dec.c:998), so the reference ignores it
and runs D = 1 (pass-through minus the IQ-DC mean); no `--IFbw` gives fewer than 5 tap columns (T = 4 D IF / (IF - 20 k)).  The case stays
as a D = 1 front-end case, the engine is made the way host/iq_dec.c maps the same arguments.

Measured, one call per case (GPU: MI355X against the oracle, as this sweep prints it; "- f64": RMS deviation from the float64 sum, GPU / oracle;
reference alone: its -Ofast build against its -O2 build, on the CPU).  All columns of all cases: DESIGN.md §2a.
  case            GPU dec RMS / max      GPU bufs RMS   - f64 GPU / oracle     reference alone RMS / max
  130k            2.22e-08 / 1.19e-07    4.38e-07       1.58e-08 / 1.66e-08    1.37e-08 / 5.96e-08
  250k            2.94e-08 / 1.49e-07    2.76e-07       1.56e-08 / 2.59e-08    2.73e-08 / 1.49e-07
  1024k           5.03e-08 / 2.68e-07    3.05e-07       1.61e-08 / 4.76e-08    5.08e-08 / 2.98e-07
  1800k           6.71e-08 / 4.77e-07    2.76e-07       1.95e-08 / 6.57e-08    6.90e-08 / 5.36e-07
  2048k           7.12e-08 / 4.47e-07    1.81e-07       2.00e-08 / 6.57e-08    7.22e-08 / 5.07e-07
  2400k           8.13e-08 / 4.47e-07    4.48e-07       2.26e-08 / 7.46e-08    8.27e-08 / 5.07e-07
  2500k           7.97e-08 / 4.77e-07    2.26e-07       2.38e-08 / 7.75e-08    8.15e-08 / 5.66e-07
  2560k           7.96e-08 / 5.07e-07    3.28e-07       2.12e-08 / 7.54e-08    8.14e-08 / 5.07e-07
  3072k           9.13e-08 / 5.07e-07    3.08e-07       2.39e-08 / 8.67e-08    9.45e-08 / 5.36e-07
  3200k           9.15e-08 / 6.56e-07    2.17e-07       2.46e-08 / 8.72e-08    9.40e-08 / 6.85e-07
  3600k           9.81e-08 / 6.56e-07    1.44e-07       2.51e-08 / 9.26e-08    1.01e-07 / 7.45e-07
  6000k           1.27e-07 / 8.35e-07    3.32e-07       3.03e-08 / 1.16e-07    1.32e-07 / 9.24e-07
  1600k --min     8.23e-08 / 5.36e-07    2.54e-07       2.40e-08 / 7.55e-08    8.29e-08 / 5.66e-07
  2048k --min     9.00e-08 / 5.36e-07    2.54e-07       2.57e-08 / 8.91e-08    9.31e-08 / 5.66e-07
  2400k --min     9.46e-08 / 5.07e-07    1.42e-07       2.74e-08 / 8.47e-08    9.78e-08 / 5.36e-07
  2048k 8-bit     7.14e-08 / 4.17e-07    2.69e-07       2.07e-08 / 6.61e-08    7.30e-08 / 4.47e-07
  2048k float32   6.05e-08 / 4.17e-07    3.48e-07       7.10e-08 / 6.70e-08    7.31e-08 / 4.77e-07
  2500k 8-bit     8.08e-08 / 4.77e-07    2.73e-07       2.22e-08 / 7.86e-08    8.19e-08 / 4.77e-07
  2500k float32   6.69e-08 / 4.47e-07    2.80e-07       7.81e-08 / 8.06e-08    8.18e-08 / 4.77e-07
  2048k --noLUT   7.18e-08 / 3.87e-07    2.79e-07       2.17e-08 / 6.83e-08    7.35e-08 / 4.17e-07
  100k 4.2 s      2.38e-08 / 1.49e-07    2.04e-06       -                      1.84e-08 / 1.19e-07
  13 channels     8.19e-08 / 6.26e-07    5.15e-07       (worst channel; 2.5 Msps; 2.048 Msps and the shared 3.6 Msps stream are below it)
  front end       8.36e-08 / 3.87e-07                   (worst: 960 k --IFbw 32, Q 11; against the compiled -Ofast iq_dec)
What this sweep found when it first ran is in DESIGN.md §4.1 (regression note): six blocks too many in every IQ-DC mean of k_mix_decimate50
(8.1e-4 RMS at fq = 0, 4.5e-6 behind every change of the mean elsewhere), and decimated IQ / bufs whose last bits depended on where a call began.
D = 64 (65 600 bytes of dynamic LDS) launched as it was.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
from decim_sweep_cases import SWEEP, LONG, REFUSED, case_id
from golden_cases import rms, need_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECONDS = 0.12
O2 = "libref_demod_O2.so"
BY_ID = {case_id(c): c for c in SWEEP}
FQ13 = [0.31, -0.07, 0.0, 0.19, -0.333, 0.1234, 0.485, -0.41, 0.27, -0.151, 0.05, -0.22, 0.37]


# ----------------------------------------------------------------------------------------------- signal and references (computed once, shared)
def _wrap(f):
    return (f + 0.5) % 1.0 - 0.5


def _tones(sr, fqs, seed, seconds, amp):
    rng = np.random.default_rng(seed)
    n = int(round(sr * seconds))
    t = np.arange(n)
    x = np.zeros(n, np.complex128)
    for fq in fqs:
        sym = (rng.integers(0, 2, n * 4800 // sr + 2) * 2 - 1)[t * 4800 // sr]
        x += amp * np.exp(2j * np.pi * np.cumsum(fq + sym * 2400.0 / sr))
    x += 0.2 * np.exp(2j * np.pi * _wrap(fqs[0] + 0.23) * t)
    x += 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x + (0.06 - 0.04j)


def _quantise(x, bits):
    v = np.empty(2 * len(x))
    v[0::2], v[1::2] = x.real, x.imag
    if bits == 32:
        return v.astype(np.float32)
    if bits == 8:
        return np.clip(np.round(v * 128.0 + 128.0), 0, 255).astype(np.uint8)
    return np.clip(np.round(v * 32768.0), -32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def _signal(sr, fq, seed, bits=16, seconds=SECONDS, shared=False):
    """interleaved IQ as the reference reads it from its input; shared: ONE stream that carries a tone at each of FQ13 (amplitude 0.04 each, so
    that thirteen carriers, the interferer, the offset and 4 sigma of noise stay inside the sample range), for thirteen channels to mix out of"""
    x = _quantise(_tones(sr, FQ13, seed, seconds, 0.04) if shared else _tones(sr, [fq], seed, seconds, 0.35), bits)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _ref(sr, opt_min, fq, seed, bits=16, nolut=False, seconds=SECONDS, shared=False):
    """the four IF-rate streams and the consts of the reference for one channel (None without a reference for --min / --noLUT)"""
    from oracle import bind
    x = _signal(sr, 0.0 if shared else fq, seed, bits, seconds, shared)
    if opt_min or nolut:
        if not need_ref():
            return None
        a = bind.ref_streams(x, sr, bps=bits, fq=fq, lp_iq=False, libname=O2, opt_min=opt_min, nolut=nolut)
        b = bind.ref_streams(x, sr, bps=bits, fq=fq, lp_iq=True, libname=O2, opt_min=opt_min, nolut=nolut)
    else:
        a = bind.ora_streams(x, sr, bps=bits, fq=fq, lp_iq=False)
        b = bind.ora_streams(x, sr, bps=bits, fq=fq, lp_iq=True)
    assert a["n"] == b["n"] and a["consts"]["decM"] == b["consts"]["decM"]
    out = dict(n=a["n"], dec=a["iq"], ifiq=b["iq"], fm=b["fm"], bufs=b["bufs"], consts=b["consts"])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ----------------------------------------------------------------------------------------------- the engine
def _cuts(kind, n_if, if_sr):
    """blocks per call.  A: one block, a tile +-1, two tiles -1, a workgroup (4 x (64 - 6) rows) and +1, then exactly up to the first IQ-DC segment edge.
    B: odd launches (the single-tile fallback kernel of a D = 50 engine), a call that straddles a segment edge by one block, the tail carry between kernels."""
    seg = if_sr // 32
    head = {"one": [], "A": [1, 63, 64, 65, 127, 232, 233, seg - 785], "B": [seg - 1, 3, 2 * seg - 1]}[kind]
    assert all(b > 0 for b in head) and sum(head) < n_if
    if kind == "A":
        assert sum(head) == seg
    return head + [n_if - sum(head)]


def _run(sr, fqs, X, *, cuts="one", shared=False, taps=True, **kw):
    """feed X ([C, 2n] or [2n]) in the given cut; -> (info, {tap name: [C, n_if(, 2)]})"""
    from radiosonde_auto_rx_amd import engine as E
    eng = E.Engine(fqs, sr, keep_soft=True, max_chunk=sr, **kw)
    try:
        D = eng.info["decM"]
        X = np.asarray(X)
        n_if = X.shape[-1] // 2 // D
        pos = 0
        for b in _cuts(cuts, n_if, eng.info["if_sr"]):
            eng.process_host(X[..., 2 * D * pos:2 * D * (pos + b)], shared=shared)
            pos += b
        assert pos == n_if
        names = dict(dec=E.TAP_DECIM, ifiq=E.TAP_IFIQ, fm=E.TAP_FM, bufs=E.TAP_BUFS) if taps else dict(dec=E.TAP_DECIM)
        out = {k: np.stack([eng.read_tap(c, t, 0, n_if) for c in range(len(fqs))]) for k, t in names.items()}
        return dict(eng.info), out
    finally:
        eng.close()


def _check(tag, got, ref, c=0):
    """the tolerances of the module docstring for channel c of a run; prints every figure first"""
    n = ref["n"]
    assert got["dec"].shape[1] == n
    fig = {}
    for k in got:
        d = got[k][c].astype(np.float64) - ref[k]
        fig[k] = (rms(d), float(np.abs(d).max()))
    print("SWEEP %-34s " % tag + "  ".join("%s rms %.3e max %.3e" % (k, *fig[k]) for k in fig))
    for k in ("dec", "ifiq"):
        if k in fig:
            assert fig[k][0] < 1e-6 and fig[k][1] < 2e-5, (tag, k, fig[k])
    if "fm" in fig:
        assert fig["fm"][0] < 1e-6, (tag, fig["fm"])
        assert fig["bufs"][0] < 1e-5, (tag, fig["bufs"])
    return fig


def _check_info(info, ref):
    assert (info["decM"], info["dectaps"], info["lut_len"], info["if_sr"]) == tuple(ref["consts"][k] for k in ("decM", "dectaps", "lut_len", "if_sr"))


# ----------------------------------------------------------------------------------------------- the defining sum in float64
def _segments(if_sr, D, n):
    """[first sample, length] of the reference's IQ-DC segments up to sample n (demod_mod.c:495-504: if_sr/32 blocks, doubling up to the first length >= if_sr)"""
    ln, lim, s0, out = if_sr // 32 * D, if_sr * D, 0, []
    while s0 < n:
        out.append((s0, ln))
        s0 += ln
        if ln < lim:
            ln *= 2
    return out


def _exact(x, bits, sr, fq, consts, ms, nolut=False):
    """y[m] = sum_k w[k] (x[(m+1) D - T + k] - mean) mix[(m+1) D - T + k] in float64, w / mix = the reference's float32 taps and table (liboracle.so's
    design functions), mean = the segment means as the reference updates them: (float)(double sum / (float)length) of the segment before"""
    from oracle import bind
    L = bind.lib()
    D, T, if_sr = consts["decM"], consts["dectaps"], consts["if_sr"]
    free = C.CDLL(None).free
    free.argtypes = [C.c_void_p]
    p = C.POINTER(C.c_float)()
    L.ora_lowpass_design.argtypes = [C.c_float, C.c_int, C.POINTER(C.POINTER(C.c_float))]
    assert L.ora_lowpass_design(float(np.float32((if_sr + 20e3) / (4.0 * sr))), T, C.byref(p)) == T
    w = np.ctypeslib.as_array(p, (T,)).astype(np.float64)
    free(p)
    v = np.asarray(x)
    v = v.astype(np.float64) if bits == 32 else (v.astype(np.float64) - 128.0) / 128.0 if bits == 8 else v.astype(np.float64) / 32768.0
    z = v[0::2] + 1j * v[1::2]
    n = len(z)
    mean = np.zeros(n, np.complex128)
    for s0, ln in _segments(if_sr, D, n):
        if s0 + ln < n:
            s = z[s0:s0 + ln].sum()
            mean[s0 + ln:] = complex(np.float32(s.real / np.float32(ln)), np.float32(s.imag / np.float32(ln)))
    idx = (np.asarray(ms)[:, None] + 1) * D - T + np.arange(T)[None, :]
    ok = idx >= 0
    idx = np.where(ok, idx, 0)
    if nolut:
        frac = np.mod(-fq * idx.astype(np.float64), 1.0)
        mix = np.exp(2j * np.pi * frac)
    else:
        q = C.POINTER(C.c_float)()
        L.ora_lut_design.argtypes = [C.c_double, C.c_int, C.POINTER(C.POINTER(C.c_float))]
        ll = L.ora_lut_design(-fq, sr, C.byref(q))
        assert ll == consts["lut_len"]
        t = np.ctypeslib.as_array(q, (2 * ll,)).astype(np.float64)
        free(q)
        mix = (t[0::2] + 1j * t[1::2])[idx % ll]
    y = (((z[idx] - mean[idx]) * mix * ok) @ w)
    return np.stack([y.real, y.imag], axis=1)


def _probes(n_if, if_sr, D):
    s = set(range(16)) | set(range(n_if - 16, n_if))
    for s0, _ in _segments(if_sr, D, n_if * D)[1:]:
        s |= set(range(s0 // D - 8, s0 // D + 8))
    for k in (64, 232):
        for m in range(k, 1000, k):
            s |= set(range(m - 8, m + 8))
    return np.array(sorted(m for m in s if 0 <= m < n_if))


def _check_exact(tag, x, bits, sr, fq, ref, got_dec, nolut=False):
    ms = _probes(ref["n"], ref["consts"]["if_sr"], ref["consts"]["decM"])
    y = _exact(x, bits, sr, fq, ref["consts"], ms, nolut)
    d_ref, d_gpu = rms(ref["dec"][ms] - y), rms(got_dec[ms] - y)
    print("EXACT %-34s outputs %d  oracle-float64 rms %.3e  gpu-float64 rms %.3e" % (tag, len(ms), d_ref, d_gpu))
    assert d_ref < 1e-6                                         # the float64 sum is the sum the reference computes
    assert d_gpu <= 3 * d_ref + 1e-8, (tag, d_gpu, d_ref)


@functools.lru_cache(maxsize=None)
def _one_call(cid):
    c = BY_ID[cid]
    ref = _ref(c["sr"], c["opt_min"], c["fq"], 7)
    info, got = _run(c["sr"], [c["fq"]], _signal(c["sr"], c["fq"], 7), opt_min=c["opt_min"])
    return ref, info, got


# ----------------------------------------------------------------------------------------------- decoder engine
@pytest.mark.parametrize("cid", list(BY_ID))
def test_rate(oracle, cid):
    """every rate of the table, one call: launches (D = 64 asks for 65 600 bytes of LDS), the reference's design, the four streams, the float64 sum"""
    c = BY_ID[cid]
    ref, info, got = _one_call(cid)
    assert (info["decM"], info["dectaps"], info["lut_len"], info["if_sr"]) == (c["D"], c["T"], c["lut_len"], c["if_sr"])
    if ref is None:
        return                                                  # --min without the compiled reference (SONDE_ALLOW_NO_REF=1): launch and design only
    _check_info(info, ref)
    _check(cid, got, ref)
    _check_exact(cid, _signal(c["sr"], c["fq"], 7), 16, c["sr"], c["fq"], ref, got["dec"][0])


@pytest.mark.parametrize("kind", ["A", "B"])
@pytest.mark.parametrize("cid", ["2400k", "2500k", "2560k", "1600k_min", "2048k"])
def test_call_cuts_give_the_same_bits(oracle, cid, kind):
    c = BY_ID[cid]
    ref, info, one = _one_call(cid)
    _, got = _run(c["sr"], [c["fq"]], _signal(c["sr"], c["fq"], 7), cuts=kind, opt_min=c["opt_min"])
    for k in one:
        bad = np.flatnonzero((got[k][0] != one[k][0]).reshape(len(one[k][0]), -1).any(axis=1))
        assert bad.size == 0, (cid, kind, k, "first differing IF samples", bad[:8], "of", bad.size)
    if ref is not None:
        _check("%s cut %s" % (cid, kind), got, ref)


@pytest.mark.parametrize("bits,nolut,cid", [(8, False, "2048k"), (32, False, "2048k"), (8, False, "2500k"), (32, False, "2500k"), (16, True, "2048k")])
def test_input_types(oracle, bits, nolut, cid):
    """8-bit input (converted in front of the 16-bit kernels), float32 input (k_mix_f32 + k_decimate_f32) and --noLUT (mixer from the running double phase)"""
    c = BY_ID[cid]
    ref = _ref(c["sr"], False, c["fq"], 11, bits, nolut)
    x = _signal(c["sr"], c["fq"], 11, bits)
    info, got = _run(c["sr"], [c["fq"]], x, bits=bits, nolut=nolut)
    assert info["decM"] == c["D"] and info["dectaps"] == c["T"]
    if ref is None:
        return
    tag = "%s bits %d%s" % (cid, bits, " noLUT" if nolut else "")
    _check(tag, got, ref)
    _check_exact(tag, x, bits, c["sr"], c["fq"], ref, got["dec"][0], nolut)


@pytest.mark.parametrize("G", [2, 16])
def test_tiles_per_wave(oracle, monkeypatch, G):
    """the hand-scheduled kernel with 2 and 16 tiles per wave (what large batches run with) on the 2.5 Msps case"""
    monkeypatch.setenv("SONDE_MD_G", str(G))
    c = BY_ID["2500k"]
    ref = _ref(c["sr"], False, c["fq"], 7)
    x = _signal(c["sr"], c["fq"], 7)
    info, got = _run(c["sr"], [c["fq"]], x)
    _check_info(info, ref)
    _check("2500k G %d" % G, got, ref)
    _check_exact("2500k G %d" % G, x, 16, c["sr"], c["fq"], ref, got["dec"][0])


@pytest.mark.parametrize("sr", [2_500_000, 2_048_000])
def test_thirteen_channels(oracle, sr):
    """13 channels (no multiple of 8, more than one group of 8), 13 carriers and seeds: every channel inside the same bounds"""
    X = np.stack([_signal(sr, f, 100 + i) for i, f in enumerate(FQ13)])
    info, got = _run(sr, FQ13, X)
    for i, f in enumerate(FQ13):
        ref = _ref(sr, False, f, 100 + i)
        _check_info(info, ref)
        _check("%dk ch %d fq %+.4f" % (sr // 1000, i, f), got, ref, c=i)


def test_thirteen_channels_of_one_shared_stream(oracle):
    """the same 13 carriers mixed out of ONE 3.6 Msps stream (channel stride 0) by the wide kernel, DS 25"""
    sr = 3_600_000
    x = _signal(sr, 0.0, 200, shared=True)
    info, got = _run(sr, FQ13, x, shared=True)
    assert (info["decM"], info["if_sr"]) == (75, 48_000)
    for i, f in enumerate(FQ13):
        _check("3600k shared ch %d fq %+.4f" % (i, f), got, _ref(sr, False, f, 200, shared=True), c=i)


def test_long_iq_dc_schedule(oracle):
    """100 kHz (D 2, IF 50 000), 4.2 s in 0.7 s calls: the IQ-DC segments run 1562 x 2^k blocks up to 99 968, which is then used twice; max-abs over the whole stream"""
    from radiosonde_auto_rx_amd import engine as E
    c = LONG
    sr, D = c["sr"], c["D"]
    x = _signal(sr, c["fq"], 31, seconds=4.2)
    ref = _ref(sr, False, c["fq"], 31, seconds=4.2)
    assert [s0 // D for s0, _ in _segments(c["if_sr"], D, len(x) // 2)] == [0, 1562, 4686, 10934, 23430, 48422, 98406, 198374]
    eng = E.Engine([c["fq"]], sr, keep_soft=True, max_chunk=70_000)
    _check_info(eng.info, ref)
    got = {k: [] for k in ("dec", "ifiq", "fm", "bufs")}
    per = 70_000 // D
    for i in range(6):
        eng.process_host(x[2 * 70_000 * i:2 * 70_000 * (i + 1)])
        for k, t in (("dec", E.TAP_DECIM), ("ifiq", E.TAP_IFIQ), ("fm", E.TAP_FM), ("bufs", E.TAP_BUFS)):
            got[k].append(eng.read_tap(0, t, per * i, per))
    eng.close()
    _check("100k 4.2 s", {k: np.concatenate(v)[None] for k, v in got.items()}, ref)


def test_prime_decimation_above_64_is_refused_cleanly(oracle):
    """3.216 Msps is D = 67: no piece length for the wide kernel.  sonde_engine_create returns SONDE_E_ARG, and the process goes on: the next engine works"""
    from radiosonde_auto_rx_amd import engine as E
    with pytest.raises(E.SondeError) as ei:
        E.Engine([REFUSED["fq"]], REFUSED["sr"])
    assert "(-1)" in str(ei.value) and E.lib().sonde_strerror(-1).decode() in str(ei.value)
    c = BY_ID["250k"]
    ref = _ref(c["sr"], False, c["fq"], 7)
    _, got = _run(c["sr"], [c["fq"]], _signal(c["sr"], c["fq"], 7))
    _check("250k after the refusal", got, ref)


# ----------------------------------------------------------------------------------------------- front-end-only engine (double mixer phase)
FRONT = [dict(sr=2_048_000, fq=0.21, ifbw=0, D=40), dict(sr=2_400_000, fq=-0.12, ifbw=192, D=12), dict(sr=48_000, fq=0.07, ifbw=8, D=1),
         dict(sr=960_000, fq=0.3, ifbw=32, D=30)]


@pytest.mark.parametrize("c", FRONT, ids=lambda c: "%dk_ifbw%d" % (c["sr"] // 1000, c["ifbw"]))
def test_front_end_engine_matches_compiled_iq_dec(oracle, c):
    """`iq_dec --iq fq --bo 32 [--IFbw k] - sr 16` of the compiled reference against the decimated-IQ tap of a sonde="frontend" engine: D 40 (generic kernel,
    double table phase), D 12 / Q 5, D 1, and Q 11 (more tap columns than the packed kernels hold: int16 converted for the float32 path)"""
    if not need_ref():
        return
    from radiosonde_auto_rx_amd import engine as E
    sr = c["sr"]
    x = _signal(sr, c["fq"], 51)
    args = ["--iq", repr(c["fq"]), "--bo", "32"] + (["--IFbw", str(c["ifbw"])] if c["ifbw"] else []) + ["-", str(sr), "16"]
    import subprocess
    r = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "iq_dec")] + args, input=x.tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = np.frombuffer(r.stdout, "<f4").reshape(-1, 2)
    if_rate = c["ifbw"] * 1000 if c["ifbw"] * 1000 >= 32000 else 0          # host/iq_dec.c, as iq_dec.c:998
    eng = E.Engine([c["fq"]], sr, sonde="frontend", lp_iq=False, if_rate=if_rate, max_chunk=sr)
    D = eng.info["decM"]
    said = r.stderr.decode().splitlines()
    assert D == c["D"] and "IF: %d" % eng.info["if_sr"] in said and (D == 1 or "dec: %d" % D in said), said
    n = len(x) // 2 // D * D
    eng.process_host(x[:2 * n])
    got = eng.read_tap(0, E.TAP_DECIM, 0, n // D)
    eng.close()
    m = min(len(want), len(got))
    assert m >= n // D - 1
    d = got[:m].astype(np.float64) - want[:m]
    print("FRONT %dk ifbw %d D %d  rms %.3e max %.3e" % (sr // 1000, c["ifbw"], D, rms(d), np.abs(d).max()))
    assert rms(d) < 1e-6 and np.abs(d).max() < 2e-5


# ----------------------------------------------------------------------------------------------- scanner front end
@functools.lru_cache(maxsize=None)
def _scan_case(sr):
    from oracle import bind
    from tools import synth
    fq = synth.snap_fq(0.1, sr)
    x = synth.rs41_capture(sr=sr, seconds=1.2, fq=fq, n_frames=1, t_first=0.05, noise_sigma=0.02, seed=5, dc=0.05 - 0.03j)[:2 * int(0.7 * sr)]
    g = bind.ref_scan_windows(x, sr, iq_mode=5, fq=fq, dc=True, max_win=64)
    return x, fq, g


@pytest.mark.parametrize("chunk", ["0.35s", "7x350"])
@pytest.mark.parametrize("sr,two_pass", [(2_500_000, False), (2_500_000, True), (2_048_000, False)])
def test_scanner_front_end(oracle, monkeypatch, sr, two_pass, chunk):
    """Scanner(exact=True) against the reference's own getCorrDFT per window, --dc, 0.7 s with an RS41 header inside window 1.  2.5 Msps: the one-pass
    k_mix_decimate50r + k_scan_dc_edges at IQ-DC windows of 1562 blocks, and the two-pass form; 2.048 Msps: the generic kernel with the table of window means"""
    if not need_ref():
        return
    from test_gpu_scan import _check_windows
    from radiosonde_auto_rx_amd.scan import Scanner, BBIQ
    if two_pass:
        monkeypatch.setenv("SONDE_SCAN_TWO_PASS", "1")
    else:
        monkeypatch.delenv("SONDE_SCAN_TWO_PASS", raising=False)
    x, fq, g = _scan_case(sr)
    assert g["n"] >= 5 and abs(g["mv"][1][1]) > 0.7 and g["herrs"][1][1] == 0          # RS41 (template 1) found in window 1, header without bit errors
    sc = Scanner(sr, fq=[fq], iq_mode=BBIQ, dc=True, cont=True, max_chunk=sr, exact=True)
    D = sc.info["decM"]
    assert (D, sc.info["if_sr"], sc.info["K"]) == (g["consts"]["decM"], g["consts"]["sr_if"], g["consts"]["K"])
    step = int(0.35 * sr) // D * D if chunk == "0.35s" else 7 * 350 * D
    n = len(x) // 2 // D * D
    wins = []
    for s0 in range(0, n, step):
        sc.process_host(x[2 * s0:2 * min(n, s0 + step)])
        wins += sc.last_windows()
        sc.fetch()
    sc.close()
    assert len(wins) == g["n"]
    for w in wins:
        print("SCAN %dk%s %s  window %d  RS41 mv %+.5f (ref %+.5f)" % (sr // 1000, " two-pass" if two_pass else "", chunk, w["pos"], w["mv"][1], g["mv"][len([1 for v in g["pos"] if v < w["pos"]])][1]))
    _check_windows(wins, g)
