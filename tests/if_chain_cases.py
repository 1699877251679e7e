"""The IF chain's sweep: case table, seeded signal and a float64 model of the chain — no GPU, no compiled reference.

k_if_chain / k_if_chain_multi (radiosonde_auto_rx_amd/csrc/sonde_kernels.hip, if_chain_body) turn the IF-rate IQ stream y into the IF-filtered IQ z, the FM
stream and the sliced stream `bufs`.  What they compute, written as sums (demod_mod.c:639-648, 711-719, 771-775, 778-808; oracle/ora_dsp.c: ora_sample):

  z[m]      = sum_k w_iq[k] y[m - (T1-1) + k]                      zero history before the stream start; no IF low-pass: z = y
  fm_raw[m] = 0.8 atan2(Im w, Re w) / pi, w = z[m] conj(z[m-1])    z[-1] = 0; sample 0 is atan2 of signed zeros, formed in float32 as the reference forms it
  fm[m]     = sum_k w_fm[k] fm_raw[m - (T2-1) + k]                 with the FM low-pass, otherwise fm_raw
  X1,2[m]   = z[m] e^{-+i 2 pi f1 (m - m_start) / sr}              f1 = (-h sr) / (2 sps) with float32 h sr and sps, as ora_init forms them
  F1,2[m]   = sum of the last nwin = (int)sps terms of X1,2        terms before the stream start are 0
  bufs[m]   = (|F2| - |F1|) / sps                                  --iq0: bufs = fm

model() evaluates these in float64 with vectorised forms (convolution, prefix sums); literal() evaluates them term by term on given outputs —
tests/test_if_chain_cases_design.py holds the one to the other, the model to the CPU oracle and the table below to the library's own layout rule.

CASES: every row is there for a path of the kernel (column `why`).  T1, T2, nwin, layout and lds are CLAIMS: lds_rule() restates if_chain_lds /
if_chain_overlay of the kernel file, and the design test checks claim = restatement = sonde_if_chain_lds_bytes() of the built library, and T1 / T2 against
the oracle's consts.  A change of IF_TILE or IF_NB that moves a case off its edge fails there.
"""
import ctypes as C
import functools

import numpy as np

HEADER = "1011001110001101"          # 16 symbols: L = 16 sps <= 1280, so M = 8192 and the header search stays on its main path; random bits rarely match it
NBITS = 64
SECONDS = 0.15
IF_TILE, IF_THREADS, IF_NB, IF_RUN = 960, 256, 4, 4


def _case(id, sr, baud, iq, lp_iq, lp_fm, T1, T2, nwin, layout, lds, why, *, bt=0.5, h=0.6, lpiq_bw=7400, lpfm_bw=6000, bits=16, seconds=SECONDS, D=1):
    return dict(id=id, sr=sr, baud=float(baud), iq=iq, lp_iq=lp_iq, lp_fm=lp_fm, T1=T1, T2=T2, nwin=nwin, layout=layout, lds=lds, why=why,
                bt=bt, h=h, lpiq_bw=lpiq_bw, lpfm_bw=lpfm_bw, bits=bits, seconds=seconds, D=D)


CASES = [
    _case("rs41", 48_000, 4800, 2, True, False, 49, 1, 10, "B", 19624, "the shape the other stream tests run; T1 = 1 mod 4: 4-tap loop + 1-tap tail"),
    _case("rs41_50k_lpfm", 50_000, 4800, 2, True, True, 51, 101, 10, "B", 20432, "T1 = 3 mod 4: the 2-tap tail too; FM low-pass beside the tone sums"),
    _case("dfm", 48_000, 2500, 3, True, False, 49, 1, 19, "B", 19768, "DFM preset", h=1.8, lpiq_bw=12000, lpfm_bw=4000),
    _case("m10", 48_000, 9616, 2, True, False, 49, 1, 4, "B", 19528, "nwin close to IF_RUN", bt=1.8, h=0.9, lpiq_bw=24000, lpfm_bw=10000),
    _case("edge_B", 48_000, 768, 2, True, False, 49, 1, 62, "B", 20456, "nz - xlo == 1024: a thread's two passes through the low-pass touch exactly"),
    _case("edge_A", 48_000, 755, 2, True, False, 49, 1, 63, "A", 37336, "first nwin of layout A"),
    _case("edge_B3", 49_000, 810, 2, True, True, 49, 99, 60, "B", 21248, "T2 = 3 mod 4: xlo = T2 - 3; last nwin of layout B"),
    _case("edge_A3", 49_000, 797, 2, True, True, 49, 99, 61, "A", 41192, "first nwin of layout A for T2 = 3 mod 4"),
    _case("wide96", 96_000, 1200, 2, True, True, 97, 193, 80, "A", 46128, "96 kHz IF"),
    _case("wide192", 192_000, 2500, 2, True, True, 193, 385, 76, "A", 54832, "tile history longer than half a tile"),
    _case("iq0", 48_000, 4800, 0, True, True, 49, 97, 10, "A", 22344, "tone_on = 0: bufs is the filtered FM stream"),
    _case("nolp", 46_000, 4800, 2, False, False, 1, 1, 9, "B", 19416, "T1 == 1 branch (product, not sum)"),
    _case("zeros8", 48_000, 4800, 0, False, False, 1, 1, 10, "A", 19464, "8-bit samples 128 +- 2 LSB, 30 % exact zeros: the discriminator sees signed zeros", bits=8),
    _case("big", 384_000, 4800, 2, True, True, 385, 769, 80, "A", 72624, "above 64 KB of dynamic LDS: announced at create", seconds=0.05),
]
BY_ID = {c["id"]: c for c in CASES}
# base-rate engines (2.4 Msps -> 48 kHz, D = 50) with the presets of sonde="rs41" / "dfm" / "m10": the chain behind the decimator, `sr` is the IF rate
BASE_SR = 2_400_000
BASE = {
    "rs41": _case("base_rs41", 48_000, 4800, 5, True, False, 49, 1, 10, "B", 19624, "RS41 preset behind the decimator", D=50),
    "dfm": _case("base_dfm", 48_000, 2500, 5, True, False, 49, 1, 19, "B", 19768, "DFM preset behind the decimator", h=1.8, lpiq_bw=12000, lpfm_bw=4000, D=50),
    "m10": _case("base_m10", 48_000, 9615, 5, True, False, 49, 1, 4, "B", 19528, "M10 preset behind the decimator", bt=1.8, h=0.9, lpiq_bw=24000, lpfm_bw=10000, D=50),
}
REFUSED = dict(sr=1_500_000, baud=4800.0, lds=182720)               # 1.5 Msps IF with both low-passes: more LDS than a workgroup may have


def lds_rule(T1, T2, nwin, tone_on, fm_on):
    """-> (bytes of dynamic LDS of a full tile, layout "A" / "B"): if_chain_lds / if_chain_overlay / if_chain_xlo restated"""
    hz = (T2 - 1) + max(1, nwin - 1) + (IF_RUN - 1 if tone_on else 0)
    nz = hz + IF_TILE
    ny = nz + T1 - 1
    nsf = T2 - 1 + IF_TILE if fm_on else 0
    sy = ((ny + 2 * IF_NB + 1) & ~1) * 8
    sz = (nz + 1 if fm_on else 0) * 8
    tail = (T1 + T2) * 4 + 32
    xlo = (T2 - 1) & ~(IF_NB - 1)
    if tone_on and nz - xlo <= IF_NB * IF_THREADS:
        return max(sy + sz, ((nsf + 3) & ~3) * 4 + (nz - xlo) * 16) + tail, "B"
    return sy + sz + (nz if tone_on else 0) * 16 + nsf * 4 + tail, "A"


def generic_of(c, nbits=NBITS):
    """the `generic` dict of Engine(sonde="generic", ...) for a case"""
    return dict(header=HEADER, baud=c["baud"], bt=c["bt"], h=c["h"], symlen=1, symhd=1, hdmax=0, bitofs=0, nbits=nbits, lpiq_bw=c["lpiq_bw"], lpfm_bw=c["lpfm_bw"])


def engine_kw(c):
    """keyword arguments of Engine([0.0], sr, ...) for a case (iq 0 / 2 / 3 = --iq0 / --iq2 / --iq3: Engine's iq_mode 1 / 2 / 3)"""
    return dict(sonde="generic", generic=generic_of(c), iq_mode={0: 1, 2: 2, 3: 3}[c["iq"]], lp_iq=c["lp_iq"], lp_fm=c["lp_fm"], keep_soft=True, bits=c["bits"])


def oracle_kw(c):
    """keyword arguments of oracle.bind.ora_streams(x, sr, ...) for a case"""
    return dict(bps=c["bits"], iq_mode={0: 1, 2: 2, 3: 3}[c["iq"]], lp_iq=c["lp_iq"], lp_fm=c["lp_fm"], baud=c["baud"], bt=c["bt"], h=c["h"],
                lpiq_bw=c["lpiq_bw"], lpfm_bw=c["lpfm_bw"], hdr=HEADER.encode(), symlen=1, symhd=1)


# ----------------------------------------------------------------------------------------------- signal
@functools.lru_cache(maxsize=None)
def signal(cid, seed, n=None):
    """interleaved IQ of one channel: 2-FSK of random bits at the case's baud (deviation h baud / 2, amplitude 0.35), an interferer of amplitude 0.15
    at 0.23 cycles/sample, Gaussian noise of sigma 0.05; int16.  Case zeros8: uint8 samples 128 + {-2 .. 2}, 30 % of them exactly 128."""
    c = BY_ID[cid]
    sr = c["sr"]
    rng = np.random.default_rng(seed)
    if n is None:
        n = int(round(sr * c["seconds"]))
    if c["bits"] == 8:
        v = (128 + rng.choice([-2, -1, 0, 1, 2], 2 * n, p=[0.1, 0.25, 0.3, 0.25, 0.1])).astype(np.uint8)
    else:
        t = np.arange(n)
        bits = rng.integers(0, 2, int(n * c["baud"] / sr) + 2) * 2 - 1
        sym = bits[(t * c["baud"] / sr).astype(np.int64)]
        x = 0.35 * np.exp(2j * np.pi * np.cumsum(sym * (c["h"] * c["baud"] / 2.0) / sr))
        x += 0.15 * np.exp(2j * np.pi * 0.23 * t)
        x += 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        v = np.empty(2 * n)
        v[0::2], v[1::2] = x.real, x.imag
        v = np.clip(np.round(v * 32768.0), -32768, 32767).astype(np.int16)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def signal_base(kind, seed, fq, n_if=7200):
    """the same signal for a base-rate engine: BASE_SR int16 IQ, the 2-FSK carrier at fq cycles/sample, the interferer 0.23 cycles per IF sample beside it"""
    c = BASE[kind]
    n, sr = n_if * c["D"], BASE_SR
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    bits = rng.integers(0, 2, int(n * c["baud"] / sr) + 2) * 2 - 1
    sym = bits[(t * c["baud"] / sr).astype(np.int64)]
    x = 0.35 * np.exp(2j * np.pi * np.cumsum(fq + sym * (c["h"] * c["baud"] / 2.0) / sr))
    x += 0.15 * np.exp(2j * np.pi * (fq + 0.23 / c["D"]) * t)
    x += 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    v = np.empty(2 * n)
    v[0::2], v[1::2] = x.real, x.imag
    v = np.clip(np.round(v * 32768.0), -32768, 32767).astype(np.int16)
    v.setflags(write=False)
    return v


def samples_of(x, bits):
    """the chain's input of an IF-rate engine: the input samples as the float32 values the reference reads (x / 32768, (x - 128) / 128), complex float64"""
    v = np.asarray(x).astype(np.float64)
    v = (v - 128.0) / 128.0 if bits == 8 else v / 32768.0 if bits == 16 else v
    return v[0::2] + 1j * v[1::2]


# ----------------------------------------------------------------------------------------------- the reference's float32 designs
def _lowpass(f_lp, taps):
    from oracle import bind
    L = bind.lib()
    free = C.CDLL(None).free
    free.argtypes = [C.c_void_p]
    p = C.POINTER(C.c_float)()
    L.ora_lowpass_design.argtypes = [C.c_float, C.c_int, C.POINTER(C.POINTER(C.c_float))]
    assert L.ora_lowpass_design(float(np.float32(f_lp)), taps, C.byref(p)) == taps
    w = np.ctypeslib.as_array(p, (taps,)).astype(np.float64)
    free(p)
    return w


@functools.lru_cache(maxsize=None)
def _design(sr, baud, h, lp_iq, lp_fm, lpiq_bw, lpfm_bw, D):
    sr32 = np.float32(sr)
    w_iq = w_fm = None
    if lp_iq:                                                   # ora_init: (float)(lpiq_bw / (float)sr / 2.0), (int)(4 sr / 4e3) made odd
        taps = int(4 * sr / 4e3)
        w_iq = _lowpass(np.float32(np.float32(lpiq_bw) / sr32) / 2.0, taps + 1 - taps % 2)
    if lp_fm:                                                   # lpfm_bw / (float)sr, (int)(4 sr / 2e3) made odd
        taps = int(4 * sr / 2e3)
        w_fm = _lowpass(np.float32(lpfm_bw) / sr32, taps + 1 - taps % 2)
    sps = np.float32(np.float32(sr * D) / np.float32(baud))     # (float)sr / baud with the input rate, then /= (float)decM
    if D > 1:
        sps = np.float32(sps / np.float32(D))
    hs = np.float32(np.float32(-np.float32(h)) * sr32)          # float nh = -h; float hs = nh * sr
    f1 = float(hs) / (2.0 * float(sps))
    return w_iq, w_fm, float(sps), f1


def design(c):
    """-> (w_iq or None, w_fm or None, sps, f1): the reference's float32 taps, samples per symbol and tone frequency, as float64 values"""
    return _design(c["sr"], c["baud"], c["h"], c["lp_iq"], c["lp_fm"], c["lpiq_bw"], c["lpfm_bw"], c["D"])


def _fm0(z0):
    """sample 0 of the discriminator: the float32 product cmulf(z[0], (0, -0)) of oracle/ora_dsp.c, atan2 of its signed zeros"""
    re, im = np.float32(z0.real), np.float32(z0.imag)
    p0, m0 = np.float32(0.0), np.float32(-0.0)
    with np.errstate(all="ignore"):
        wr = np.float32(re * p0) - np.float32(im * m0)
        wi = np.float32(re * m0) + np.float32(im * p0)
    return float(np.float32(0.8 * np.arctan2(np.float64(wi), np.float64(wr)) / np.pi))


def _phasor(m, f1, sr):
    """e^{-i 2 pi f1 m / sr} from the phase reduced mod 1 in float64"""
    return np.exp(-2j * np.pi * np.mod(f1 * np.asarray(m, np.float64) / sr, 1.0))


# ----------------------------------------------------------------------------------------------- the model
def model(c, y, *, zero_last_tap=False, drop_term_every=0, m_start=0):
    """the chain of case c on the complex float64 input y from a stream start -> dict(ifiq [n, 2], fm [n], bufs [n]) in float64.
    m_start: sample the tone phase counts from (the stream start; another origin turns every term of a window by the same angle, which |F| does not see).
    Mutants for the design test: zero_last_tap = the last IF tap left out; drop_term_every = K: the outputs at multiples of K lose the oldest term of their window."""
    w_iq, w_fm, sps, f1 = design(c)
    y = np.asarray(y, np.complex128)
    n = len(y)
    z = y
    if w_iq is not None:
        w = w_iq.copy()
        if zero_last_tap:
            w[-1] = 0.0
        z = np.convolve(y, w[::-1])[:n]
    zp = np.concatenate([[0.0], z[:-1]])
    wv = z * np.conj(zp)
    fm = 0.8 * np.arctan2(wv.imag, wv.real) / np.pi
    fm[0] = _fm0(z[0])
    if w_fm is not None:
        fm = np.convolve(fm, w_fm[::-1])[:n]
    if c["iq"] == 0:
        bufs = fm
    else:
        nwin = int(sps)
        m = np.arange(n)
        ph = _phasor(m - m_start, f1, c["sr"])
        F = []
        for X in (z * ph, z * np.conj(ph)):
            cs = np.concatenate([[0.0], np.cumsum(X)])
            f = cs[1:] - cs[np.maximum(m + 1 - nwin, 0)]
            if drop_term_every:
                k = m[(m % drop_term_every == 0) & (m >= nwin - 1)]
                f[k] -= X[k - (nwin - 1)]
            F.append(f)
        bufs = (np.abs(F[1]) - np.abs(F[0])) / sps
    return dict(ifiq=np.stack([z.real, z.imag], axis=1), fm=fm, bufs=bufs)


def probes(n):
    """the first and last 16 outputs and +-8 around every multiple of 960 (tile) and of 1024 (a thread's second pass)"""
    s = set(range(16)) | set(range(n - 16, n))
    for k in (960, 1024):
        for m in range(k, n, k):
            s |= set(range(m - 8, m + 8))
    return np.array(sorted(m for m in s if 0 <= m < n))


def literal(c, y, ms):
    """the defining sums term by term at the outputs ms -> dict(ifiq [len(ms), 2], fm, bufs)"""
    w_iq, w_fm, sps, f1 = design(c)
    y = np.asarray(y, np.complex128)
    ms = np.asarray(ms, np.int64)
    T1 = 1 if w_iq is None else len(w_iq)
    T2 = 1 if w_fm is None else len(w_fm)
    nwin = int(sps)
    ypad = np.concatenate([np.zeros(T1 - 1, np.complex128), y])
    zs = {}

    def z_at(idx):                                              # z[m] = sum_k w[k] y[m - (T1-1) + k], one dot product per output; z[m < 0] = 0
        idx = np.asarray(idx, np.int64)
        new = np.array(sorted({int(i) for i in idx.ravel() if i >= 0 and int(i) not in zs}), np.int64)
        for a in range(0, len(new), 2048):
            part = new[a:a + 2048]
            rows = ypad[part[:, None] + np.arange(T1)[None, :]]
            val = rows[:, 0] if w_iq is None else (rows * w_iq[None, :]).sum(axis=1)
            zs.update(zip(part.tolist(), val.tolist()))
        return np.array([zs[int(i)] if i >= 0 else 0j for i in idx.ravel()], np.complex128).reshape(idx.shape)

    def fm_raw_at(idx):
        idx = np.asarray(idx, np.int64)
        wv = z_at(idx) * np.conj(z_at(idx - 1))
        v = 0.8 * np.arctan2(wv.imag, wv.real) / np.pi
        v = np.where(idx == 0, _fm0(z_at(np.array([0]))[0]), v)
        return np.where(idx < 0, 0.0, v)

    z = z_at(ms)
    if w_fm is None:
        fm = fm_raw_at(ms)
    else:
        fm = (fm_raw_at(ms[:, None] - (T2 - 1) + np.arange(T2)[None, :]) * w_fm[None, :]).sum(axis=1)
    if c["iq"] == 0:
        bufs = fm
    else:
        idx = ms[:, None] - np.arange(nwin)[None, :]
        zz = z_at(idx)
        ph = _phasor(np.maximum(idx, 0), f1, c["sr"])
        F1, F2 = (zz * ph).sum(axis=1), (zz * np.conj(ph)).sum(axis=1)
        bufs = (np.abs(F2) - np.abs(F1)) / sps
    return dict(ifiq=np.stack([z.real, z.imag], axis=1), fm=fm, bufs=bufs)


def rms(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a * a))) if a.size else 0.0


def figures(got, want):
    """-> {stream: (rms, max-abs)} of got - want over the streams both have"""
    out = {}
    for k in ("ifiq", "fm", "bufs"):
        if k in got and k in want:
            d = np.asarray(got[k], np.float64) - np.asarray(want[k], np.float64)
            out[k] = (rms(d), float(np.abs(d).max()))
    return out
