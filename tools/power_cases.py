"""Fixtures of the spectrum survey shared by tools/make_golden_power.py and the tests: the seeded captures, the float64 reference periodogram,
the random peak-pick cases, and a driver that runs auto_rx's OWN peak-pick lines (SondeScanner.sonde_search, autorx/scan.py:1007-1063, with
autorx/utils.py detect_peaks) on a given spectrum — the reference's text is executed where it lies, none of it is restated here."""
from __future__ import annotations

import os
import sys
import threading
import types

import numpy as np

from tools import synth

AUTORX = "/root/reference/auto_rx"
SR = 2_400_000
CENTER_HZ = 402.0e6
CROP = 0.25
FLOOR_DB = -200.0
RECT, HANN = 0, 1

# spectrum cases: name -> (nfft, window, bits, complex samples, first sample of the capture)
SPECTRA = {
    "n256_rect_cs16": (256, RECT, 16, 5 * 256 + 37, 200_000),
    "n4096_hann_cu8": (4096, HANN, 8, 4 * 4096 + 100, 150_000),
    "n16384_hann_cs16": (16384, HANN, 16, 3 * 16384 + 11, 130_000),
    "n1024_rect_cf32": (1024, RECT, 32, 6 * 1024 + 5, 250_000),
}
# peak fixtures (whole capture, crop 25 %): name -> (nfft, window, capture seed, snr_threshold, min_distance)
PEAKS = {
    "n256_rect": (256, RECT, 3, 9.0, 1000.0),
    "n4096_hann": (4096, HANN, 8, 8.0, 5000.0),
    "n16384_hann": (16384, HANN, 2, 9.0, 5000.0),
}
PICK = dict(quantization=10000.0, min_freq=400.05, max_freq=403.0, max_peaks=10)
SIGNALS = [dict(kind="rs41", fq=203_400 / SR, amp=0.10), dict(kind="dfm", fq=-700_600 / SR, amp=0.08), dict(kind="m10", fq=861_000 / SR, amp=0.06)]

_captures = {}


def capture(seed: int = 1) -> np.ndarray:
    """int16 interleaved IQ, 0.25 s at 2.4 Msps: RS41 +203.4 kHz, DFM -700.6 kHz, M10 +861 kHz over noise 0.01 (computed once per seed)."""
    if seed not in _captures:
        x = synth.wideband_capture(SR, 0.25, SIGNALS, noise_sigma=0.01, seed=seed)
        x.setflags(write=False)
        _captures[seed] = x
    return _captures[seed]


def as_bits(x16: np.ndarray, bits: int) -> np.ndarray:
    """the same stream in the family's other input formats: cu8 = high byte + 128, cf32 = x / 32768 * 1.5"""
    if bits == 16:
        return x16
    if bits == 8:
        return ((x16.astype(np.int32) >> 8) + 128).astype(np.uint8)
    return (x16.astype(np.float32) / np.float32(32768.0) * np.float32(1.5)).astype(np.float32)


def spectrum_input(name: str) -> np.ndarray:
    nfft, window, bits, n, first = SPECTRA[name]
    return as_bits(capture(1)[2 * first:2 * (first + n)], bits)


def to_complex(x: np.ndarray, bits: int, dtype=np.complex128) -> np.ndarray:
    """the family's conversion: cs16 / 32768, (cu8 - 128) / 128, cf32 as it is"""
    v = x.astype(np.float64)
    if bits == 16:
        v = v / 32768.0
    elif bits == 8:
        v = (v - 128.0) / 128.0
    return (v[0::2] + 1j * v[1::2]).astype(dtype)


def window_weights(nfft: int, window: int) -> np.ndarray:
    return np.ones(nfft) if window == RECT else 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(nfft) / nfft)


def ref_power(x: np.ndarray, bits: int, nfft: int, window: int, single: bool = False) -> np.ndarray:
    """mean |X|^2 / (sum w)^2 over the whole segments of x, linear, in transform order.  single: the same in complex64 (numpy's float32 FFT),
    the yardstick the goldens record beside the float64 value."""
    z = to_complex(x, bits, np.complex64 if single else np.complex128)
    w = window_weights(nfft, window)
    nseg = len(z) // nfft
    seg = z[:nseg * nfft].reshape(nseg, nfft)
    if single:
        X = np.fft.fft(seg * w.astype(np.float32))
        assert X.dtype == np.complex64
        p = (X.real.astype(np.float32) ** 2 + X.imag.astype(np.float32) ** 2).astype(np.float64)
    else:
        X = np.fft.fft(seg * w)
        p = X.real ** 2 + X.imag ** 2
    return p.mean(axis=0) / w.sum() ** 2


def shift_crop_db(p: np.ndarray, crop: float = 0.0):
    """transform order -> (kept bins in ascending frequency [dB], first kept bin's offset from the centre in bins)"""
    n = len(p)
    drop = int(crop * n / 2.0)
    q = np.fft.fftshift(p)[drop:n - drop]
    db = np.full(len(q), FLOOR_DB)
    db[q > 0] = np.maximum(10.0 * np.log10(q[q > 0]), FLOOR_DB)
    return db, drop - n // 2


def bin_freqs(nfft: int, crop: float, center_hz: float = CENTER_HZ, sr: int = SR):
    drop = int(crop * nfft / 2.0)
    step = sr / nfft
    return center_hz + (drop - nfft // 2) * step, center_hz + (nfft - drop - 1 - nfft // 2) * step, step


# ---- auto_rx, executed where it lies

def autorx_modules():
    """-> (autorx.scan, autorx.sdr_wrappers, autorx.utils), or None where the reference is not present"""
    if not os.path.isdir(AUTORX):
        return None
    sys.modules.setdefault("semver", types.ModuleType("semver"))      # the one import of autorx.utils this image lacks (version check of its updater)
    if AUTORX not in sys.path:
        sys.path.insert(0, AUTORX)
    import autorx.scan
    import autorx.sdr_wrappers
    import autorx.utils
    return autorx.scan, autorx.sdr_wrappers, autorx.utils


def autorx_pick(scan_mod, freq, power, step, *, snr_threshold, min_distance, quantization, min_freq, max_freq, never_scan, max_peaks):
    """Run SondeScanner.sonde_search on (freq, power, step): its spectrum source and its detector are replaced, everything between them — the
    peak pick — is the reference's own code.  -> (peak frequencies in the order it would try them, noise floor)"""
    tried = []
    s = object.__new__(scan_mod.SondeScanner)
    for k, v in dict(only_scan=[], always_scan=[], sdr_type="RTLSDR", min_freq=min_freq, max_freq=max_freq, search_step=step, scan_dwell_time=1,
                     rtl_device_idx="0", rtl_power_path="rtl_power", rtl_fm_path="rtl_fm", ppm=0, gain=-1, bias=False, sdr_hostname="", sdr_port=0,
                     ss_power_path="", ss_iq_path="", sonde_scanner_running=True, snr_threshold=snr_threshold, min_distance=min_distance,
                     quantization=quantization, never_scan=list(never_scan), max_peaks=max_peaks, temporary_block_list={},
                     temporary_block_list_lock=threading.Lock(), temporary_block_time=60, detect_dwell_time=1, save_detection_audio=False,
                     wideband_sondes=False, rs_path="./", max_async_scan_workers=1).items():
        setattr(s, k, v)
    for m in ("log_debug", "log_info", "log_error", "log_warning"):
        setattr(s, m, lambda *a, **kw: None)
    saved = {k: getattr(scan_mod, k) for k in ("get_power_spectrum", "detect_sonde", "flask_emit_event")}
    scan_mod.get_power_spectrum = lambda **kw: (np.array(freq, dtype=np.float64), np.array(power, dtype=np.float64), step)
    scan_mod.detect_sonde = lambda f, **kw: (tried.append(f), (None, 0.0))[1]
    scan_mod.flask_emit_event = lambda *a, **kw: None
    try:
        with np.errstate(all="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                s.sonde_search(first_only=False)
    finally:
        for k, v in saved.items():
            setattr(scan_mod, k, v)
    return np.array(tried, dtype=np.float64), float(scan_mod.scan_result["threshold"])


# ---- random peak-pick cases

def random_case(rng: np.random.Generator, i: int) -> dict:
    """One spectrum with its pick parameters.  The draw cycles through the shapes the pick has branches for: n < 3, even and odd counts (median),
    plateaus, NaNs, peaks on the first / last two bins, nothing above the threshold, never_scan hits, max_peaks truncation, range edges inside the
    band, min_distance below / at / above one bin, quantisation steps that put bins exactly half way (round half to even).  Values are continuous
    draws, so no two local maxima tie (np.argsort on ties has no defined answer); plateaus repeat a value on ADJACENT bins only."""
    kind = i % 12
    n = int(rng.choice([1, 2])) if kind == 0 else int(rng.integers(3, 7)) if kind == 1 else int(rng.integers(20, 400))
    step = float(rng.choice([585.9375, 146.484375, 800.0, 1000.0, 9375.0, 2343.75]))
    f_low = 400.0e6 + float(rng.integers(0, 5000)) * step
    f_high = f_low + (n - 1) * step
    power = -70.0 + 1.5 * rng.standard_normal(n)
    npk = 0 if kind == 2 else int(rng.integers(1, 9))
    centres = []
    for _ in range(npk if n >= 3 else 0):
        c = int(rng.integers(0, n))
        if kind == 3:
            c = int(rng.choice([0, 1, n - 2, n - 1]))
        centres.append(c)
        h, wd = float(rng.uniform(4.0, 40.0)), float(rng.uniform(0.6, 6.0))
        power += h * np.exp(-0.5 * ((np.arange(n) - c) / wd) ** 2)
    if kind == 4 and n >= 6:                                       # plateaus: a maximum repeated on the next one or two bins
        for c in centres + [int(rng.integers(1, n - 3))]:
            c = min(max(c, 1), n - 3)
            power[c + 1] = power[c]
            if rng.random() < 0.5:
                power[c + 2] = power[c]
    if kind == 5 and n >= 3:                                       # NaNs, as rtl_power occasionally writes them
        power[rng.integers(0, n, size=int(rng.integers(1, 4)))] = np.nan
    quant = float(rng.choice([10000.0, 5000.0, 25000.0, 1000.0, 2.0 * step]))
    snr = float(rng.uniform(3.0, 15.0)) if kind != 2 else 60.0
    mind = float(rng.choice([1000.0, 5000.0, step, 0.5 * step, 2.5 * step, 20.0 * step, 3.0 * step]))
    lo_mhz, hi_mhz = 100.0, 1000.0
    if kind in (6, 7) and n >= 3:                                  # range edges inside the band, on the q/2 grid the mask compares against
        a = np.round((f_low + rng.uniform(0.2, 0.8) * (f_high - f_low)) / (quant / 2.0)) * (quant / 2.0)
        if kind == 6:
            lo_mhz = float(a) / 1e6
        else:
            hi_mhz = float(a) / 1e6
    never = []
    if kind == 8 and centres:                                      # never_scan: on a peak, just inside and just outside q/2 of one
        f = f_low + centres[0] * step
        never = [float(np.round(f / quant) * quant) / 1e6, (f + 0.49 * quant) / 1e6, (f_low - 5 * quant) / 1e6]
        if len(centres) > 1:
            never.append((f_low + centres[1] * step + 0.51 * quant) / 1e6)
    max_peaks = int(rng.choice([0, 1, 2, 3])) if kind == 9 else int(rng.choice([10, 100]))
    return dict(power=power, f_low=f_low, f_high=f_high, step=step, snr_threshold=snr, min_distance=mind, quantization=quant,
                min_freq=lo_mhz, max_freq=hi_mhz, never_scan=never, max_peaks=max_peaks)


def case_kwargs(c: dict) -> dict:
    return {k: c[k] for k in ("snr_threshold", "min_distance", "quantization", "min_freq", "max_freq", "never_scan", "max_peaks")}


def local_maxima(power: np.ndarray) -> np.ndarray:
    """indices i with power[i-1] < power[i] >= power[i+1] (what a rising-edge peak detector can return)"""
    p = np.asarray(power, dtype=np.float64)
    return 1 + np.where((p[1:-1] > p[:-2]) & (p[1:-1] >= p[2:]))[0]
