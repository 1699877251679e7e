"""ctypes binding of the spectrum survey and peak pick in libsonde_hip.so (include/sonde_power.h).

Python mirror of auto_rx's first step: `get_power_spectrum` (autorx/sdr_wrappers.py:571-766, the rtl_power call and its log reader) becomes
`PowerSurvey.fetch()`, and the peak pick of `SondeScanner.sonde_search` (autorx/scan.py:1007-1063) becomes `pick_peaks`.  No CPU fallback for the
spectrum: the constructor raises without the in-tree HIP library / a GPU.  `pick_peaks` and `csv_line` are host code and need neither.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .engine import ABI_VERSION, _chk, lib

RECT, HANN = 0, 1
FLOOR_DB = -200.0


class PowerCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "device", "n_streams", "sample_rate", "bits", "nfft", "window", "max_chunk")] + \
               [("center_hz", C.c_double), ("crop", C.c_float), ("reserved", C.c_int32 * 3)]


class PowerInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("nfft", "bins", "threads", "lds_bytes", "workgroups_per_cu", "max_workgroups")] + \
               [("step_hz", C.c_double), ("window_sum", C.c_double), ("reserved", C.c_int32 * 4)]


_proto_done = False


def _lib():
    global _proto_done
    L = lib()
    if not _proto_done:
        D = C.POINTER(C.c_double)
        L.sonde_power_create.argtypes = [C.POINTER(PowerCfg), C.POINTER(C.c_void_p)]
        L.sonde_power_destroy.argtypes = [C.c_void_p]
        L.sonde_power_info.argtypes = [C.c_void_p, C.POINTER(PowerInfo)]
        L.sonde_power_reset.argtypes = [C.c_void_p]
        L.sonde_power_process_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
        L.sonde_power_process_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
        L.sonde_power_segments.argtypes = [C.c_void_p, C.c_int32]
        L.sonde_power_segments.restype = C.c_int64
        L.sonde_power_fetch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, D, D, D, C.c_int32, C.c_int]
        L.sonde_power_kernel_ms.argtypes = [C.c_void_p, C.c_char_p, D, C.POINTER(C.c_int64)]
        L.sonde_power_peaks.argtypes = [C.c_void_p, C.c_int32] + [C.c_double] * 8 + [C.c_void_p, C.c_int32, C.c_int32, D, C.c_void_p, C.c_int32]
        L.sonde_power_csv_line.argtypes = [C.c_int64, C.c_double, C.c_double, C.c_double, C.c_int64, C.c_void_p, C.c_int32, C.c_char_p, C.c_size_t]
        _proto_done = True
    return L


class PowerSurvey:
    """Averaged periodogram of n_streams wideband IQ streams on one GPU: `rtl_power -f ... -i ... -c crop` for a stream that is already there."""

    def __init__(self, sample_rate: int, nfft: int, *, center_hz: float = 0.0, n_streams: int = 1, bits: int = 16, window: int | str = RECT,
                 crop: float = 0.0, max_chunk: int | None = None, device: int = 0):
        if isinstance(window, str):
            window = {"rect": RECT, "rectangular": RECT, "hann": HANN}[window.lower()]
        self.sample_rate, self.nfft, self.n_streams, self.bits = sample_rate, nfft, n_streams, bits
        self._dtype = {8: np.uint8, 32: np.float32}.get(bits, np.int16)
        cfg = PowerCfg(ABI_VERSION, device, n_streams, sample_rate, bits, nfft, window, max_chunk or sample_rate, center_hz, crop)
        h = C.c_void_p()
        _chk(_lib().sonde_power_create(C.byref(cfg), C.byref(h)))
        self._h = h
        info = PowerInfo()
        _chk(_lib().sonde_power_info(h, C.byref(info)))
        self.info = {n: getattr(info, n) for n, _ in PowerInfo._fields_ if n != "reserved"}

    def close(self):
        if getattr(self, "_h", None):
            _lib().sonde_power_destroy(self._h)
            self._h = None

    __del__ = close

    def process_host(self, x: np.ndarray):
        """x: int16 (bits=8: uint8, bits=32: float32) [n_streams, 2*n] interleaved I/Q, or [2*n] for one stream."""
        x = np.ascontiguousarray(x, dtype=self._dtype)
        if x.ndim == 1:
            x = x[None, :]
        assert x.shape[0] == self.n_streams
        n = x.shape[1] // 2
        _chk(_lib().sonde_power_process_host(self._h, x.ctypes.data_as(C.c_void_p), x.shape[1] // 2, n))

    def process_device(self, ptr: int, stream_stride: int, n: int):
        """ptr: device address of stream 0; stream c starts stream_stride complex samples behind stream c - 1.  Queued on the survey's stream."""
        _chk(_lib().sonde_power_process_device(self._h, C.c_void_p(ptr), stream_stride, n))

    def segments(self, stream: int = 0) -> int:
        return _chk(_lib().sonde_power_segments(self._h, stream))

    def reset(self):
        _chk(_lib().sonde_power_reset(self._h))

    def fetch(self, stream: int = 0, reset: bool = False):
        """-> (freq [Hz], power [dB], step [Hz]) as auto_rx's get_power_spectrum returns them: float64 arrays over the kept bins, ascending."""
        db = np.zeros(self.info["bins"], np.float32)
        lo, hi, step = C.c_double(0), C.c_double(0), C.c_double(0)
        k = _chk(_lib().sonde_power_fetch(self._h, stream, db.ctypes.data_as(C.c_void_p), C.byref(lo), C.byref(hi), C.byref(step), len(db), int(reset)))
        return np.linspace(lo.value, hi.value, k), db[:k].astype(np.float64), step.value

    def kernel_ms(self, name: str = "k_power"):
        ms, n = C.c_double(0), C.c_int64(0)
        _chk(_lib().sonde_power_kernel_ms(self._h, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value


def pick_peaks(freq, power, step, *, snr_threshold: float = 10.0, min_distance: float = 1000.0, quantization: float = 10000.0,
               min_freq: float = 400.05, max_freq: float = 403.0, never_scan=(), max_peaks: int = 10, return_floor: bool = False):
    """auto_rx's peak pick (scan.py:1007-1063) with its own parameter names and units: min_freq / max_freq / never_scan in MHz, the rest in Hz / dB.
    freq must be what the survey (or auto_rx's log reader) returns: linspace(freq[0], freq[-1], len(freq)).  -> peak frequencies [Hz] in auto_rx's
    order (by power, descending); with return_floor also the noise floor it thresholds against."""
    power = np.ascontiguousarray(power, dtype=np.float64)
    freq = np.asarray(freq, dtype=np.float64)
    assert len(freq) == len(power)
    never = np.ascontiguousarray(np.array(list(never_scan), dtype=np.float64) * 1e6)
    out = np.zeros(max(1, len(power)), np.float64)
    nf = C.c_double(0)
    f0, f1 = (float(freq[0]), float(freq[-1])) if len(freq) else (0.0, 0.0)
    k = _chk(_lib().sonde_power_peaks(power.ctypes.data_as(C.c_void_p), len(power), f0, f1, float(step), float(snr_threshold), float(min_distance),
                                      float(quantization), min_freq * 1e6, max_freq * 1e6, never.ctypes.data_as(C.c_void_p), len(never), int(max_peaks),
                                      C.byref(nf), out.ctypes.data_as(C.c_void_p), len(out)))
    pk = out[:k].copy()
    return (pk, nf.value) if return_floor else pk


def csv_line(unix_time: int, freq_low: float, freq_high: float, step: float, samples: int, power) -> str:
    """One rtl_power log line for the spectrum (what auto_rx's read_rtl_power_log / read_rtl_power parse)."""
    db = np.ascontiguousarray(power, dtype=np.float32)
    n = _lib().sonde_power_csv_line(int(unix_time), freq_low, freq_high, step, int(samples), db.ctypes.data_as(C.c_void_p), len(db), None, 0)
    buf = C.create_string_buffer(_chk(n) + 1)
    _chk(_lib().sonde_power_csv_line(int(unix_time), freq_low, freq_high, step, int(samples), db.ctypes.data_as(C.c_void_p), len(db), buf, len(buf)))
    return buf.value.decode()
