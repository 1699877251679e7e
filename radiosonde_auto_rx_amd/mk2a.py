"""ctypes mirror of include/sonde_mk2a.h: the LMS6-1680 / MkIIa engine (GPU, many channels per call) and its printer (host code).

    eng = Mk2aEngine(fqs, 240000, lp_iq=True, lpbw_hz=160000, dec_fm=4, dc=True)     # auto_rx: --iq fq --lpIQ --lpbw 160 --decFM --dc
    eng.process_host(x)           # x: (n_channels, n * 2) int16 IQ, n <= max_chunk, a multiple of dec_m
    eng.finish()                  # at the end of the input: the frame in progress is handed out as it is
    for f in eng.fetch_frames():  # {"channel", "bits", "mv", "df", "inv", "mv_pos", "sample"}
        text = printer.frame(f["bits"], f["mv"], f["df"])

Mk2aPrinter(json=True).frame(...) returns the characters the reference's mk2a1680mod prints for that frame."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._frame_engine import EngineHandle, PrinterHandle
from .engine import SondeError, lib

MAX_BITS = 1760


class Mk2aCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("sample_rate", "bits", "opt_iq", "lp_iq", "lpbw_hz", "lp_fm", "dec_fm", "dc", "min", "invert", "shift")] + \
               [("thres", C.c_float), ("baud", C.c_float), ("reserved", C.c_int32 * 7)]


class Mk2aInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("if_rate", "dec_m", "dec_fm", "L", "M", "K", "N", "taps_dec", "taps_iq", "taps_fm", "taps_iqfm")] + \
               [("sps", C.c_float), ("reserved", C.c_int32 * 8)]


class Mk2aFrame(C.Structure):
    _fields_ = [("channel", C.c_int32), ("nbits", C.c_int32), ("inv", C.c_int32), ("mv", C.c_float), ("df", C.c_double), ("mv_pos", C.c_uint32),
                ("reserved", C.c_uint32), ("sample", C.c_uint64), ("bits", C.c_uint8 * MAX_BITS)]


class Mk2aState(C.Structure):
    """sonde_mk2a_state_t: one channel's state between calls (testing tap)"""
    _fields_ = [(n, C.c_double) for n in ("df", "ddf", "dc", "sum_x", "sum_y", "f0")] + \
               [(n, C.c_uint64) for n in ("base", "if_samples", "out_samples", "n_start", "n_hdr")] + \
               [(n, C.c_float) for n in ("avg_x", "avg_y", "mv")] + [(n, C.c_uint32) for n in ("cnt", "maxcnt", "maxlim", "mv_pos")] + \
               [(n, C.c_int32) for n in ("lut_len", "locked", "mode", "inv", "buffered0", "bitpos")]


# testing taps (SONDE_MK2A_TAP_*): name -> (number, floats per sample)
TAPS = {"if": (0, 2), "zrot": (1, 2), "zlp": (2, 2), "fmr": (3, 1), "sraw": (4, 1), "bufs": (5, 1), "fmbuf": (6, 1)}


class Mk2aOpts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("raw", "crc", "vbs", "json", "jsn_freq_khz", "show_df", "if_rate", "sample_rate")] + \
               [("version", C.c_char * 32), ("reserved", C.c_int32 * 4)]


def _sigs(L):
    if getattr(L, "_mk2a_sigs", False):
        return L
    P = C.c_void_p
    L.sonde_mk2a_create.argtypes = [C.POINTER(Mk2aCfg), C.c_int32, C.POINTER(C.c_double), C.c_int32, C.POINTER(P)]
    L.sonde_mk2a_destroy.argtypes = [P]
    L.sonde_mk2a_destroy.restype = None
    L.sonde_mk2a_info.argtypes = [P, C.POINTER(Mk2aInfo)]
    L.sonde_mk2a_design.argtypes = [C.POINTER(Mk2aCfg), C.POINTER(Mk2aInfo)]
    L.sonde_mk2a_process_host.argtypes = [P, P, C.c_int32]
    L.sonde_mk2a_process_device.argtypes = [P, P, C.c_int32]
    L.sonde_mk2a_finish.argtypes = [P]
    L.sonde_mk2a_fetch_frames.argtypes = [P, C.POINTER(Mk2aFrame), C.c_int32]
    L.sonde_mk2a_read_tap.argtypes = [P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, P]
    L.sonde_mk2a_read_state.argtypes = [P, C.c_int32, C.POINTER(Mk2aState)]
    L.sonde_mk2a_printer_create.argtypes = [C.POINTER(Mk2aOpts), C.POINTER(P)]
    L.sonde_mk2a_printer_destroy.argtypes = [P]
    L.sonde_mk2a_printer_destroy.restype = None
    L.sonde_mk2a_print_frame.argtypes = [P, C.POINTER(C.c_uint8), C.c_int32, C.c_float, C.c_double, C.c_char_p, C.c_size_t]
    L.sonde_mk2a_crc16.argtypes = [C.POINTER(C.c_uint8), C.c_int32]
    L._mk2a_sigs = True
    return L


def crc16(data: bytes) -> int:
    b = (C.c_uint8 * max(1, len(data))).from_buffer_copy(bytes(data) or b"\0")
    return _sigs(lib()).sonde_mk2a_crc16(b, len(data))


def _cfg(sr, bits, opt_iq, lp_iq, lpbw_hz, lp_fm, dec_fm, dc, min, invert, shift, thres, baud):
    return Mk2aCfg(sample_rate=sr, bits=bits, opt_iq=opt_iq, lp_iq=int(lp_iq), lpbw_hz=int(lpbw_hz), lp_fm=int(lp_fm), dec_fm=int(dec_fm), dc=int(dc),
                   min=int(min), invert=int(invert), shift=int(shift), thres=float(thres), baud=float(baud))


def design(sr: int, *, bits: int = 16, opt_iq: int = 6, lp_iq: bool = True, lpbw_hz: int = 0, lp_fm: bool = False, dec_fm: int = 0, dc: bool = False,
           min: bool = False, invert: bool = False, shift: int = 0, thres: float = 0.0, baud: float = 0.0) -> dict:
    """the rates, tap counts and window sizes init_buffers_Lband derives for that configuration (host code, no GPU)"""
    L = _sigs(lib())
    cfg, inf = _cfg(sr, bits, opt_iq, lp_iq, lpbw_hz, lp_fm, dec_fm, dc, min, invert, shift, thres, baud), Mk2aInfo()
    rc = L.sonde_mk2a_design(C.byref(cfg), C.byref(inf))
    if rc:
        raise SondeError(rc, "sonde_mk2a_design")
    return {n: getattr(inf, n) for n, _ in Mk2aInfo._fields_ if n != "reserved"}


def _frame_dict(f) -> dict:
    return {"channel": f.channel, "sample": int(f.sample), "mv": float(f.mv), "df": float(f.df), "inv": f.inv, "mv_pos": f.mv_pos,
            "bits": np.frombuffer(bytes(f.bits), np.uint8)[:f.nbits].copy()}


class Mk2aPrinter(PrinterHandle):
    """frame bits -> the reference's text / -r / -v.. / JSON lines (host code, no GPU)."""
    _prefix = "sonde_mk2a"

    def __init__(self, *, raw: bool = False, crc: bool = False, vbs: int = 0, json: bool = False, jsn_freq_khz: int = 0, show_df: bool = False,
                 if_rate: int = 240000, sample_rate: int = 240000, version: str = ""):
        o = Mk2aOpts(raw=int(raw), crc=int(crc), vbs=int(vbs), json=int(json), jsn_freq_khz=int(jsn_freq_khz), show_df=int(show_df),
                     if_rate=int(if_rate), sample_rate=int(sample_rate), version=version.encode())
        self._open_printer(_sigs(lib()), o, 1 << 16)

    def frame(self, bits, mv: float = 0.0, df: float = 0.0) -> str:
        b = np.ascontiguousarray(bits, dtype=np.uint8)
        return self._print("latin-1", b.ctypes.data_as(C.POINTER(C.c_uint8)), len(b), mv, df)


class Mk2aEngine(EngineHandle):
    """k_mk2a_mix + k_mk2a behind sonde_mk2a_create: one channel per entry of fqs, all at sample rate sr."""
    _prefix, _Frame, _frame_dict = "sonde_mk2a", Mk2aFrame, staticmethod(_frame_dict)

    def __init__(self, fqs, sr: int, *, bits: int = 16, opt_iq: int = 6, lp_iq: bool = True, lpbw_hz: int = 160000, lp_fm: bool = False, dec_fm: int = 4,
                 dc: bool = True, min: bool = False, invert: bool = False, shift: int = 0, thres: float = 0.0, baud: float = 0.0,
                 max_chunk: int | None = None):
        self.n_ch = len(fqs)
        self.bits = bits
        self.max_chunk = int(max_chunk or sr // 4)
        cfg = _cfg(sr, bits, opt_iq, lp_iq, lpbw_hz, lp_fm, dec_fm, dc, min, invert, shift, thres, baud)
        fq = (C.c_double * self.n_ch)(*[float(f) for f in fqs])
        self._open(_sigs(lib()), "create", C.byref(cfg), self.n_ch, fq, self.max_chunk, nbuf=32)
        inf = Mk2aInfo()
        self._L.sonde_mk2a_info(self._h, C.byref(inf))
        self.info = {n: getattr(inf, n) for n, _ in Mk2aInfo._fields_ if n != "reserved"}
        self.if_rate, self.dec_m = inf.if_rate, inf.dec_m

    @staticmethod
    def dec_m_of(sr: int) -> int:
        """the decimation the front end applies to an input rate (calls take whole multiples of it)"""
        return design(sr)["dec_m"]

    def process_host(self, x: np.ndarray):
        dt = np.int16 if self.bits == 16 else np.uint8
        x = np.ascontiguousarray(x, dtype=dt).reshape(self.n_ch, -1)
        self._call("process_host", self._h, x.ctypes.data, x.shape[1] // 2)

    finish = EngineHandle._finish

    def read_tap(self, channel: int, tap: str, first: int, count: int) -> np.ndarray:
        """testing tap: `count` samples of TAPS[tap] from absolute sample `first` (IF rate; output rate for bufs / fmbuf), which must still
        be inside the ring ("if": inside the last call).  complex64 for the IQ taps, float32 otherwise"""
        num, width = TAPS[tap]
        out = np.empty(count * width, np.float32)
        self._call("read_tap", self._h, channel, num, first, count, out.ctypes.data)
        return out.view(np.complex64) if width == 2 else out

    def read_state(self, channel: int = 0) -> dict:
        """testing tap: the channel's state record between calls"""
        st = Mk2aState()
        self._call("read_state", self._h, channel, C.byref(st))
        return {n: getattr(st, n) for n, _ in Mk2aState._fields_}
