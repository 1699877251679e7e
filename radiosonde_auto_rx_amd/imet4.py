"""ctypes mirror of include/sonde_imet4.h: the iMet-4 / iMet-1-RS engine (GPU, many channels per call) and its printer (host code).

    eng = Imet4Engine(fqs, sr, bits=16, iq=True, lp_iq=True, dc=True)      # the auto_rx IMET form: --iq 0.0 --lpIQ --dc - 48000 16
    eng.process_host(x)           # x: (n_channels, n * 2) int16 IQ (or (n_channels, n) for FM audio), n <= max_chunk, a multiple of dec_m;
                                  # bits=8: uint8, bits=32: float32 taken as it is
    for f in eng.fetch_frames():  # {"channel", "sample", "bits"}
        text = printer.frame(f["bits"])

Imet4Printer(json=True).frame(bits) returns the characters the reference's imet4iq prints for that frame.

Channels at run time (ChannelizedReceiver): release_channel(c) takes a channel out of the launches, restart_channel(c, fq) makes it a fresh
channel at a new fq, process_device(ptr, n, ch_stride=...) reads rows of a staging array."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._frame_engine import EngineHandle, PrinterHandle
from .engine import SondeError, lib

FRAME_BITS = 1000


class Imet4Cfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("sample_rate", "bits", "iq", "lp_iq", "lpbw_hz", "lp_fm", "dc", "min", "imet1")] + \
               [("reserved", C.c_int32 * 7)]


class Imet4Frame(C.Structure):
    _fields_ = [("channel", C.c_int32), ("nbits", C.c_int32), ("sample", C.c_uint64), ("bits", C.c_uint8 * FRAME_BITS)]


class Imet4Opts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("raw", "rawbits", "json", "jsn_freq_khz")] + [("version", C.c_char * 32), ("reserved", C.c_int32 * 4)]


class Imet4State(C.Structure):
    """sonde_imet4_state_t: one channel's state between calls (testing tap)"""
    _fields_ = [(n, C.c_double) for n in ("df", "dc", "sum_x", "sum_y", "f0", "f1_re", "f1_im", "f2_re", "f2_im", "pos_bit")] + \
               [(n, C.c_uint64) for n in ("sample_hi", "base")] + \
               [(n, C.c_float) for n in ("xsum", "avg_x", "avg_y", "prev_re", "prev_im")] + \
               [(n, C.c_uint32) for n in ("sample", "pre_pos", "cnt", "maxcnt", "maxlim", "hreg")] + \
               [(n, C.c_int32) for n in ("lut_len", "locked", "bit0", "pos", "hf", "bitpos", "hcount", "bb0", "bb1", "bb2")]


# testing taps (SONDE_IMET4_TAP_*): name -> (number, floats per sample)
TAPS = {"if": (0, 2), "zring": (1, 2), "fmring": (2, 1), "xring": (3, 1)}


def _sigs(L):
    if getattr(L, "_imet4_sigs", False):
        return L
    P = C.c_void_p
    L.sonde_imet4_create.argtypes = [C.POINTER(Imet4Cfg), C.c_int32, C.POINTER(C.c_double), C.c_int32, C.POINTER(P),
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.sonde_imet4_destroy.argtypes = [P]
    L.sonde_imet4_destroy.restype = None
    L.sonde_imet4_process_host.argtypes = [P, P, C.c_int32]
    L.sonde_imet4_process_device.argtypes = [P, P, C.c_int32]
    L.sonde_imet4_process_device_strided.argtypes = [P, P, C.c_int64, C.c_int32]
    L.sonde_imet4_restart_channel.argtypes = [P, C.c_int32, C.c_double]
    L.sonde_imet4_release_channel.argtypes = [P, C.c_int32]
    L.sonde_imet4_channel_active.argtypes = [P, C.c_int32]
    L.sonde_imet4_fetch_frames.argtypes = [P, C.POINTER(Imet4Frame), C.c_int32]
    L.sonde_imet4_read_tap.argtypes = [P, C.c_int32, C.c_int32, C.c_int64, C.c_int32, P]
    L.sonde_imet4_read_state.argtypes = [P, C.c_int32, C.POINTER(Imet4State)]
    L.sonde_imet4_tap_ring.argtypes = [P]
    L.sonde_imet4_printer_create.argtypes = [C.POINTER(Imet4Opts), C.POINTER(P)]
    L.sonde_imet4_printer_destroy.argtypes = [P]
    L.sonde_imet4_printer_destroy.restype = None
    L.sonde_imet4_print_frame.argtypes = [P, C.POINTER(C.c_uint8), C.c_int32, C.c_char_p, C.c_size_t]
    L.sonde_imet4_crc16.argtypes = [C.POINTER(C.c_uint8), C.c_int32]
    L._imet4_sigs = True
    return L


def crc16(data: bytes) -> int:
    b = (C.c_uint8 * max(1, len(data))).from_buffer_copy(bytes(data) or b"\0")
    return _sigs(lib()).sonde_imet4_crc16(b, len(data))


def _frame_dict(f) -> dict:
    return {"channel": f.channel, "sample": int(f.sample), "bits": np.frombuffer(bytes(f.bits), np.uint8)[:f.nbits].copy()}


class Imet4Printer(PrinterHandle):
    """bits -> the reference's text / -r / --rawbits / JSON lines (host code, no GPU)."""
    _prefix = "sonde_imet4"

    def __init__(self, *, raw: bool = False, rawbits: bool = False, json: bool = False, jsn_freq_khz: int = 0, version: str = ""):
        o = Imet4Opts(raw=int(raw), rawbits=int(rawbits), json=int(json), jsn_freq_khz=int(jsn_freq_khz), version=version.encode())
        self._open_printer(_sigs(lib()), o, 1 << 16)

    def frame(self, bits) -> str:
        b = np.ascontiguousarray(bits, dtype=np.uint8)
        return self._print("latin-1", b.ctypes.data_as(C.POINTER(C.c_uint8)), len(b))


class Imet4Engine(EngineHandle):
    """k_imet4_afsk behind sonde_imet4_create: one channel per entry of fqs (ignored for FM audio), all at sample rate sr."""
    _prefix, _Frame, _frame_dict = "sonde_imet4", Imet4Frame, staticmethod(_frame_dict)

    def __init__(self, fqs, sr: int, *, bits: int = 16, iq: bool = True, lp_iq: bool = True, lpbw_hz: int = 0, lp_fm: bool = False,
                 dc: bool = True, min: bool = False, imet1: bool = False, max_chunk: int | None = None):
        self._L = _sigs(lib())
        self.n_ch = len(fqs)
        self.iq, self.bits = bool(iq), bits
        self.max_chunk = int(max_chunk or sr // 4)
        cfg = Imet4Cfg(sample_rate=sr, bits=bits, iq=int(iq), lp_iq=int(lp_iq), lpbw_hz=int(lpbw_hz), lp_fm=int(lp_fm), dc=int(dc),
                       min=int(min), imet1=int(imet1))
        fq = (C.c_double * self.n_ch)(*[float(f) for f in fqs])
        self._h, self._buf = C.c_void_p(), (Imet4Frame * 64)()
        ifr, dec = C.c_int32(), C.c_int32()
        rc = self._L.sonde_imet4_create(C.byref(cfg), self.n_ch, fq, self.max_chunk, C.byref(self._h), C.byref(ifr), C.byref(dec))
        self.if_rate, self.dec_m = ifr.value, dec.value
        if rc:
            raise SondeError(rc, "sonde_imet4_create")

    def process_host(self, x: np.ndarray):
        dt = {8: np.uint8, 16: np.int16, 32: np.float32}[self.bits]
        x = np.ascontiguousarray(x, dtype=dt).reshape(self.n_ch, -1)
        n = x.shape[1] // (2 if self.iq else 1)
        self._call("process_host", self._h, x.ctypes.data, n)

    def process_device(self, ptr: int, n: int, ch_stride: int | None = None):
        """n samples per channel at device pointer ptr; channel c's row starts at c * ch_stride samples (complex ones for IQ), c * n when None"""
        if ch_stride is None:
            self._call("process_device", self._h, C.c_void_p(ptr), n)
        else:
            self._call("process_device_strided", self._h, C.c_void_p(ptr), int(ch_stride), n)

    def restart_channel(self, c: int, fq: float = 0.0):
        """from the next call on channel c is a fresh channel at --iq fq (FM audio: fq is ignored), and active"""
        self._call("restart_channel", self._h, int(c), float(fq))

    def release_channel(self, c: int):
        """channel c takes no part in the calls that follow: nothing of it is read or written; its frame in progress is dropped"""
        self._call("release_channel", self._h, int(c))

    def channel_active(self, c: int) -> bool:
        return bool(self._call("channel_active", self._h, int(c)))

    def read_tap(self, channel: int, tap: str, first: int, count: int) -> np.ndarray:
        """testing tap: `count` samples of TAPS[tap] from absolute IF sample `first`, which must still be inside the history ring (the last
        tap_ring - 64 samples; "if": inside the last call).  complex64 for the IQ taps, float32 otherwise"""
        num, width = TAPS[tap]
        out = np.empty(count * width, np.float32)
        self._call("read_tap", self._h, channel, num, first, count, out.ctypes.data)
        return out.view(np.complex64) if width == 2 else out

    def read_state(self, channel: int = 0) -> dict:
        """testing tap: the channel's state record between calls"""
        st = Imet4State()
        self._call("read_state", self._h, channel, C.byref(st))
        return {n: getattr(st, n) for n, _ in Imet4State._fields_}

    @property
    def tap_ring(self) -> int:
        return int(self._L.sonde_imet4_tap_ring(self._h))
