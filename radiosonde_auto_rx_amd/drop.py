"""ctypes mirror of include/sonde_drop.h: the RD94 / RD41 dropsonde engine (GPU, many channels per call), its printer and its soft-bit
framer (host code).

    eng = DropEngine(fqs, 48000, opt_b=True)                # iq_dec --FM --lpFM --wav --bo 16 --iq fq | rd94rd41drop -b
    eng.process_host(x)           # x: (n_channels, n * 2) int16 IQ, n <= max_chunk, a multiple of dec_m
    eng.finish()                  # at the end of the input: with -b a frame whose header is open is handed out with complete = False
    for f in eng.fetch_frames():  # {"channel", "bytes", "nraw", "complete", "sample", "err94", "err41"}
        text = printer.frame(f["bytes"])

    DropEngine.fm(n_channels, 48000, bits=16)               # the slicer alone, on integer FM samples of the caller

DropPrinter(json=True).frame(bytes) returns the characters the reference's rd94rd41drop prints for that frame.

Channels at run time (ChannelizedReceiver): DropEngine(fqs, sr, bits=32) takes float32 IQ at a rate at which iq_dec does not decimate;
release_channel(c) takes a channel out of the launches, restart_channel(c, fq) makes it a fresh channel at a new fq, finish_channel(c) ends its
stream (with -b the frame of an open header is handed out) and releases it, process_device(ptr, n, ch_stride=...) reads rows of a staging
array."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._frame_engine import EngineHandle, PrinterHandle, SoftinHandle
from .engine import SondeError, lib

FRAME_LEN, RAWBITS = 120, 2400
IN_IQ, IN_FM = 0, 1


class DropCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("sample_rate", "input", "bits", "invert", "opt_b")] + [("baud", C.c_float), ("reserved", C.c_int32 * 8)]


class DropInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("if_rate", "dec_m", "taps_dec", "taps_fm")] + [("sps", C.c_float), ("reserved", C.c_int32 * 7)]


class DropFrame(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("channel", "nraw", "complete", "err94", "err41", "reserved")] + \
               [("sample", C.c_uint64), ("bytes", C.c_uint8 * FRAME_LEN)]


class DropOpts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("raw", "vbs", "json", "type", "jsn_freq_khz")] + [("version", C.c_char * 32), ("reserved", C.c_int32 * 4)]


def _sigs(L):
    if getattr(L, "_drop_sigs", False):
        return L
    P, U8 = C.c_void_p, C.POINTER(C.c_uint8)
    L.sonde_drop_create.argtypes = [C.POINTER(DropCfg), C.c_int32, C.POINTER(C.c_double), C.c_int32, C.POINTER(P)]
    L.sonde_drop_destroy.argtypes = [P]
    L.sonde_drop_destroy.restype = None
    L.sonde_drop_info.argtypes = [P, C.POINTER(DropInfo)]
    L.sonde_drop_design.argtypes = [C.POINTER(DropCfg), C.POINTER(DropInfo)]
    L.sonde_drop_process_host.argtypes = [P, P, C.c_int32]
    L.sonde_drop_process_device.argtypes = [P, P, C.c_int32]
    L.sonde_drop_finish.argtypes = [P]
    L.sonde_drop_process_device_strided.argtypes = [P, P, C.c_int64, C.c_int32]
    L.sonde_drop_restart_channel.argtypes = [P, C.c_int32, C.c_double]
    L.sonde_drop_release_channel.argtypes = [P, C.c_int32]
    L.sonde_drop_channel_active.argtypes = [P, C.c_int32]
    L.sonde_drop_finish_channel.argtypes = [P, C.c_int32]
    L.sonde_drop_read_fm.argtypes = [P, C.c_int32, C.c_int64, C.c_int32, P]
    L.sonde_drop_fetch_frames.argtypes = [P, C.POINTER(DropFrame), C.c_int32]
    L.sonde_drop_printer_create.argtypes = [C.POINTER(DropOpts), C.POINTER(P)]
    L.sonde_drop_printer_destroy.argtypes = [P]
    L.sonde_drop_printer_destroy.restype = None
    L.sonde_drop_print_frame.argtypes = [P, U8, C.c_char_p, C.c_size_t]
    L.sonde_drop_printer_last.argtypes = [P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.sonde_drop_chksum16.argtypes = [U8, C.c_int32]
    L.sonde_drop_chksum16.restype = C.c_uint32
    L.sonde_drop_crc16.argtypes = [U8, C.c_int32]
    L.sonde_drop_crc16.restype = C.c_uint32
    L.sonde_drop_errs.argtypes = [U8, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.sonde_drop_rawhex.argtypes = [C.c_char_p, U8]
    L.sonde_drop_softin_create.argtypes = [C.c_int32, C.POINTER(P)]
    L.sonde_drop_softin_destroy.argtypes = [P]
    L.sonde_drop_softin_destroy.restype = None
    L.sonde_drop_softin_push.argtypes = [P, C.POINTER(C.c_float), C.c_int32, C.POINTER(DropFrame), C.c_int32]
    L.sonde_drop_frame_from_rawbits.argtypes = [U8, C.c_int32, C.POINTER(DropFrame)]
    L._drop_sigs = True
    return L


def _u8(data):
    return (C.c_uint8 * max(1, len(data))).from_buffer_copy(bytes(data) or b"\0")


def chksum16(data: bytes) -> int:
    return _sigs(lib()).sonde_drop_chksum16(_u8(data), len(data))


def crc16(data: bytes) -> int:
    return _sigs(lib()).sonde_drop_crc16(_u8(data), len(data))


def errs(frame: bytes) -> tuple[int, int]:
    """(err94, err41): bit i set = block i of that type fails its check"""
    if len(frame) != FRAME_LEN:
        raise ValueError("a frame has %d bytes" % FRAME_LEN)
    e94, e41 = C.c_int32(), C.c_int32()
    _sigs(lib()).sonde_drop_errs(_u8(frame), C.byref(e94), C.byref(e41))
    return e94.value, e41.value


def rawhex(line: bytes, prev: bytes = bytes(FRAME_LEN)) -> tuple[bytes, bool]:
    """one --rawhex line -> (120 bytes, printed?); prev = the bytes of the line before (a pair that is no hex number keeps its byte)"""
    b = _u8(prev)
    ok = _sigs(lib()).sonde_drop_rawhex(bytes(line), b)
    return bytes(b), ok == 1


def frame_from_rawbits(rawbits, nraw: int | None = None) -> dict:
    """print_bitframe's bytes and both check masks from raw bits 0 / 1 (anything else 'x'), bits behind nraw as '0' (host code)"""
    b = np.ascontiguousarray(rawbits, dtype=np.uint8)
    if len(b) != RAWBITS:
        raise ValueError("a frame has %d raw bits" % RAWBITS)
    f = DropFrame()
    rc = _sigs(lib()).sonde_drop_frame_from_rawbits(b.ctypes.data_as(C.POINTER(C.c_uint8)), RAWBITS if nraw is None else int(nraw), C.byref(f))
    if rc:
        raise SondeError(rc, "sonde_drop_frame_from_rawbits")
    return _frame_dict(f)


def _cfg(sr, input, bits, invert, opt_b, baud):
    return DropCfg(sample_rate=sr, input=input, bits=bits, invert=int(invert), opt_b=int(opt_b), baud=float(baud))


def design(sr: int, *, input: int = IN_IQ, bits: int = 16, baud: float = 0.0) -> dict:
    """IF rate, decimation, tap counts and samples per raw bit of that configuration (host code, no GPU); bits=32 where the engine takes
    float32 (IQ at dec_m = 1), a SondeError elsewhere"""
    L = _sigs(lib())
    cfg, inf = _cfg(sr, input, bits, False, False, baud), DropInfo()
    rc = L.sonde_drop_design(C.byref(cfg), C.byref(inf))
    if rc:
        raise SondeError(rc, "sonde_drop_design")
    return {n: getattr(inf, n) for n, _ in DropInfo._fields_ if n != "reserved"}


def _frame_dict(f) -> dict:
    return {"channel": f.channel, "sample": int(f.sample), "nraw": f.nraw, "complete": bool(f.complete), "err94": f.err94, "err41": f.err41,
            "bytes": bytes(f.bytes)}


class DropPrinter(PrinterHandle):
    """frame bytes -> the reference's text / -r / -R / JSON lines (host code, no GPU); keeps the fields that persist between frames."""
    _prefix = "sonde_drop"

    def __init__(self, *, raw: int = 0, vbs: int = 0, json: bool = False, type: int = 0, jsn_freq_khz: int = 0, version: str = ""):
        o = DropOpts(raw=int(raw), vbs=int(vbs), json=int(json), type=int(type), jsn_freq_khz=int(jsn_freq_khz), version=version.encode())
        self._open_printer(_sigs(lib()), o, 1 << 12)

    def frame(self, data) -> str:
        if len(data) != FRAME_LEN:
            raise ValueError("a frame has %d bytes" % FRAME_LEN)
        return self._print("utf-8", _u8(data))

    @property
    def last(self) -> tuple[int, bool]:
        """(type of the last frame: 41 / 94, whether its JSON was printed)"""
        t, j = C.c_int32(), C.c_int32()
        self._L.sonde_drop_printer_last(self._h, C.byref(t), C.byref(j))
        return t.value, bool(j.value)


class DropSoftin(SoftinHandle):
    """the --softin / --softinv bit loop: float32 soft bits -> frames (host code, no GPU); invert = (--softinv) xor (-i)"""
    _prefix, _Frame, _frame_dict = "sonde_drop", DropFrame, staticmethod(_frame_dict)

    def __init__(self, *, invert: bool = False):
        self._open(_sigs(lib()), "softin_create", int(invert), nbuf=16)


class DropEngine(EngineHandle):
    """the iq_dec front end + k_drop_slice behind sonde_drop_create: one channel per entry of fqs, all at sample rate sr."""
    _prefix, _Frame, _frame_dict = "sonde_drop", DropFrame, staticmethod(_frame_dict)

    def __init__(self, fqs, sr: int, *, bits: int = 16, invert: bool = False, opt_b: bool = True, baud: float = 0.0, max_chunk: int | None = None,
                 input: int = IN_IQ, n_channels: int | None = None):
        self.n_ch = len(fqs) if input == IN_IQ else int(n_channels or 1)
        self.bits, self.input = bits, input
        self.max_chunk = int(max_chunk or sr // 4)
        cfg = _cfg(sr, input, bits, invert, opt_b, baud)
        fq = (C.c_double * self.n_ch)(*[float(f) for f in fqs]) if input == IN_IQ else None
        self._open(_sigs(lib()), "create", C.byref(cfg), self.n_ch, fq, self.max_chunk, nbuf=32)
        inf = DropInfo()
        self._L.sonde_drop_info(self._h, C.byref(inf))
        self.info = {n: getattr(inf, n) for n, _ in DropInfo._fields_ if n != "reserved"}
        self.if_rate, self.dec_m = inf.if_rate, inf.dec_m

    @classmethod
    def fm(cls, n_channels: int, sr: int, *, bits: int = 16, **kw):
        """the slicer on FM samples of the caller: 16-bit signed or 8-bit unsigned PCM"""
        return cls((), sr, bits=bits, input=IN_FM, n_channels=n_channels, **kw)

    @staticmethod
    def dec_m_of(sr: int) -> int:
        """the decimation the front end applies to an input rate (calls take whole multiples of it)"""
        return design(sr)["dec_m"]

    def process_host(self, x: np.ndarray):
        per = 2 if self.input == IN_IQ else 1
        x = np.ascontiguousarray(x, dtype={8: np.uint8, 16: np.int16, 32: np.float32}[self.bits]).reshape(self.n_ch, -1)
        self._call("process_host", self._h, x.ctypes.data, x.shape[1] // per)

    finish = EngineHandle._finish

    # ---- channels at run time: engines created with bits=32
    def process_device(self, ptr: int, n: int, ch_stride: int | None = None):
        """n samples per channel at device pointer ptr; channel c's row starts at c * ch_stride complex samples, c * n when None"""
        if ch_stride is None:
            self._call("process_device", self._h, C.c_void_p(ptr), n)
        else:
            self._call("process_device_strided", self._h, C.c_void_p(ptr), int(ch_stride), n)

    def restart_channel(self, c: int, fq: float = 0.0):
        """from the next call on channel c is a fresh channel at --iq fq, and active; its frames' "sample" counts from here"""
        self._call("restart_channel", self._h, int(c), float(fq))

    def release_channel(self, c: int):
        """channel c takes no part in the calls that follow: nothing of it is read or written; its frame in progress is dropped"""
        self._call("release_channel", self._h, int(c))

    def finish_channel(self, c: int):
        """the end of channel c's stream: with -b the frame of an open header is queued with complete = False; then the channel is released"""
        self._call("finish_channel", self._h, int(c))

    def channel_active(self, c: int) -> bool:
        return bool(self._call("channel_active", self._h, int(c)))

    def read_fm(self, channel: int, first: int, count: int) -> np.ndarray:
        """testing tap: `count` samples of the channel's FM stream from its sample `first` (counted from its restart, still inside the ring) as
        `iq_dec --FM --lpFM --wav --bo 16` writes them (int16)"""
        out = np.empty(count, np.int16)
        self._call("read_fm", self._h, int(channel), int(first), int(count), out.ctypes.data)
        return out
