"""ctypes mirror of include/sonde_wxr.h: the Weathex WxR-301D engine (GPU, many channels per call), its printer and its soft-bit framer
for one stream (host code).  For many channels behind the GPU modem the soft-bit loop runs on the device: fsk.SoftinDev(n, kind="wxr") / fetch_wxr(), whose
records WxrPrinter.decoded(rec) prints.

    eng = WxrEngine(fqs, 96000, if_bw_khz=64, opt_b=True)          # auto_rx: iq_dec --FM --IFbw 64 --lpFM --iq fq | weathex301d -b
    eng.process_host(x)           # x: (n_channels, n * 2) int16 IQ, n <= max_chunk, a multiple of dec_m
    eng.finish()                  # at the end of the input: a frame whose header is open is handed out with complete = False
    for f in eng.fetch_frames():  # {"channel", "bits", "nbits", "complete", "sample"}
        text = printer.frame(f["bits"])

    WxrEngine.fm(n_channels, 96000, bits=32)                       # the slicer alone, on FM samples of the caller

WxrPrinter(json=True).frame(bits) returns the characters the reference's weathex301d prints for that frame."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._frame_engine import EngineHandle, PrinterHandle, SoftinHandle
from .engine import SondeError, lib

BITS = 552
IN_IQ, IN_FM = 0, 1


class WxrCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("sample_rate", "input", "bits", "pn9", "invert", "opt_b", "if_bw_khz")] + \
               [("baud", C.c_float), ("reserved", C.c_int32 * 8)]


class WxrInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("if_rate", "dec_m", "taps_dec", "taps_fm")] + [("sps", C.c_float), ("reserved", C.c_int32 * 7)]


class WxrFrame(C.Structure):
    _fields_ = [("channel", C.c_int32), ("nbits", C.c_int32), ("complete", C.c_int32), ("reserved", C.c_int32), ("sample", C.c_uint64),
                ("bits", C.c_uint8 * BITS)]


class WxrOpts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("raw", "vbs", "json", "pn9", "jsn_freq_khz")] + [("version", C.c_char * 32), ("ts", C.c_int32), ("reserved", C.c_int32 * 3)]


def _sigs(L):
    if getattr(L, "_wxr_sigs", False):
        return L
    P = C.c_void_p
    L.sonde_wxr_create.argtypes = [C.POINTER(WxrCfg), C.c_int32, C.POINTER(C.c_double), C.c_int32, C.POINTER(P)]
    L.sonde_wxr_destroy.argtypes = [P]
    L.sonde_wxr_destroy.restype = None
    L.sonde_wxr_info.argtypes = [P, C.POINTER(WxrInfo)]
    L.sonde_wxr_design.argtypes = [C.POINTER(WxrCfg), C.POINTER(WxrInfo)]
    L.sonde_wxr_process_host.argtypes = [P, P, C.c_int32]
    L.sonde_wxr_process_device.argtypes = [P, P, C.c_int32]
    L.sonde_wxr_finish.argtypes = [P]
    L.sonde_wxr_fetch_frames.argtypes = [P, C.POINTER(WxrFrame), C.c_int32]
    L.sonde_wxr_printer_create.argtypes = [C.POINTER(WxrOpts), C.POINTER(P)]
    L.sonde_wxr_printer_destroy.argtypes = [P]
    L.sonde_wxr_printer_destroy.restype = None
    L.sonde_wxr_print_frame.argtypes = [P, C.POINTER(C.c_uint8), C.c_char_p, C.c_size_t]
    L.sonde_wxr_print_decoded.argtypes = [P, P, C.c_char_p, C.c_size_t]
    L.sonde_wxr_xor8sum.argtypes = [C.POINTER(C.c_uint8), C.c_int32]
    L.sonde_wxr_softin_create.argtypes = [C.c_int32, C.c_int32, C.POINTER(P)]
    L.sonde_wxr_softin_destroy.argtypes = [P]
    L.sonde_wxr_softin_destroy.restype = None
    L.sonde_wxr_softin_push.argtypes = [P, C.POINTER(C.c_float), C.c_int32, C.POINTER(WxrFrame), C.c_int32]
    L.sonde_wxr_softin_finish.argtypes = [P, C.POINTER(WxrFrame)]
    L._wxr_sigs = True
    return L


def xor8sum(data: bytes) -> int:
    b = (C.c_uint8 * max(1, len(data))).from_buffer_copy(bytes(data) or b"\0")
    return _sigs(lib()).sonde_wxr_xor8sum(b, len(data))


def _cfg(sr, input, bits, pn9, invert, opt_b, if_bw_khz, baud):
    return WxrCfg(sample_rate=sr, input=input, bits=bits, pn9=int(pn9), invert=int(invert), opt_b=int(opt_b), if_bw_khz=int(if_bw_khz), baud=float(baud))


def design(sr: int, *, input: int = IN_IQ, bits: int = 16, pn9: bool = False, if_bw_khz: int = 64, baud: float = 0.0) -> dict:
    """IF rate, decimation, tap counts and samples per bit of that configuration (host code, no GPU)"""
    L = _sigs(lib())
    cfg, inf = _cfg(sr, input, bits, pn9, False, False, if_bw_khz, baud), WxrInfo()
    rc = L.sonde_wxr_design(C.byref(cfg), C.byref(inf))
    if rc:
        raise SondeError(rc, "sonde_wxr_design")
    return {n: getattr(inf, n) for n, _ in WxrInfo._fields_ if n != "reserved"}


def _frame_dict(f) -> dict:
    return {"channel": f.channel, "sample": int(f.sample), "nbits": f.nbits, "complete": bool(f.complete),
            "bits": np.frombuffer(bytes(f.bits), np.uint8).copy()}


class WxrPrinter(PrinterHandle):
    """frame bits, or a record of the device soft-bit consumer -> the reference's text / -r / -R / JSON lines (host code, no GPU); remembers the id-1 frame the
    JSON of an id-2 frame needs."""
    _prefix = "sonde_wxr"

    def __init__(self, *, raw: int = 0, vbs: bool = False, json: bool = False, pn9: bool = False, jsn_freq_khz: int = 0, version: str = "", ts: bool = False):
        """ts = -t of the --softin loop: decoded() puts "<seconds> " of the record's hdr_bit in front (frame() has no time to print)"""
        o = WxrOpts(raw=int(raw), vbs=int(vbs), json=int(json), pn9=int(pn9), jsn_freq_khz=int(jsn_freq_khz), version=version.encode(), ts=int(ts))
        self._open_printer(_sigs(lib()), o, 1 << 12)

    def frame(self, bits) -> str:
        b = np.ascontiguousarray(bits, dtype=np.uint8)
        if len(b) != BITS:
            raise ValueError("a frame has %d bit values" % BITS)
        return self._print("latin-1", b.ctypes.data_as(C.POINTER(C.c_uint8)))


    def decoded(self, rec) -> str:
        """the same text from a record of the device soft-bit consumer (a dict of fsk.SoftinDev.fetch_wxr, or a fsk.WxrSoftinRec): its bytes, check values, verdict,
        frame id, serial and counter are printed as they are, nothing is recomputed"""
        from .fsk import WXR_REC_FIELDS, WxrSoftinRec
        if not isinstance(rec, WxrSoftinRec):
            r = WxrSoftinRec()
            for k in WXR_REC_FIELDS:
                v = rec[k]
                setattr(r, k, type(getattr(r, k))(*bytes(v)) if isinstance(v, (bytes, bytearray)) else int(v))
            rec = r
        n = self._call("print_decoded", self._h, C.byref(rec), self._out, len(self._out))
        return self._out.raw[:n].decode("latin-1")


class WxrSoftin(SoftinHandle):
    """the --softin bit loop for one stream: float32 soft bits -> frames (host code, no GPU; a batch of channels: fsk.SoftinDev(kind="wxr"))"""
    _prefix, _Frame, _frame_dict = "sonde_wxr", WxrFrame, staticmethod(_frame_dict)

    def __init__(self, *, pn9: bool = False, invert: bool = False):
        self._open(_sigs(lib()), "softin_create", int(pn9), int(invert), nbuf=16)

    def finish(self) -> list[dict]:
        return [_frame_dict(f) for f in self._buf[:self._call("softin_finish", self._h, self._buf)]]


class WxrEngine(EngineHandle):
    """the iq_dec front end + k_wxr_slice behind sonde_wxr_create: one channel per entry of fqs, all at sample rate sr."""
    _prefix, _Frame, _frame_dict = "sonde_wxr", WxrFrame, staticmethod(_frame_dict)

    def __init__(self, fqs, sr: int, *, bits: int = 16, pn9: bool = False, invert: bool = False, opt_b: bool = True, if_bw_khz: int = 64,
                 baud: float = 0.0, max_chunk: int | None = None, input: int = IN_IQ, n_channels: int | None = None):
        self.n_ch = len(fqs) if input == IN_IQ else int(n_channels or 1)
        self.bits, self.input = bits, input
        self.max_chunk = int(max_chunk or sr // 4)
        cfg = _cfg(sr, input, bits, pn9, invert, opt_b, if_bw_khz, baud)
        fq = (C.c_double * self.n_ch)(*[float(f) for f in fqs]) if input == IN_IQ else None
        self._open(_sigs(lib()), "create", C.byref(cfg), self.n_ch, fq, self.max_chunk, nbuf=32)
        inf = WxrInfo()
        self._L.sonde_wxr_info(self._h, C.byref(inf))
        self.info = {n: getattr(inf, n) for n, _ in WxrInfo._fields_ if n != "reserved"}
        self.if_rate, self.dec_m = inf.if_rate, inf.dec_m

    @classmethod
    def fm(cls, n_channels: int, sr: int, *, bits: int = 32, **kw):
        """the slicer on FM samples of the caller: float32, or 16-bit signed / 8-bit unsigned PCM"""
        return cls((), sr, bits=bits, input=IN_FM, n_channels=n_channels, **kw)

    @staticmethod
    def dec_m_of(sr: int, if_bw_khz: int = 64) -> int:
        """the decimation the front end applies to an input rate (calls take whole multiples of it)"""
        return design(sr, if_bw_khz=if_bw_khz)["dec_m"]

    def process_host(self, x: np.ndarray):
        if self.input == IN_IQ:
            dt, per = (np.int16 if self.bits == 16 else np.uint8), 2
        else:
            dt, per = {8: np.uint8, 16: np.int16, 32: np.float32}[self.bits], 1
        x = np.ascontiguousarray(x, dtype=dt).reshape(self.n_ch, -1)
        self._call("process_host", self._h, x.ctypes.data, x.shape[1] // per)

    finish = EngineHandle._finish
