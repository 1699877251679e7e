"""ctypes bindings of the single-sonde front-end harnesses (oracle/ref_mk2a_harness.c, oracle/ref_imet4_harness.c): the reference's own
mk2a1680mod.c / imet4iq.c driven over an
in-memory capture, every stream sample, the AFC / IQ-dc schedule, the frames and the tables copied out.

TEST INFRASTRUCTURE, like oracle/bind.py: imported by tests/ only.  The libraries are read from oracle/_ref/ (built by `make -C oracle ref`
where the reference lies; they travel with the tree to a machine without it)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .bind import REFDIR, reflib

MK2A_CONSTS = ("if_sr", "decM", "decFM", "L", "M", "K", "N", "delay", "dectaps", "lut_len", "iq_taps", "fm_taps", "iqfm_taps", "lp", "sps",
               "tone_sps", "maxcnt0", "maxlim", "df_end", "locked_end", "n_iqbuf", "mp_ofs")
MK2A_WIN = ("sample", "mv", "mv_pos", "dc", "dDf", "Df", "nominal", "found", "mv2")
MK2A_FRAME = ("nbits", "mv", "mv_pos", "Df", "inv", "sample")
_INT_CONSTS = {"if_sr", "decM", "decFM", "L", "M", "K", "N", "delay", "dectaps", "lut_len", "iq_taps", "fm_taps", "iqfm_taps", "lp", "maxcnt0",
               "maxlim", "locked_end", "n_iqbuf", "mp_ofs"}


class RefMk2aCfg(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("sr", "bps", "opt_iq", "lp_iq", "lpbw_hz", "lp_fm", "dec_fm", "dc", "opt_min", "invert", "shift")] + \
               [("thres", C.c_float), ("baud", C.c_float), ("fq", C.c_double)]


class RefMk2aOut(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("max_if", "max_out", "max_win", "max_dc", "max_frames", "max_lut", "max_taps", "max_tone",
                                       "n_if", "n_out", "n_win", "n_dc", "n_frames", "n_tone")] + \
               [(n, C.c_void_p) for n in ("ifin", "zlp", "fm", "sraw", "bufs", "fmbuf", "win", "dcev", "bits", "bytes", "fmeta", "lut",
                                          "ws_dec", "ws_iq0", "ws_iq1", "ws_fm", "ws_iqfm", "tone")] + \
               [("consts", C.c_double * 22)]


def have_mk2a(libname: str = "libref_mk2a.so") -> bool:
    return os.path.exists(os.path.join(REFDIR, libname))


def ref_mk2a_run(raw, sr: int, *, bits: int = 16, opt_iq: int = 6, fq: float = 0.0, lp_iq: bool = False, lpbw_hz: int = 0, lp_fm: bool = False, dec_fm: int = 0,
                 dc: bool = False, opt_min: bool = False, invert: bool = False, shift: int = 0, thres: float = 0.7, baud: float = 0.0,
                 libname: str = "libref_mk2a.so") -> dict:
    """mk2a1680mod's sample loop on `raw` (interleaved int16 or uint8 IQ) with the CLI's options -> streams, schedule, frames, tables.
    libname: libref_mk2a.so (the reference's -Ofast) or libref_mk2a_O2.so."""
    raw = np.ascontiguousarray(raw)
    n_base = raw.size // 2
    max_if = n_base + 16
    arr = dict(ifin=np.zeros((max_if, 2), np.float32), zlp=np.zeros((max_if, 2), np.float32), fm=np.zeros(max_if, np.float32), sraw=np.zeros(max_if, np.float32),
               bufs=np.zeros(max_if, np.float32), fmbuf=np.zeros(max_if, np.float32), win=np.zeros((4096, len(MK2A_WIN)), np.float64),
               dcev=np.zeros((256, 4), np.float64), bits=np.zeros((256, 1760), np.uint8), bytes=np.zeros((256, 176), np.uint8),
               fmeta=np.zeros((256, len(MK2A_FRAME)), np.float64), lut=np.zeros((1 << 18, 2), np.float32), tone=np.zeros((256, 5), np.float64))
    for k in ("ws_dec", "ws_iq0", "ws_iq1", "ws_fm", "ws_iqfm"):
        arr[k] = np.zeros(1 << 14, np.float32)
    o = RefMk2aOut(max_if=max_if, max_out=max_if, max_win=4096, max_dc=256, max_frames=256, max_lut=1 << 18, max_taps=1 << 14, max_tone=256)
    for k, v in arr.items():
        setattr(o, k, v.ctypes.data)
    cfg = RefMk2aCfg(sr=sr, bps=bits, opt_iq=opt_iq, lp_iq=int(lp_iq), lpbw_hz=int(lpbw_hz), lp_fm=int(lp_fm), dec_fm=int(dec_fm), dc=int(dc), opt_min=int(opt_min),
                     invert=int(invert), shift=int(shift), thres=float(thres), baud=float(baud), fq=float(fq))
    L = reflib(libname)
    L.ref_mk2a_run.restype = C.c_int
    L.ref_mk2a_run.argtypes = [C.POINTER(RefMk2aCfg), C.c_void_p, C.c_size_t, C.POINTER(RefMk2aOut)]
    rc = L.ref_mk2a_run(C.byref(cfg), raw.ctypes.data, raw.nbytes, C.byref(o))
    if rc:
        raise RuntimeError("ref_mk2a_run failed: %d" % rc)
    consts = {k: (int(v) if k in _INT_CONSTS else float(v)) for k, v in zip(MK2A_CONSTS, o.consts)}
    cx = lambda a: a.astype(np.float32).view(np.complex64).reshape(-1)                      # noqa: E731
    n_if, n_out = o.n_if, o.n_out
    taps = dict(dec=consts["dectaps"], iq0=consts["iq_taps"], iq1=consts["iq_taps"], fm=consts["fm_taps"], iqfm=consts["iqfm_taps"])
    out = dict(n_if=n_if, n_out=n_out, consts=consts, dc=bool(dc),
               ifin=cx(arr["ifin"][:n_if]), zlp=cx(arr["zlp"][:n_if]), fm=arr["fm"][:n_if].copy(), sraw=arr["sraw"][:n_if].copy() if opt_iq == 5 else None,
               bufs=arr["bufs"][:n_out].copy(), fmbuf=arr["fmbuf"][:n_out].copy(),
               win=[dict(zip(MK2A_WIN, row)) for row in arr["win"][:o.n_win].tolist()],
               dcev=arr["dcev"][:o.n_dc].copy(),
               frames=[dict(zip(MK2A_FRAME, m), bits=arr["bits"][i, :int(m[0])].copy(), bytes=arr["bytes"][i].copy()) for i, m in enumerate(arr["fmeta"][:o.n_frames].tolist())],
               lut=cx(arr["lut"][:consts["lut_len"]]), tone=arr["tone"][:o.n_tone].copy(),
               ws={k: arr["ws_" + k][:2 * t].copy() for k, t in taps.items()})
    return out


# ----------------------------------------------------------------------------------------------- iMet-4
IMET4_CONSTS = ("if_sr", "decM", "dectaps", "lut_len", "iq_taps", "fm_taps", "M", "sps", "lp", "maxcnt0", "maxlim", "sr_base", "iq", "df_end", "locked_end", "n")
_IMET4_FLOAT = {"sps", "df_end"}


class RefImet4Cfg(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("sr", "bps", "wav", "lp_iq", "lpbw_hz", "lp_fm", "dc", "opt_min", "imet1")] + [("fq", C.c_double)]


class RefImet4Out(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("max_n", "max_frames", "max_dc", "max_lut", "max_taps", "n", "n_frames", "n_dc")] + \
               [(n, C.c_void_p) for n in ("ifin", "zrot", "zlp", "fm", "x", "df", "dc", "nominal", "pre_pos", "mv_pos", "xsum", "F", "dcev", "bits", "fsample", "bytes",
                                          "lut", "ws_dec", "ws_iq0", "ws_iq1", "ws_fm")] + \
               [("consts", C.c_double * 16)]


def ref_imet4_run(raw, sr: int, *, bits: int = 16, wav: bool = False, fq: float = 0.0, lp_iq: bool = False, lpbw_hz: int = 0, lp_fm: bool = False,
                  dc: bool = False, opt_min: bool = False, imet1: bool = False, libname: str = "libref_imet4.so") -> dict:
    """imet4iq's main() on `raw` (interleaved int16 / uint8 IQ, or with wav=True the bytes of a WAV file of FM audio) with the CLI's options
    -> per-sample streams and schedule, frames, tables.  libname: libref_imet4.so (the reference's -Ofast) or libref_imet4_O2.so."""
    raw = np.ascontiguousarray(np.frombuffer(raw, np.uint8) if isinstance(raw, (bytes, bytearray)) else raw)
    max_n = raw.size + 16
    f32, f64 = np.float32, np.float64
    arr = dict(ifin=np.zeros((max_n, 2), f32), zrot=np.zeros((max_n, 2), f32), zlp=np.zeros((max_n, 2), f32), fm=np.zeros(max_n, f32), x=np.zeros(max_n, f32),
               df=np.zeros(max_n, f64), dc=np.zeros(max_n, f64), nominal=np.zeros(max_n, np.uint8), pre_pos=np.zeros(max_n, np.uint32),
               mv_pos=np.zeros(max_n, np.uint32), xsum=np.zeros(max_n, f32), F=np.zeros((max_n, 4), f64), dcev=np.zeros((256, 4), f64),
               bits=np.zeros((64, 1000), np.uint8), fsample=np.zeros(64, f64), bytes=np.zeros((64, 100), np.uint8), lut=np.zeros((1 << 19, 2), f32))
    for k in ("ws_dec", "ws_iq0", "ws_iq1", "ws_fm"):
        arr[k] = np.zeros(1 << 14, f32)
    o = RefImet4Out(max_n=max_n, max_frames=64, max_dc=256, max_lut=1 << 19, max_taps=1 << 14)
    for k, v in arr.items():
        setattr(o, k, v.ctypes.data)
    cfg = RefImet4Cfg(sr=sr, bps=bits, wav=int(wav), lp_iq=int(lp_iq), lpbw_hz=int(lpbw_hz), lp_fm=int(lp_fm), dc=int(dc), opt_min=int(opt_min),
                      imet1=int(imet1), fq=float(fq))
    L = reflib(libname)
    L.ref_imet4_run.restype = C.c_int
    L.ref_imet4_run.argtypes = [C.POINTER(RefImet4Cfg), C.c_void_p, C.c_size_t, C.POINTER(RefImet4Out)]
    rc = L.ref_imet4_run(C.byref(cfg), raw.ctypes.data, raw.nbytes, C.byref(o))
    if rc:
        raise RuntimeError("ref_imet4_run failed: %d" % rc)
    consts = {k: (float(v) if k in _IMET4_FLOAT else int(v)) for k, v in zip(IMET4_CONSTS, o.consts)}
    cx = lambda a: a.astype(np.float32).view(np.complex64).reshape(-1)                      # noqa: E731
    n = o.n
    iq = bool(consts["iq"])
    out = dict(n=n, consts=consts, dc=bool(dc), iq=iq,
               ifin=cx(arr["ifin"][:n]) if iq else None, zrot=cx(arr["zrot"][:n]) if consts["iq_taps"] else None, zlp=cx(arr["zlp"][:n]) if iq else None,
               fm=arr["fm"][:n].copy() if consts["fm_taps"] else None, x=arr["x"][:n].copy(),
               df=arr["df"][:n].copy(), dc_of=arr["dc"][:n].copy(), nominal=arr["nominal"][:n].copy(), pre_pos=arr["pre_pos"][:n].copy(),
               mv_pos=arr["mv_pos"][:n].copy(), xsum=arr["xsum"][:n].copy(), F=arr["F"][:n].copy(), dcev=arr["dcev"][:o.n_dc].copy(),
               frames=[dict(bits=arr["bits"][i].copy(), bytes=arr["bytes"][i].copy(), sample=int(arr["fsample"][i])) for i in range(o.n_frames)],
               lut=cx(arr["lut"][:consts["lut_len"]]),
               ws=dict(dec=arr["ws_dec"][:2 * consts["dectaps"]].copy(), iq0=arr["ws_iq0"][:2 * consts["iq_taps"]].copy(),
                       iq1=arr["ws_iq1"][:2 * consts["iq_taps"]].copy(), fm=arr["ws_fm"][:2 * consts["fm_taps"]].copy()))
    return out
