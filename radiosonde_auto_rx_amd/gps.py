"""The RS92 position solve's 4-satellite subset search on the GPU (include/sonde_gps.h): ctypes mirrors of a job and a pick, and GpsSolver.

An RS92 frame carries raw GPS ranges; the default solver takes the closed-form solution of every 4-satellite subset (up to 495 a frame) and keeps the one with the
best GDOP.  GpsSolver runs that search for many frames in one launch (one wavefront per frame) and returns which subset wins; the host decoder then solves that one
subset with the functions it always used, so the printed text does not change.  No CPU fallback: without a device the constructor raises."""
import ctypes as C

import numpy as np

from .engine import SondeError, lib

MAX_SATS = 12
FRAME_LEN = 240
VIA = ("host", "pick", "doubt", "mismatch")                       # SONDE_GPS_VIA_*


class GpsSat(C.Structure):
    """sonde_gps_sat_t (include/sonde_rs92.h)"""
    _fields_ = [("X", C.c_double), ("Y", C.c_double), ("Z", C.c_double), ("x", C.c_double), ("y", C.c_double), ("z", C.c_double), ("p", C.c_double)]


class GpsJob(C.Structure):
    """sonde_gps_job_t"""
    _fields_ = [("sat", GpsSat * MAX_SATS), ("n", C.c_int32), ("reserved", C.c_int32)]


class GpsPick(C.Structure):
    """sonde_gps_pick_t"""
    _fields_ = [("num", C.c_int32), ("best", C.c_int32), ("doubt", C.c_int32), ("n", C.c_int32), ("gdop", C.c_double)]

    def key(self):
        """what two solvers must share: every field, gdop as its 64 bits"""
        return (self.num, self.best, self.doubt, self.n, np.float64(self.gdop).tobytes())


class GpsStats(C.Structure):
    """sonde_gps_stats_t (include/sonde_gps.h)"""
    _fields_ = [("jobs", C.c_int64), ("launches", C.c_int64), ("doubts", C.c_int64), ("mismatches", C.c_int64), ("picked", C.c_int64), ("reserved", C.c_int64 * 3)]

    def as_dict(self):
        return {k: getattr(self, k) for k in ("jobs", "launches", "doubts", "mismatches", "picked")}


assert C.sizeof(GpsJob) == 680 and C.sizeof(GpsPick) == 24

_proto = False


def _lib():
    global _proto
    L = lib()
    if not _proto:
        L.sonde_gps_job_fill.argtypes = [C.POINTER(GpsJob), C.c_int32] + [C.POINTER(C.c_double)] * 4
        L.sonde_gps_host_solve.argtypes = [C.POINTER(GpsJob), C.POINTER(GpsPick)]
        L.sonde_gps_dev_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
        L.sonde_gps_dev_destroy.argtypes = [C.c_void_p]
        L.sonde_gps_dev_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.sonde_gps_dev_stats.argtypes = [C.c_void_p, C.POINTER(GpsStats)]
        L.sonde_gps_rs92_text_batch.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)]
        L.sonde_rs92_dec_begin.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.POINTER(GpsJob)]
        L.sonde_rs92_dec_end.argtypes = [C.c_void_p, C.POINTER(GpsPick), C.c_char_p, C.c_size_t]
        L.sonde_rs92_dec_gps_via.argtypes = [C.c_void_p]
        _proto = True
    return L


def _chk(rc: int, what: str) -> int:
    if rc < 0:
        raise SondeError(f"{what}: {lib().sonde_strerror(rc).decode()} ({rc})")
    return rc


def job_from(X, Y, Z, p) -> GpsJob:
    """a job from satellite positions as sent [m, ECEF] and p = pseudorange + clock correction [m]: the library turns the positions (sonde_gps_job_fill)"""
    n = len(p)
    arr = [(C.c_double * n)(*[float(v) for v in a]) for a in (X, Y, Z, p)]
    j = GpsJob()
    _chk(_lib().sonde_gps_job_fill(C.byref(j), n, *arr), "sonde_gps_job_fill")
    return j


def host_solve(job: GpsJob) -> GpsPick:
    """the selection by the host decoder's own functions (sonde_gps_host_solve): what GpsSolver.solve must give, doubt apart"""
    p = GpsPick()
    _chk(_lib().sonde_gps_host_solve(C.byref(job), C.byref(p)), "sonde_gps_host_solve")
    return p


def text_batch(solver, handles, frames, ec, text_max: int = 2048):
    """sonde_gps_rs92_text_batch: handles = one sonde_rs92_dec_t handle per record (the same one may appear several times: its records are taken in order),
    frames = the 240 corrected bytes of each, ec = rs_decode's value of each; solver = a GpsSolver or None (a plain loop over sonde_rs92_dec_corrected).
    -> the text of each record"""
    n = len(handles)
    if n == 0:
        return []
    hs = (C.c_void_p * n)(*[h.value if isinstance(h, C.c_void_p) else h for h in handles])
    fr = np.frombuffer(b"".join(bytes(f[:FRAME_LEN]) for f in frames), np.uint8)
    if len(fr) != n * FRAME_LEN or len(ec) != n:
        raise ValueError("a record is 240 frame bytes and a value of ec")
    ecs = (C.c_int32 * n)(*[int(v) for v in ec])
    out = C.create_string_buffer(n * text_max)
    ln = (C.c_int32 * n)()
    _chk(_lib().sonde_gps_rs92_text_batch(solver._h if solver is not None else None, hs, fr.ctypes.data, ecs, n, out, text_max, ln), "sonde_gps_rs92_text_batch")
    texts = []
    for i in range(n):
        _chk(ln[i], "sonde_gps_rs92_text_batch: record %d" % i)
        texts.append(out.raw[i * text_max:i * text_max + ln[i]].decode(errors="replace"))
    return texts


class GpsSolver:
    """sonde_gps_dev_t: device and page-locked memory for max_jobs jobs a launch, a stream of its own; solve() is synchronous"""

    def __init__(self, max_jobs: int = 1024):
        h = C.c_void_p()
        _chk(_lib().sonde_gps_dev_create(int(max_jobs), C.byref(h)), "sonde_gps_dev_create")
        self._h, self.max_jobs = h, int(max_jobs)

    def close(self):
        if getattr(self, "_h", None):
            _lib().sonde_gps_dev_destroy(self._h)
            self._h = None

    __del__ = close

    def solve(self, jobs):
        """jobs: a sequence of GpsJob (or a ctypes array of them) -> a list of GpsPick, one per job; more than max_jobs go in chunks"""
        n = len(jobs)
        arr = jobs if isinstance(jobs, C.Array) else (GpsJob * max(n, 1))(*jobs)
        picks = (GpsPick * max(n, 1))()
        _chk(_lib().sonde_gps_dev_solve(self._h, arr, n, picks), "sonde_gps_dev_solve")
        return [picks[i] for i in range(n)]

    def stats(self) -> dict:
        st = GpsStats()
        _chk(_lib().sonde_gps_dev_stats(self._h, C.byref(st)), "sonde_gps_dev_stats")
        return st.as_dict()

    def text_batch(self, handles, frames, ec, text_max: int = 2048):
        return text_batch(self, handles, frames, ec, text_max)
