"""What the ctypes mirrors of the single-sonde engines (imet4.py, mk2a.py, wxr.py, drop.py) share: the handle of an engine, of a printer
and of a soft-bit framer.  A subclass names the C prefix ("sonde_wxr"), its frame Structure and the function that turns one into a dict,
and creates the C object in its __init__."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .engine import SondeError


class _Handle:
    _prefix = ""

    def _call(self, name: str, *args) -> int:
        """<prefix>_<name>(*args); a negative return is an error (every SONDE_E_* code is negative; create, process_* and finish
        return 0 otherwise, the calls that hand out frames or text their count)"""
        rc = getattr(self._L, "%s_%s" % (self._prefix, name))(*args)
        if rc < 0:
            raise SondeError(rc, "%s_%s" % (self._prefix, name))
        return rc

    def _drain(self, name: str, *args) -> list[dict]:
        """the frames <prefix>_<name>(handle, *args, buffer, len) hands out, until it leaves the buffer unfilled"""
        out = []
        while True:
            k = self._call(name, self._h, *args, self._buf, len(self._buf))
            out += [self._frame_dict(f) for f in self._buf[:k]]
            if k < len(self._buf):
                return out

    def _open(self, L, create: str, *args, nbuf: int = 0):
        """<prefix>_<create>(*args, &handle), and a buffer of nbuf frames"""
        self._L, self._h = L, C.c_void_p()
        if nbuf:
            self._buf = (self._Frame * nbuf)()
        self._call(create, *args, C.byref(self._h))

    def close(self):
        if self._h:
            getattr(self._L, "%s_%s" % (self._prefix, self._destroy))(self._h)
            self._h = C.c_void_p()

    __del__ = close


class EngineHandle(_Handle):
    """process_device / fetch_frames / close of an engine; `finish = EngineHandle._finish` where the C ABI has one"""
    _destroy = "destroy"

    def process_device(self, ptr: int, n: int):
        self._call("process_device", self._h, C.c_void_p(ptr), n)

    def _finish(self):
        self._call("finish", self._h)

    def fetch_frames(self) -> list[dict]:
        return self._drain("fetch_frames")


class PrinterHandle(_Handle):
    _destroy = "printer_destroy"

    def _open_printer(self, L, opts, outlen: int):
        self._open(L, "printer_create", C.byref(opts))
        self._out = C.create_string_buffer(outlen)

    def _print(self, encoding: str, *args) -> str:
        """<prefix>_print_frame(handle, *args, out, len) as text"""
        n = self._call("print_frame", self._h, *args, self._out, len(self._out))
        return self._out.raw[:n].decode(encoding)


class SoftinHandle(_Handle):
    _destroy = "softin_destroy"

    def push(self, soft) -> list[dict]:
        x = np.ascontiguousarray(soft, dtype=np.float32)
        out, n, p = [], len(x), x.ctypes.data_as(C.POINTER(C.c_float))
        while True:
            k = self._call("softin_push", self._h, p, n, self._buf, len(self._buf))
            out += [self._frame_dict(f) for f in self._buf[:k]]
            n, p = 0, None
            if k < len(self._buf):
                return out
