"""ctypes binding of the batched 2-FSK modem in libsonde_hip.so (include/sonde_fsk.h).

Python mirror of the reference's `fsk_demod` (utils/fsk_demod.c, the codec2 modem auto_rx pipes IQ into) for many
channels at once.  No CPU fallback: the constructor raises without the in-tree HIP library / a GPU.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .engine import ABI_VERSION, _chk, lib

S16, CS16, CU8, CF32 = 1, 2, 3, 4


class FskCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "device", "n_channels", "Fs", "Rs", "M", "P", "nsym", "format",
                                         "fsk_lower", "fsk_upper", "mask", "tone_spacing", "max_chunk")] + \
               [("burst_mode", C.c_int32), ("raw_eye", C.c_int32), ("reserved", C.c_int32 * 2)]


class FskInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("Ts", "N", "Ndft", "Nmem", "Nbits")] + [("tc", C.c_float), ("reserved", C.c_int32 * 4)]


class FskFrame(C.Structure):
    _fields_ = [("nin", C.c_int32), ("nin_next", C.c_int32), ("f_est", C.c_float * 4), ("norm_rx_timing", C.c_float),
                ("ppm", C.c_float), ("EbNodB", C.c_float), ("snr_est", C.c_float)]


class Lms6Opts(C.Structure):
    """sonde_lms6_opts_t (include/sonde_lms6.h)"""
    _fields_ = [("raw", C.c_int32), ("ecc", C.c_int32), ("vit", C.c_int32), ("json", C.c_int32), ("typ", C.c_int32), ("gpsweek", C.c_int32),
                ("jsn_freq_khz", C.c_int32), ("version", C.c_char * 32), ("reserved", C.c_int32 * 4)]


LMS6_TEXT_MAX = 2048


class Lms6SoftinRec(C.Structure):
    """sonde_lms6_softin_t (include/sonde_fsk.h)"""
    _fields_ = [("channel", C.c_int32), ("type", C.c_int32), ("mv", C.c_float), ("text_len", C.c_int32), ("hdr_bit", C.c_uint64),
                ("blen", C.c_int32), ("err", C.c_int32), ("text", C.c_char * LMS6_TEXT_MAX)]


RS92_TEXT_MAX = 2048


class Rs92SoftinRec(C.Structure):
    """sonde_rs92_softin_t (include/sonde_fsk.h)"""
    _fields_ = [("channel", C.c_int32), ("ec", C.c_int32), ("mv", C.c_float), ("text_len", C.c_int32), ("hdr_bit", C.c_uint64),
                ("frame", C.c_uint8 * 240), ("text", C.c_char * RS92_TEXT_MAX)]


# auto_rx's `rs92mod -vx -v --crc --ecc --vel --json --softin -i` (auto_rx/autorx/decode.py:976-987; --json makes --ecc an --ecc2)
RS92_DEFAULTS = dict(verbose=1, aux=1, ecc=2, gps_vel=4, json=1, inv=1, gpsepoch=-1)

IMET54_TEXT_MAX = 1024


class Imet54SoftinRec(C.Structure):
    """sonde_imet54_softin_t (include/sonde_fsk.h)"""
    _fields_ = [("channel", C.c_int32), ("ecc_frm", C.c_int32), ("ecc_tlm", C.c_int32), ("ecc_std", C.c_int32), ("crc", C.c_int32), ("mv", C.c_float),
                ("hdr_bit", C.c_uint64), ("text_len", C.c_int32), ("frame", C.c_uint8 * 108), ("text", C.c_char * IMET54_TEXT_MAX)]


# auto_rx's `imet54mod --ecc --json --softin -i --ptu` (auto_rx/autorx/decode.py:1215-1250)
IMET54_DEFAULTS = dict(ecc=1, json=1, ptu=1, inv=1)

MEISEI_TEXT_MAX = 1024


class MeiseiSoftinRec(C.Structure):
    """sonde_meisei_softin_t (include/sonde_fsk.h)"""
    _fields_ = [("channel", C.c_int32), ("block_err", C.c_uint8 * 12), ("err_frm", C.c_int32), ("err_blks", C.c_int32), ("mv", C.c_float), ("hdr_bit", C.c_uint64),
                ("text_len", C.c_int32), ("bits", C.c_uint8 * 75), ("text", C.c_char * MEISEI_TEXT_MAX)]


# auto_rx's `meisei100mod --softin --json --ptu --ecc` (auto_rx/autorx/decode.py:1343-1379)
MEISEI_DEFAULTS = dict(ecc=1, json=1, ptu=1)

MRZ_TEXT_MAX = 1024


class MrzSoftinRec(C.Structure):
    """sonde_mrz_softin_t (include/sonde_fsk.h)"""
    _fields_ = [("channel", C.c_int32), ("nbits", C.c_int32), ("inv", C.c_int32), ("crc_ok", C.c_int32), ("crclen", C.c_int32), ("mv", C.c_float),
                ("hdr_bit", C.c_uint64), ("text_len", C.c_int32), ("bits", C.c_uint8 * 52), ("text", C.c_char * MRZ_TEXT_MAX)]


# auto_rx's `mp3h1mod --auto --json --softin --ptu` (auto_rx/autorx/decode.py:1256-1293)
MRZ_DEFAULTS = dict(aut=1, json=1, ptu=1)

MTS01_TEXT_MAX = 4096


class Mts01SoftinRec(C.Structure):
    """sonde_mts01_softin_t (include/sonde_fsk.h)"""
    _fields_ = [("channel", C.c_int32), ("crcval", C.c_int32), ("crcdat", C.c_int32), ("crc_ok", C.c_int32), ("mv", C.c_float), ("text_len", C.c_int32),
                ("hdr_bit", C.c_uint64), ("bytes", C.c_uint8 * 131), ("text", C.c_char * MTS01_TEXT_MAX)]


# `mts01mod --softin --json` (auto_rx starts this decoder on IQ; the pipe is the decoder's own)
MTS01_DEFAULTS = dict(json=1)



class WxrSoftinOpts(C.Structure):
    """sonde_wxr_softin_opts_t (include/sonde_fsk.h)"""
    _fields_ = [("pn9", C.c_int32), ("invert", C.c_int32), ("reserved", C.c_int32 * 6)]


class WxrSoftinRec(C.Structure):
    """sonde_wxr_softin_rec_t (include/sonde_fsk.h): 176 bytes"""
    _fields_ = [("channel", C.c_int32), ("reserved0", C.c_int32), ("hdr_bit", C.c_uint64), ("raw", C.c_uint8 * 69), ("x", C.c_uint8 * 69), ("reserved1", C.c_uint8 * 2),
                ("chkval", C.c_uint32), ("chkdat", C.c_uint32), ("chk_ok", C.c_uint8), ("frid", C.c_uint8), ("reserved2", C.c_uint8 * 2), ("sn", C.c_uint32),
                ("cnt", C.c_uint32)]


WXR_REC_FIELDS = ("channel", "hdr_bit", "raw", "x", "chkval", "chkdat", "chk_ok", "frid", "sn", "cnt")
# auto_rx's `weathex301d --softin -i --json [--pn9]` (auto_rx/autorx/decode.py:1414-1423, :1458-1467)
WXR_DEFAULTS = dict(pn9=0, inv=1)

# the kinds whose consumer is made from the options struct of their host decoder: struct (family.py), auto_rx's defaults, create call
_OPTS_KINDS = {"rs92": ("Rs92Opts", RS92_DEFAULTS, "sonde_softin_dev_create_rs92"), "imet54": ("Imet54Opts", IMET54_DEFAULTS, "sonde_softin_dev_create_imet54"),
               "meisei": ("MeiseiOpts", MEISEI_DEFAULTS, "sonde_softin_dev_create_meisei"), "mrz": ("MrzOpts", MRZ_DEFAULTS, "sonde_softin_dev_create_mrz"),
               "mts01": ("Mts01Opts", MTS01_DEFAULTS, "sonde_softin_dev_create_mts01")}

_proto = False


def _lib():
    global _proto
    L = lib()
    if not _proto:
        L.sonde_fsk_create.argtypes = [C.POINTER(FskCfg), C.POINTER(C.c_void_p)]
        L.sonde_fsk_destroy.argtypes = [C.c_void_p]
        L.sonde_fsk_info.argtypes = [C.c_void_p, C.POINTER(FskInfo)]
        L.sonde_fsk_process_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
        L.sonde_fsk_process_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
        L.sonde_fsk_submit_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
        L.sonde_fsk_wait.argtypes = [C.c_void_p]
        L.sonde_fsk_fetch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(FskFrame), C.c_int32, C.POINTER(C.c_int32)]
        L.sonde_fsk_stats.argtypes = [C.c_void_p, C.c_int32, C.POINTER(FskFrame), C.c_void_p, C.POINTER(C.c_int64)]
        L.sonde_fsk_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        L.sonde_fsk_eye.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.sonde_fsk_process_host_var.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]
        L.sonde_fsk_reset_channel.argtypes = [C.c_void_p, C.c_int32]
        L.sonde_fsk_fetch_bits.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.sonde_softin_dev_create.argtypes = [C.c_int32] * 6 + [C.POINTER(C.c_void_p)]
        L.sonde_softin_dev_destroy.argtypes = [C.c_void_p]
        L.sonde_softin_dev_push_fsk.argtypes = [C.c_void_p, C.c_void_p]
        L.sonde_softin_dev_submit_fsk.argtypes = [C.c_void_p, C.c_void_p]
        L.sonde_softin_dev_submit_fsk_behind.argtypes = [C.c_void_p, C.c_void_p]
        L.sonde_softin_dev_collect.argtypes = [C.c_void_p]
        L.sonde_softin_dev_push_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
        L.sonde_softin_dev_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.sonde_softin_dev_counts.argtypes = [C.c_void_p] + [C.POINTER(C.c_int64)] * 5
        L.sonde_softin_dev_fetch_dfm.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.sonde_softin_dev_fetch_m10.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.sonde_softin_dev_fetch_m20.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.sonde_softin_dev_set_m20_skip.argtypes = [C.c_void_p, C.c_int32]
        L.sonde_softin_dev_fetch_drop.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.sonde_softin_dev_create_lms6.argtypes = [C.c_int32, C.POINTER(Lms6Opts), C.c_int32, C.POINTER(C.c_void_p)]
        L.sonde_softin_dev_fetch_lms6.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        from .family import Rs92Opts
        L.sonde_softin_dev_create_rs92.argtypes = [C.c_int32, C.POINTER(Rs92Opts), C.c_int32, C.POINTER(C.c_void_p)]
        L.sonde_softin_dev_rs92_load_ephemeris.argtypes = [C.c_void_p, C.c_char_p]
        L.sonde_softin_dev_rs92_load_almanac.argtypes = [C.c_void_p, C.c_char_p]
        L.sonde_softin_dev_fetch_rs92.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        from .gps import GpsStats
        L.sonde_softin_dev_set_rs92_gps.argtypes = [C.c_void_p, C.c_int32]
        L.sonde_softin_dev_rs92_gps_stats.argtypes = [C.c_void_p, C.POINTER(GpsStats)]
        from .family import Imet54Opts
        L.sonde_softin_dev_create_imet54.argtypes = [C.c_int32, C.POINTER(Imet54Opts), C.c_int32, C.POINTER(C.c_void_p)]
        L.sonde_softin_dev_fetch_imet54.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        from .family import MeiseiOpts
        L.sonde_softin_dev_create_meisei.argtypes = [C.c_int32, C.POINTER(MeiseiOpts), C.c_int32, C.POINTER(C.c_void_p)]
        L.sonde_softin_dev_fetch_meisei.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        from .family import MrzOpts, Mts01Opts
        L.sonde_softin_dev_create_mrz.argtypes = [C.c_int32, C.POINTER(MrzOpts), C.c_int32, C.POINTER(C.c_void_p)]
        L.sonde_softin_dev_fetch_mrz.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.sonde_softin_dev_create_mts01.argtypes = [C.c_int32, C.POINTER(Mts01Opts), C.c_int32, C.POINTER(C.c_void_p)]
        L.sonde_softin_dev_fetch_mts01.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.sonde_softin_dev_create_wxr.argtypes = [C.c_int32, C.POINTER(WxrSoftinOpts), C.c_int32, C.POINTER(C.c_void_p)]
        L.sonde_softin_dev_fetch_wxr.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        _proto = True
    return L


class FskModem:
    """Batched `fsk_demod [--cs16|--cu8] -s [-b lo] [-u hi] [--mask S] [--nsym N] [-p P] (2|4) Fs Rs - -` for n channels."""

    def __init__(self, Fs: int, Rs: int, *, n_channels: int = 1, P: int = 8, nsym: int = 50, fmt: int = CS16,
                 lower: int | None = None, upper: int | None = None, mask: int = 0, max_chunk: int | None = None, device: int = 0, M: int = 2):
        self.n_channels, self.Fs, self.Rs, self.nsym, self.fmt, self.M = n_channels, Fs, Rs, nsym, fmt, M
        if lower is None:
            lower = -Fs // 2 if fmt != S16 else 0
        if upper is None:
            upper = Fs // 2
        cfg = FskCfg(ABI_VERSION, device, n_channels, Fs, Rs, M, P, nsym, fmt, lower, upper, int(mask > 0), mask if mask else 100,
                     max_chunk or Fs)
        h = C.c_void_p()
        _chk(_lib().sonde_fsk_create(C.byref(cfg), C.byref(h)))
        self._h = h
        info = FskInfo()
        _chk(_lib().sonde_fsk_info(h, C.byref(info)))
        self.info = {n: getattr(info, n) for n, _ in FskInfo._fields_ if n != "reserved"}

    def close(self):
        if getattr(self, "_h", None):
            _lib().sonde_fsk_destroy(self._h)
            self._h = None

    __del__ = close

    def process_host(self, x: np.ndarray):
        """x: [n_channels, n*k] int16 (k = 2 for cs16) or uint8 pairs (cu8)."""
        x = np.ascontiguousarray(x)
        if x.ndim == 1:
            x = x[None, :]
        per = 1 if self.fmt == S16 else 2
        n = x.shape[1] // per
        _chk(_lib().sonde_fsk_process_host(self._h, x.ctypes.data_as(C.c_void_p), n, n))

    def process_host_var(self, chunks):
        """Channels fed independently (what the broker does): chunks[c] = samples of channel c for this call (None / empty = nothing)."""
        per = 1 if self.fmt == S16 else 2
        ptrs = (C.c_void_p * self.n_channels)()
        ns = (C.c_int32 * self.n_channels)()
        keep = []
        for c in range(self.n_channels):
            x = chunks[c] if c < len(chunks) else None
            if x is None or len(x) == 0:
                ptrs[c] = None; ns[c] = 0
                continue
            x = np.ascontiguousarray(x); keep.append(x)
            ptrs[c] = x.ctypes.data; ns[c] = x.shape[-1] // per
        _chk(_lib().sonde_fsk_process_host_var(self._h, ptrs, ns))

    def reset_channel(self, ch: int):
        """Back to the fsk_create_hbr() state for one channel (a new stream starts on it)."""
        _chk(_lib().sonde_fsk_reset_channel(self._h, ch))

    def process_device(self, ptr: int, ch_stride: int, n: int):
        _chk(_lib().sonde_fsk_process_device(self._h, C.c_void_p(ptr), ch_stride, n))

    def submit_device(self, ptr: int, ch_stride: int, n: int):
        """process_device in two halves: everything enqueued on the engine's stream, no waiting; wait() (or any other call) blocks until it is through"""
        _chk(_lib().sonde_fsk_submit_device(self._h, C.c_void_p(ptr), ch_stride, n))

    def wait(self):
        _chk(_lib().sonde_fsk_wait(self._h))

    def fetch(self, ch: int = 0):
        """-> (soft decisions [frames, Nbits], list of per-frame dicts) of the last process call."""
        cap = 4096
        fr = (FskFrame * cap)()
        nf = C.c_int32(0)
        nbits = self.info["Nbits"]
        sd = np.zeros(cap * nbits, np.float32)
        nb = _chk(_lib().sonde_fsk_fetch(self._h, ch, sd.ctypes.data_as(C.c_void_p), len(sd), fr, cap, C.byref(nf)))
        recs = [dict(nin=fr[i].nin, nin_next=fr[i].nin_next, f_est=tuple(fr[i].f_est[m] for m in range(self.M)), norm_rx_timing=fr[i].norm_rx_timing,
                     ppm=fr[i].ppm, EbNodB=fr[i].EbNodB, snr_est=fr[i].snr_est) for i in range(nf.value)]
        return sd[:nb].reshape(-1, nbits), recs

    def stats(self, ch: int = 0):
        last = FskFrame()
        Sf = np.zeros(self.info["Ndft"], np.float32)
        n = C.c_int64(0)
        _chk(_lib().sonde_fsk_stats(self._h, ch, C.byref(last), Sf.ctypes.data_as(C.c_void_p), C.byref(n)))
        return dict(f_est=tuple(last.f_est[m] for m in range(self.M)), ppm=last.ppm, EbNodB=last.EbNodB, snr_est=last.snr_est,
                    norm_rx_timing=last.norm_rx_timing, nin=last.nin_next, Sf=Sf, samples=n.value)

    def eye(self, ch: int = 0) -> np.ndarray:
        """Eye diagram of the last modem frame: [8 traces, 2P/ceil(2P/160) samples], normalised (MODEM_STATS.rx_eye)."""
        buf = np.zeros(8 * 160, np.float32)
        ntr, nes = C.c_int32(0), C.c_int32(0)
        n = _chk(_lib().sonde_fsk_eye(self._h, ch, buf.ctypes.data_as(C.c_void_p), C.byref(ntr), C.byref(nes)))
        return buf[:n].reshape(ntr.value, nes.value)

    def kernel_ms(self):
        ms, n = C.c_double(0), C.c_int64(0)
        _chk(_lib().sonde_fsk_kernel_ms(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value


class SoftinDev:
    """Batched `rs41mod --softin [-i] [--ecc|--ecc2]` on the device (include/sonde_fsk.h sonde_softin_dev_*): the consumer of a modem
    engine's soft decisions where they lie — auto_rx's pipe `fsk_demod ... | rs41mod --softin -i` (auto_rx/autorx/decode.py:901-909)
    without the soft-decision stream crossing to the host.  No CPU fallback."""

    def __init__(self, n_channels: int, *, ecc: int = 2, softinv: bool = False, inv: bool = True, auto: bool = False, kind: str = "rs41",
                 vit: int = 2, typ: int = 0, json: bool = False, raw: bool = False, gpsweek: int = 0, freq_khz: int = 0, version: str = "", skip: bool = True,
                 rs92_opts: dict | None = None, ephemeris: str | None = None, almanac: str | None = None, imet54_opts: dict | None = None,
                 meisei_opts: dict | None = None, mrz_opts: dict | None = None, mts01_opts: dict | None = None, gps_device: bool = False, lms6_rs: bool = False,
                 wxr_opts: dict | None = None):
        """kind: "rs41" (rs41mod --softin), "dfm" (dfm09mod --softin: ecc 0 / 1 = --ecc / 2 = --ecc2), "m10" (m10mod --softin), "m20" (m20mod --softin: skip = the rest of
        the second behind a frame is dropped, as m20mod does below -vvv; auto_rx runs `m20mod --json --ptu -vvv --softin -i`: skip=False; ecc, inv and auto mean nothing to it), "drop" (rd94rd41drop --softin /
        --softinv [-i]: auto_rx runs it as softinv=True, inv=False; ecc and auto are ignored) or "lms6" (lms6Xmod --softin: vit 1 = --vit / 2 = --vit2, typ 0 = auto
        detection / 6 = --lms6 / 10 = --lmsX, ecc != 0 = --ecc, json, raw = -r, gpsweek, freq_khz and version as sonde_lms6_opts_t; inv (-i) means nothing to it) or
        "rs92" (rs92mod --softin: rs92_opts = fields of family.Rs92Opts over auto_rx's defaults verbose 1, aux 1, ecc 2, gps_vel 4, json 1, inv 1 — inv there is -i;
        ephemeris = a RINEX navigation file (-e), almanac = an SEM almanac (-a) for every channel's decoder; gps_device = the 4-satellite subset search of the
        position solve runs on the device, one launch per fetch (gps.py; off by default, the texts are the same); ecc, inv and auto of this call mean nothing to it) or
        "imet54" (imet54mod --softin: imet54_opts = fields of family.Imet54Opts over auto_rx's defaults ecc 1, json 1, ptu 1, inv 1 — inv there is -i, aut is --auto, json
        implies ecc; ecc, inv and auto of this call mean nothing to it) or "meisei" (meisei100mod --softin: meisei_opts = fields of family.MeiseiOpts over auto_rx's
        defaults ecc 1, json 1, ptu 1 — json implies ecc; there is no -i: biphase-S compares neighbours, and a header counts in either polarity; ecc, inv and auto of
        this call mean nothing to it) or "mrz" (mp3h1mod --softin: mrz_opts = fields of family.MrzOpts over auto_rx's defaults aut 1, json 1, ptu 1 — inv there is
        -i, aut is --auto, bits_ofs with bits_ofs_given is --ofs; the frame length follows the device's CRC verdict) or "mts01" (mts01mod --softin: mts01_opts =
        fields of family.Mts01Opts over the default json 1; a header counts in either polarity and the bits are read raw, so an inverted stream needs softinv);
        ecc, inv and auto of this call mean nothing to either; or "wxr" (weathex301d --softin: wxr_opts = pn9 (--pn9: 5000 Bd, header AA AA AA C1 94) and inv (-i) over
        auto_rx's defaults pn9 0, inv 1; softinv XORs with inv, as for the dropsondes; bytes, PN9 and the check are the device's, WxrPrinter.decoded prints a record;
        ecc, inv and auto of this call mean nothing to it)"""
        from .engine import SONDE_RS41, SONDE_DFM09, SONDE_M10, SONDE_M20, SONDE_RD94RD41
        h = C.c_void_p()
        self.kind, self.ecc = kind, ecc
        if gps_device and kind != "rs92":
            raise ValueError("gps_device is an RS92 consumer's switch")
        if kind in _OPTS_KINDS:
            from . import family
            opts_name, defaults, create = _OPTS_KINDS[kind]
            kw = dict(defaults)
            kw.update({"rs92": rs92_opts, "imet54": imet54_opts, "meisei": meisei_opts, "mrz": mrz_opts, "mts01": mts01_opts}[kind] or {})
            if isinstance(kw.get("version"), str):
                kw["version"] = kw["version"].encode()
            o = getattr(family, opts_name)(**kw)
            _chk(getattr(_lib(), create)(n_channels, C.byref(o), int(softinv), C.byref(h)))
            self._h, self.n_channels = h, n_channels
            if kind == "rs92" and ephemeris:
                self.load_rs92_ephemeris(ephemeris)
            if kind == "rs92" and almanac:
                self.load_rs92_almanac(almanac)
            if gps_device:
                self.set_rs92_gps(True)
            return
        if kind == "wxr":
            kw = dict(WXR_DEFAULTS)
            kw.update(wxr_opts or {})
            o = WxrSoftinOpts(pn9=int(bool(kw.pop("pn9"))), invert=int(bool(kw.pop("inv"))))
            if kw:
                raise ValueError("wxr_opts has pn9 and inv, not %s" % sorted(kw))
            _chk(_lib().sonde_softin_dev_create_wxr(n_channels, C.byref(o), int(softinv), C.byref(h)))
            self._h, self.n_channels = h, n_channels
            return
        if kind == "lms6":
            o = Lms6Opts(raw=int(raw), ecc=1 if ecc else 0, vit=vit, json=int(json), typ=typ, gpsweek=gpsweek, jsn_freq_khz=freq_khz, version=version.encode())
            _chk(_lib().sonde_softin_dev_create_lms6(n_channels, C.byref(o), int(softinv), C.byref(h)))
            self._h, self.n_channels = h, n_channels
            if lms6_rs:
                self.set_lms6_rs(True)
            return
        _chk(_lib().sonde_softin_dev_create(n_channels, {"rs41": SONDE_RS41, "dfm": SONDE_DFM09, "m10": SONDE_M10, "m20": SONDE_M20, "drop": SONDE_RD94RD41}[kind], ecc, int(softinv), int(inv), int(auto), C.byref(h)))
        self._h, self.n_channels = h, n_channels
        if kind == "m20":
            self.set_m20_skip(skip)

    def set_m20_skip(self, skip: bool):
        """M20 consumers: True = the rest of the second behind a frame is dropped (m20mod below -vvv), False = -vvv; from the next push on"""
        _chk(_lib().sonde_softin_dev_set_m20_skip(self._h, int(bool(skip))))

    def close(self):
        if getattr(self, "_h", None):
            _lib().sonde_softin_dev_destroy(self._h)
            self._h = None

    __del__ = close

    def push_fsk(self, modem: "FskModem"):
        """consume what the modem's last process call left in device memory"""
        _chk(_lib().sonde_softin_dev_push_fsk(self._h, modem._h))

    def submit_fsk(self, modem: "FskModem"):
        """push_fsk without waiting for the result: waits for the modem's launch, then enqueues the consumer on its own stream; the modem can be given its next second
        (submit_device) before collect() — it keeps the soft decisions of two launches"""
        _chk(_lib().sonde_softin_dev_submit_fsk(self._h, modem._h))

    def submit_fsk_behind(self, modem: "FskModem"):
        """the consumer over the modem's launch BEFORE the one in flight (order: wait, submit_device, collect, submit_fsk_behind): nothing waits"""
        _chk(_lib().sonde_softin_dev_submit_fsk_behind(self._h, modem._h))

    def collect(self):
        _chk(_lib().sonde_softin_dev_collect(self._h))

    def push_device(self, ptr: int, ch_stride: int, n_bits: int):
        _chk(_lib().sonde_softin_dev_push_device(self._h, C.c_void_p(ptr), ch_stride, n_bits))

    def fetch(self, max_frames: int = 4096):
        """-> list of dicts (channel, len, ecc, mv, mv_pos, frame bytes, line = the `rs41mod -r` text) of the frames completed since the last fetch"""
        from .engine import SondeFrame, lib
        buf = (SondeFrame * max_frames)()
        n = _chk(_lib().sonde_softin_dev_fetch(self._h, buf, max_frames))
        out = []
        line = C.create_string_buffer(1200)
        for i in range(n):
            f = buf[i]
            ll = lib().sonde_rs41_rawline(C.byref(f), line, 1200)
            out.append(dict(channel=f.channel, len=f.len, ecc=f.ecc, mv=f.mv, mv_pos=f.mv_pos, nbytes=f.nbytes, frame=bytes(f.frame), line=line.raw[:ll].decode()))
        return out

    def fetch_dfm(self, max_frames: int = 8192):
        """DFM consumers: dicts with ecc (per block), conf / dat1 / dat2 nibbles, frame_in_hit, frm_count, inv, line = the `dfm09mod -r [--ecc]` text"""
        from .engine import SondeDfmFrame, lib
        buf = (SondeDfmFrame * max_frames)()
        n = _chk(_lib().sonde_softin_dev_fetch_dfm(self._h, buf, max_frames))
        out = []
        line = C.create_string_buffer(160)
        for i in range(n):
            f = buf[i]
            ll = lib().sonde_dfm_rawline(C.byref(f), self.ecc, line, 128)
            out.append(dict(channel=f.channel, frame_in_hit=f.frame_in_hit, ecc=tuple(f.ecc), mv=f.mv, mv_pos=f.mv_pos, frm_count=f.frm_count, inv=f.inv,
                            conf=bytes(f.conf), dat1=bytes(f.dat1), dat2=bytes(f.dat2), rawbits=bytes(f.rawbits), line=line.raw[:ll].decode()))
        return out

    def fetch_m10(self, max_frames: int = 4096, verbose: int = 1):
        """M10 consumers: dicts with len, cs_ok, cs_calc, frame bytes, line = the `m10mod -r [-v]` text"""
        from .engine import SondeM10Frame, lib
        buf = (SondeM10Frame * max_frames)()
        n = _chk(_lib().sonde_softin_dev_fetch_m10(self._h, buf, max_frames))
        out = []
        line = C.create_string_buffer(420)
        for i in range(n):
            f = buf[i]
            ll = lib().sonde_m10_rawline(C.byref(f), verbose, line, 420)
            out.append(dict(channel=f.channel, nbits=f.nbits, len=f.len, cs_ok=f.cs_ok, cs_calc=f.cs_calc, mv=f.mv, mv_pos=f.mv_pos, frame=bytes(f.frame), line=line.raw[:ll].decode()))
        return out

    def fetch_m20(self, max_frames: int = 4096, verbose: int = 1):
        """M20 consumers: dicts with the fields of SondeM20Frame (channel, nbits, len, cs_ok, cs_calc, blk_ok, fw, mv_pos, mv, frame — what telemetry.M20Telemetry.decode
        takes) and line = the `m20mod -r [-v]` text"""
        from .engine import SondeM20Frame, lib
        buf = (SondeM20Frame * max_frames)()
        n = _chk(_lib().sonde_softin_dev_fetch_m20(self._h, buf, max_frames))
        out = []
        line = C.create_string_buffer(420)
        for i in range(n):
            f = buf[i]
            ll = lib().sonde_m20_rawline(C.byref(f), verbose, line, 420)
            out.append(dict(channel=f.channel, nbits=f.nbits, len=f.len, cs_ok=f.cs_ok, cs_calc=f.cs_calc, blk_ok=f.blk_ok, fw=f.fw, mv_pos=f.mv_pos, mv=f.mv,
                            frame=bytes(f.frame), line=line.raw[:ll].decode()))
        return out

    def fetch_drop(self, max_frames: int = 4096):
        """dropsonde consumers: the frame records of drop.py (channel, sample = soft bits read at the header, bytes, err94, err41, nraw, complete)"""
        from .drop import DropFrame, _frame_dict
        buf = (DropFrame * max_frames)()
        n = _chk(_lib().sonde_softin_dev_fetch_drop(self._h, buf, max_frames))
        return [_frame_dict(buf[i]) for i in range(n)]

    def set_lms6_rs(self, on: bool):
        """LMS6 consumers (lms6_rs=True at creation): RS(255,223) of the blocks on the device as well (k_lms6_rs); the channels' decoders take its results instead
        of decoding.  Off by default; the text is the same either way."""
        f = _lib().sonde_softin_dev_set_lms6_rs
        f.argtypes = [C.c_void_p, C.c_int32]
        _chk(f(self._h, int(bool(on))))

    def lms6_rs_stats(self):
        """LMS6 consumers: (RS results the decoders took from device records, decoded on the host instead), over all channels"""
        u, m = C.c_int64(0), C.c_int64(0)
        f = _lib().sonde_softin_dev_lms6_rs_stats
        f.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        _chk(f(self._h, C.byref(u), C.byref(m)))
        return u.value, m.value

    def fetch_lms6(self, max_blocks: int = 1024):
        """LMS6 consumers: a dict per completed block — channel, hdr_bit (the header's bit index in the channel's stream), mv, type (6 / 0x0206 / 10 in effect
        after the block), blen, err, text = what `lms6Xmod` prints for the block, lines = its non-empty lines"""
        buf = (Lms6SoftinRec * max_blocks)()
        n = _chk(_lib().sonde_softin_dev_fetch_lms6(self._h, buf, max_blocks))
        out = []
        for i in range(n):
            r = buf[i]
            text = r.text.decode()
            out.append(dict(channel=r.channel, hdr_bit=r.hdr_bit, mv=r.mv, type=r.type, blen=r.blen, err=r.err, text=text, lines=[l for l in text.splitlines() if l]))
        return out

    def load_rs92_ephemeris(self, path: str):
        """RS92 consumers: a RINEX navigation file (rs92mod -e) for every channel's decoder"""
        _chk(_lib().sonde_softin_dev_rs92_load_ephemeris(self._h, os.fsencode(path)))

    def load_rs92_almanac(self, path: str):
        """RS92 consumers: an SEM almanac (rs92mod -a) for every channel's decoder"""
        _chk(_lib().sonde_softin_dev_rs92_load_almanac(self._h, os.fsencode(path)))

    def set_rs92_gps(self, on: bool):
        """RS92 consumers: True = fetch_rs92 sends the 4-satellite subset search of every fetched frame to the device in one launch (gps.py) and
        solves only the winning subset on the host; the texts do not change.  From the next fetch on"""
        _chk(_lib().sonde_softin_dev_set_rs92_gps(self._h, int(bool(on))))

    def rs92_gps_stats(self):
        """RS92 consumers: jobs / launches / doubts / mismatches / picked of the device subset search so far (all 0 while the switch is off)"""
        from .gps import GpsStats
        st = GpsStats()
        _chk(_lib().sonde_softin_dev_rs92_gps_stats(self._h, C.byref(st)))
        return st.as_dict()

    def _fetch_text(self, call: str, rec, max_frames: int, fields, encoding: str = "utf-8"):
        """the records whose text is made at fetch time: the named fields (byte arrays as bytes) and text"""
        buf = (rec * max_frames)()
        n = _chk(getattr(_lib(), call)(self._h, buf, max_frames))
        out = []
        for r in buf[:n]:
            d = {k: getattr(r, k) for k in fields}
            d.update({k: bytes(v) for k, v in d.items() if isinstance(v, C.Array)})
            d["text"] = r.text[:max(r.text_len, 0)].decode(encoding)
            out.append(d)
        return out

    def fetch_rs92(self, max_frames: int = 1024):
        """RS92 consumers: a dict per completed frame — channel, ec (rs_decode's value: 0, repaired bytes, negative = left as received), mv, hdr_bit (symbols read when
        the header matched), frame = the 240 bytes behind rs92_ecc, text = what `rs92mod` prints for it (the channel's own decoder: calibration rows, orbit data)"""
        return self._fetch_text("sonde_softin_dev_fetch_rs92", Rs92SoftinRec, max_frames, ("channel", "ec", "mv", "hdr_bit", "frame"))

    def fetch_imet54(self, max_frames: int = 1024):
        """iMet-54 consumers: a dict per completed frame — channel, ecc_frm / ecc_tlm / ecc_std (print_frame's sums: repaired codewords, -1 behind an uncorrectable
        one), crc (0 neither check sum, 1 the standard frame's, 2 the continuous frame's), mv, hdr_bit (symbols read when the header matched), frame = the 108 bytes
        behind Hamming(8,4), text = what `imet54mod` prints for it from the device's verdicts"""
        return self._fetch_text("sonde_softin_dev_fetch_imet54", Imet54SoftinRec, max_frames, ("channel", "ecc_frm", "ecc_tlm", "ecc_std", "crc", "mv", "hdr_bit", "frame"))

    def fetch_meisei(self, max_frames: int = 1024):
        """Meisei consumers: a dict per completed frame — channel, block_err (12 verdicts, subframe 0 first: 0 / 1 / 2 corrected bits, 0xF padding or word parity,
        0xE uncorrectable), err_frm / err_blks (blocks 0xE / 0xF, blocks not 0), mv (with its sign), hdr_bit (half symbols read when the header matched), bits =
        the 600 frame bits behind BCH in 75 bytes, MSB first, text = what `meisei100mod` prints for it from the device's bits and verdicts"""
        return self._fetch_text("sonde_softin_dev_fetch_meisei", MeiseiSoftinRec, max_frames, ("channel", "block_err", "err_frm", "err_blks", "mv", "hdr_bit", "bits"))

    def fetch_mrz(self, max_frames: int = 1024):
        """MRZ consumers: a dict per completed frame — channel, nbits (408 ECEF / 384 lat / lon: the length in effect for the frame), inv (polarity in effect),
        crc_ok / crclen (the device's verdict and the 42 / 45 bytes it covers; 0 with -R), mv (with its sign), hdr_bit (half symbols read when the header matched),
        bits = the frame bits from the header's first in 52 bytes, MSB first, text = what `mp3h1mod` prints for it from the device's bits and verdict"""
        return self._fetch_text("sonde_softin_dev_fetch_mrz", MrzSoftinRec, max_frames, ("channel", "nbits", "inv", "crc_ok", "crclen", "mv", "hdr_bit", "bits"))

    def fetch_mts01(self, max_frames: int = 256):
        """MTS01 consumers: a dict per completed frame — channel, crcval / crcdat / crc_ok (the device's CRC-16, the stored one, the verdict), mv (with its sign),
        hdr_bit (symbols read when the header matched), bytes = the 131 frame bytes, text = what `mts01mod` prints for it from the device's bytes and verdict (the
        frame's own characters are part of it, whatever a damaged frame holds: a character per byte, latin-1)"""
        return self._fetch_text("sonde_softin_dev_fetch_mts01", Mts01SoftinRec, max_frames, ("channel", "crcval", "crcdat", "crc_ok", "mv", "hdr_bit", "bytes"),
                                encoding="latin-1")

    def fetch_wxr(self, max_frames: int = 4096):
        """WxR-301D consumers: a dict per completed frame — channel, hdr_bit (soft bits read before the one that completed the header), raw / x = the 69 frame bytes
        before / behind PN9, chkval / chkdat / chk_ok (the device's xor8 << 8 | sum8, the stored one, the verdict), frid, sn, cnt: what wxr.WxrPrinter.decoded takes"""
        buf = (WxrSoftinRec * max_frames)()
        n = _chk(_lib().sonde_softin_dev_fetch_wxr(self._h, buf, max_frames))
        out = []
        for r in buf[:n]:
            d = {k: getattr(r, k) for k in WXR_REC_FIELDS}
            d.update({k: bytes(v) for k, v in d.items() if isinstance(v, C.Array)})
            out.append(d)
        return out

    def counts(self):
        v = [C.c_int64(0) for _ in range(5)]
        _chk(_lib().sonde_softin_dev_counts(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("frames", "ecc_ok", "repaired", "symbols", "dropped"), [x.value for x in v]))
