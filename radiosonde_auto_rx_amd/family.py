"""The rest of the decoder family behind the engine's generic sonde description: descriptors (what the reference's decoders put into dsp_t and pass to
find_header / read_softbit*) and ctypes bindings of their bit-rate tiers (include/sonde_lms6.h, sonde_meisei.h, sonde_imet54.h, sonde_mrz.h,
sonde_mts01.h, sonde_rs92.h).  Host-side; `FamilyDecoder.hit(h)` takes one dict of Engine(sonde="generic").fetch_hits() and returns the characters the
reference decoder prints for that header hit; `.json_objects(text)` picks the JSON lines out of them.

The scanner's type names (dft_detect.c:172-191) are the keys."""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np

from .engine import SondeError, lib

_I = C.c_int32


def _opts(names):
    return [(n, _I) for n in names] + [("version", C.c_char * 32), ("reserved", _I * 4)]


class Lms6Opts(C.Structure):
    _fields_ = [(n, _I) for n in ("raw", "ecc", "vit", "json", "typ", "gpsweek", "jsn_freq_khz")] + [("version", C.c_char * 32), ("reserved", _I * 4)]


class MeiseiOpts(C.Structure):
    _fields_ = _opts(("raw", "verbose", "dbg", "ecc", "json", "ptu", "ims100", "ref_year", "jsn_freq_khz"))


class Imet54Opts(C.Structure):
    _fields_ = _opts(("raw", "verbose", "ecc", "ptu", "silent", "json", "inv", "aut", "jsn_freq_khz"))


class MrzOpts(C.Structure):
    _fields_ = [(n, _I) for n in ("raw", "verbose", "dbg", "ptu", "uniq", "color", "json", "inv", "aut", "bits_ofs", "jsn_freq_khz")] + \
               [("version", C.c_char * 32), ("bits_ofs_given", _I), ("reserved", _I * 3)]


class Mts01Opts(C.Structure):
    _fields_ = _opts(("raw", "verbose", "json", "jsn_freq_khz"))


class Rs92Opts(C.Structure):
    _fields_ = [(n, _I) for n in ("raw", "verbose", "aux", "ecc", "ptu", "inv", "ngp", "dbg", "json", "gps_verbose", "gps_iter", "gps_vel", "exsat", "gpsepoch")] + \
               [("dop_limit", C.c_float), ("d_err", C.c_float), ("jsn_freq_khz", _I), ("version", C.c_char * 32), ("reserved", _I * 4)]


# RS92 sends raw GPS ranges: its decoder needs orbit data (auto_rx downloads a RINEX navigation file per flight, decode.py:423-446)
RS92_ORBITS = {"ephemeris": None, "almanac": None}


def set_rs92_orbits(ephemeris: str | None = None, almanac: str | None = None):
    RS92_ORBITS.update(ephemeris=ephemeris, almanac=almanac)


# generic = sonde_generic_t; thres / keep_soft / auto = engine configuration; pol: what the decoder wants — "raw" (un-flip the engine's bits when the
# header score is negative), "engine" (bits in the polarity in effect, as stored)
FAMILY = {
    "LMS6": dict(generic=dict(header="0101011000001000" "0001110010010111" "0001101010100111" "0011110100111110", baud=4800.0, bt=1.2, h=0.9, symlen=1, symhd=1,
                              hdmax=10, bitofs=0, nbits=261 * 16 - 80, l_win=-1.0, lpiq_bw=16000, lpfm_bw=6000),      # lms6Xmod.c:100,1283-1305,1358
                 thres=0.65, auto=True, pol="raw", prefix="lms6", opts=Lms6Opts, kw=dict(ecc=1, vit=2, json=1), sep_hz=8000.0),
    "MEISEI": dict(generic=dict(header="101010101011010100101011001101001100101011001101", baud=2400.0, bt=1.2, h=2.4, symlen=1, symhd=1,
                                hdmax=1, bitofs=0, nbits=1152, l_win=-1.0, lpiq_bw=16000, lpfm_bw=4000),               # meisei100mod.c:200,626-644,690
                   thres=0.7, auto=True, pol="engine", prefix="meisei", opts=MeiseiOpts, kw=dict(ecc=1, json=1, ptu=1), sep_hz=12000.0),
    "IMET5": dict(generic=dict(header="0000000001" "0101010101" "0001001001" "0001001001", baud=4798.0, bt=1.0, h=0.8, symlen=1, symhd=1,
                               hdmax=4, bitofs=1, nbits=2200, l_win=2.0, lpiq_bw=7400, lpfm_bw=6000),                  # imet54mod.c:91-98,945-962,1013
                  thres=0.7, auto=False, pol="engine", prefix="imet54", opts=Imet54Opts, kw=dict(ecc=1, json=1, ptu=1), sep_hz=8000.0),
    "MRZ": dict(generic=dict(header="100110011001100110011001100110011001" "10101010", baud=2399.0, bt=1.0, h=2.0, symlen=2, symhd=2,
                             hdmax=2, bitofs=2, nbits=386, l_win=2.0, lpiq_bw=9000, lpfm_bw=6000),                     # mp3h1mod.c:117,1112-1131,1181
                thres=0.76, auto=False, pol="engine", prefix="mrz", opts=MrzOpts, kw=dict(json=1, ptu=1, uniq=1), sep_hz=10000.0),
    "RS92": dict(generic=dict(header="10100110011001101001" "1010011001100110100110101010100110101001", baud=4800.0, bt=0.5, h=0.8, symlen=2, symhd=2,
                              hdmax=3, bitofs=2, nbits=2340, l_win=4.0, lpiq_bw=8000, lpfm_bw=6000),                   # rs92mod.c:88-92,1914-1943,1992
                 thres=0.7, auto=False, pol="engine", prefix="rs92", opts=Rs92Opts, kw=dict(verbose=1, aux=1, ecc=2, gps_vel=4, json=1, gpsepoch=-1), sep_hz=8000.0),
    "MTS01": dict(generic=dict(header="10101010" "10101010" "10110100" "00101011", baud=1200.0, bt=1.5, h=0.9, symlen=1, symhd=1,
                               hdmax=2, bitofs=0, nbits=1048, l_win=2.0, lpiq_bw=4000, lpfm_bw=4000),                  # mts01mod.c:47-48,514-533,575
                  thres=0.76, auto=True, pol="raw", prefix="mts01", opts=Mts01Opts, kw=dict(json=1), sep_hz=6000.0),
}


# An LMS6 whose blocks turn out to be LMS-X (lms6Xmod.c:1436-1462): same filters and header, bit clock 4797.8 Bd and 4720 bits per block.  Not a scanner type:
# the receivers move a sonde to an engine of this description when its decoder object reports the change (FamilyDecoder.lms_type), and back.
FAMILY["LMSX"] = dict(FAMILY["LMS6"], generic=dict(FAMILY["LMS6"]["generic"], slice_baud=4797.8, nbits=300 * 16 - 80))
LMS_BASE = {"LMSX": "LMS6"}                      # receiver bookkeeping: the scanner's name of a sonde's type


# The kinds whose hits a generic engine decodes on the device (sonde_engine_set_family, include/sonde_hip.h): FAMILY key -> SONDE_* kind.  DEVICE_KINDS are the four
# of k_family_hits, one verdict per hit; MRZ (k_mrz_hits) comes with a verdict for either frame length and its --ofs, so it has entries of its own
# (decode_mrz_hits_device, Engine.set_family's bits_ofs).  Membership is asked of DEVICE_KINDS_ALL.  LMS6 / LMS-X (k_lms6_hits) have a record type of their own
# — a block has up to 308 bytes — so they are DEVICE_KINDS_LMS, with Lms6Hit, decode_lms6_hits_device and Engine.set_family's vit.
DEVICE_KINDS = {"MEISEI": 11, "IMET5": 54, "MTS01": 71, "RS92": 92}
DEVICE_KINDS_ALL = dict(DEVICE_KINDS, MRZ=31)
DEVICE_KINDS_LMS = {"LMS6": 6, "LMSX": 6}


class FamilyHit(C.Structure):
    """sonde_family_hit_t (include/sonde_hip.h)"""
    _fields_ = [("channel", _I), ("kind", _I), ("nbits", _I), ("decoded", _I), ("mv_pos", C.c_uint32), ("mv", C.c_float), ("v", _I * 6), ("aux", C.c_uint8 * 12),
                ("data", C.c_uint8 * 240)]


def family_hit_dict(r: FamilyHit) -> dict:
    return dict(channel=r.channel, kind=r.kind, nbits=r.nbits, decoded=r.decoded, mv_pos=r.mv_pos, mv=r.mv, v=list(r.v), aux=bytes(r.aux), data=bytes(r.data))


def decode_hits_device(kind: str, hits, ecc: int = 1):
    """The engines' per-hit device decoder (k_family_hits) on hits in host memory (sonde_family_decode_device): kind = a key of DEVICE_KINDS, hits = float32 soft-bit
    arrays as the engine stores them, each up to the kind's frame length (a shorter one comes back with decoded = 0).  -> dicts; channel = the hit's index."""
    nb = FAMILY[kind]["generic"]["nbits"]
    soft = np.zeros((max(len(hits), 1), nb), np.float32)
    n = np.zeros(max(len(hits), 1), np.int32)
    for i, h in enumerate(hits):
        h = np.asarray(h, np.float32)
        soft[i, :len(h)] = h
        n[i] = len(h)
    out = (FamilyHit * max(len(hits), 1))()
    fn = lib().sonde_family_decode_device
    fn.argtypes = [_I, _I, C.c_void_p, C.c_int64, C.c_void_p, _I, C.POINTER(FamilyHit)]
    rc = fn(DEVICE_KINDS[kind], int(ecc), soft.ctypes.data, nb, n.ctypes.data, len(hits), out)
    if rc < 0:
        raise SondeError(f"sonde_family_decode_device: {lib().sonde_strerror(rc).decode()} ({rc})")
    return [family_hit_dict(out[i]) for i in range(len(hits))]


def decode_mrz_hits_device(hits, bits_ofs: int = 8):
    """The engines' per-hit MRZ decoder (k_mrz_hits) on hits in host memory (sonde_mrz_decode_device): hits = float32 soft-bit arrays as the engine stores them, each
    up to 386 long (a shorter one comes back with decoded = 0); bits_ofs = the decoder's --ofs.  -> dicts; channel = the hit's index."""
    nb = FAMILY["MRZ"]["generic"]["nbits"]
    soft = np.zeros((max(len(hits), 1), nb), np.float32)
    n = np.zeros(max(len(hits), 1), np.int32)
    for i, h in enumerate(hits):
        h = np.asarray(h, np.float32)
        soft[i, :len(h)] = h
        n[i] = len(h)
    out = (FamilyHit * max(len(hits), 1))()
    fn = lib().sonde_mrz_decode_device
    fn.argtypes = [_I, C.c_void_p, C.c_int64, C.c_void_p, _I, C.POINTER(FamilyHit)]
    rc = fn(int(bits_ofs), soft.ctypes.data, nb, n.ctypes.data, len(hits), out)
    if rc < 0:
        raise SondeError(f"sonde_mrz_decode_device: {lib().sonde_strerror(rc).decode()} ({rc})")
    return [family_hit_dict(out[i]) for i in range(len(hits))]


class Lms6Hit(C.Structure):
    """sonde_lms6_hit_t (include/sonde_hip.h)"""
    _fields_ = [("channel", _I), ("kind", _I), ("nbits", _I), ("decoded", _I), ("mv_pos", C.c_uint32), ("mv", C.c_float), ("len", _I), ("blen", _I), ("err", _I),
                ("vit", _I), ("bytes", C.c_uint8 * 308)]


def lms6_hit_dict(r: Lms6Hit) -> dict:
    return dict(channel=r.channel, kind=r.kind, nbits=r.nbits, decoded=r.decoded, mv_pos=r.mv_pos, mv=r.mv, len=r.len, blen=r.blen, err=r.err, vit=r.vit,
                bytes=bytes(r.bytes))


def decode_lms6_hits_device(hits, mvs, vit: int = 2, lmsx: bool = False):
    """The engines' per-hit LMS6 / LMS-X decoder (k_lms6_hits) on hits in host memory (sonde_lms6_decode_device): hits = float32 soft-bit arrays as the engine
    stores them, each up to 4096 (lmsx: 4720) long (a shorter one comes back with decoded = 0); mvs = their header scores, whose sign is the phase of the raw bits'
    sign alternation; vit = 1 (--vit) or 2 (--vit2).  -> dicts; channel = the hit's index."""
    nb = FAMILY["LMSX" if lmsx else "LMS6"]["generic"]["nbits"]
    if len(mvs) != len(hits):
        raise SondeError("decode_lms6_hits_device: a header score per hit")
    soft = np.zeros((max(len(hits), 1), nb), np.float32)
    n = np.zeros(max(len(hits), 1), np.int32)
    mv = np.zeros(max(len(hits), 1), np.float32)
    for i, h in enumerate(hits):
        h = np.asarray(h, np.float32)
        if len(h) > nb:
            raise SondeError(f"decode_lms6_hits_device: hit {i} has {len(h)} soft bits, a block has {nb}")
        soft[i, :len(h)] = h
        n[i] = len(h)
        mv[i] = mvs[i]
    out = (Lms6Hit * max(len(hits), 1))()
    fn = lib().sonde_lms6_decode_device
    fn.argtypes = [_I, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, _I, C.POINTER(Lms6Hit)]
    rc = fn(int(vit), soft.ctypes.data, nb, n.ctypes.data, mv.ctypes.data, len(hits), out)
    if rc < 0:
        raise SondeError(f"sonde_lms6_decode_device: {lib().sonde_strerror(rc).decode()} ({rc})")
    return [lms6_hit_dict(out[i]) for i in range(len(hits))]


class Lms6RsHyp(C.Structure):
    """sonde_lms6_rs_hyp_t (include/sonde_hip.h)"""
    _fields_ = [("at", _I), ("err", _I), ("pos", C.c_uint8 * 16), ("val", C.c_uint8 * 16)]


class Lms6Rs(C.Structure):
    """sonde_lms6_rs_t (include/sonde_hip.h): RS(255,223) of one LMS6 / LMS-X block under the three hypotheses the host decoder can ask for"""
    _fields_ = [("h6", Lms6RsHyp), ("hX", Lms6RsHyp), ("h6X", Lms6RsHyp)]


def decode_lms6_rs_device(blocks, blen):
    """RS(255,223) of LMS6 / LMS-X blocks on the device (k_lms6_rs) on block records in host memory (sonde_lms6_rs_device): blocks = their block bytes (up to 308
    each, zero behind blen[i]); -> a list of Lms6Rs, for FamilyDecoder.decoded(rec, rs=..)."""
    n = len(blocks)
    if len(blen) != n:
        raise SondeError("decode_lms6_rs_device: a block length per block")
    by = np.zeros((max(n, 1), 308), np.uint8)
    for i, b in enumerate(blocks):
        b = np.frombuffer(bytes(b), np.uint8)
        if len(b) > 308:
            raise SondeError(f"decode_lms6_rs_device: block {i} has {len(b)} bytes, a block has at most 308")
        by[i, :len(b)] = b
    bl = np.ascontiguousarray(list(blen) + [0] * (1 - min(n, 1)), np.int32)
    out = (Lms6Rs * max(n, 1))()
    fn = lib().sonde_lms6_rs_device
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, _I, C.POINTER(Lms6Rs)]
    rc = fn(by.ctypes.data, 308, bl.ctypes.data, n, out)
    if rc < 0:
        raise SondeError(f"sonde_lms6_rs_device: {lib().sonde_strerror(rc).decode()} ({rc})")
    return [Lms6Rs.from_buffer_copy(out[i]) for i in range(n)]


class FamilyDecoder:
    """one decoder object of type `typ` (a key of FAMILY): state lives across hits like the reference's gpx_t"""

    def __init__(self, typ: str, /, *, freq_khz: int = 0, version: str = "sonde_hip", **kw):
        # (typ is positional only: the LMS6 decoder has an option of that name, 0 = auto detection, 6 = --lms6, 10 = --lmsX)
        self.typ, self.f = typ, FAMILY[typ]
        L = lib()
        p = self.f["prefix"]
        self._create, self._destroy = getattr(L, f"sonde_{p}_dec_create"), getattr(L, f"sonde_{p}_dec_destroy")
        self._create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        self._destroy.argtypes = [C.c_void_p]
        okw = {k: v for k, v in kw.items() if k not in ("ephemeris", "almanac")}
        o = self.f["opts"](**{**self.f["kw"], **okw}, jsn_freq_khz=freq_khz, version=version.encode())
        self._h = C.c_void_p()
        if self._create(C.byref(o), C.byref(self._h)) < 0:
            raise SondeError(f"sonde_{p}_dec_create: unsupported options")
        self._buf = C.create_string_buffer(1 << 16)
        if typ == "LMS6":
            self._fn = L.sonde_lms6_dec_block
            self._fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _I, C.c_float, C.c_float, C.c_double, C.c_char_p, C.c_size_t]
            L.sonde_lms6_dec_block_bits.argtypes = [C.c_void_p]
            L.sonde_lms6_dec_vit.argtypes = [C.c_void_p, C.POINTER(_I)]
            self._last_pos = 0
        else:
            self._fn = getattr(L, f"sonde_{p}_dec_frame")
            self._fn.argtypes = [C.c_void_p, C.c_void_p, _I, C.c_char_p, C.c_size_t]
        if typ == "MRZ":
            L.sonde_mrz_dec_frame_bits.argtypes = [C.c_void_p]
            self.bits_ofs = int(o.bits_ofs) if o.bits_ofs_given else 8     # --ofs as sonde_mrz_dec_create takes it: a device record must have been made under it
        if typ == "RS92":                                              # without orbit data: frames and JSON-less text only, as `rs92mod` without -e / -a
            for kind in ("almanac", "ephemeris"):
                path = kw.get(kind) or RS92_ORBITS[kind]
                fn = getattr(L, f"sonde_rs92_dec_load_{kind}")
                fn.argtypes = [C.c_void_p, C.c_char_p]
                if path and fn(self._h, os.fsencode(path)) < 0:
                    raise SondeError(f"RS92: {kind} file {path} not readable as such")

    def close(self):
        if getattr(self, "_h", None):
            self._destroy(self._h)
            self._h = None

    __del__ = close

    def _lms_rate(self, mv_pos: int, if_sr: int) -> float:
        """LMS6: frm_rate of the block behind the header at mv_pos, from the header before it (lms6Xmod.c:1372)"""
        d = (int(mv_pos) - self._last_pos) & 0xFFFFFFFF
        rate = 4800.0 * if_sr / d if d else float("inf")
        if getattr(self, "moved", False):                                  # first block on another engine (receivers, LMS6 <-> LMS-X): no header position to take the
            rate, self.moved = 4800.0, False                              # frame rate from; a rate outside 4000..5000 would send the decoder back (lms6Xmod.c:959)
        self._last_pos = int(mv_pos)
        return rate

    def lms_block_bits(self) -> int:
        """LMS6 only: raw bits the decoder reads behind a header for the type in effect, 4096 or 4720"""
        return lib().sonde_lms6_dec_block_bits(self._h)

    def hit(self, h: dict, if_sr: int = 48000) -> str:
        soft = np.ascontiguousarray(h["soft"], np.float32)
        if self.f["pol"] == "raw" and h["mv"] < 0:
            soft = -soft
        n = len(soft)
        if self.typ == "LMS6":
            n = min(n, lib().sonde_lms6_dec_block_bits(self._h))           # a decoder that went over to LMS-X wants more bits than a fixed description slices
            rate = self._lms_rate(h["mv_pos"], if_sr)
            k = self._fn(self._h, soft.ctypes.data, None, n, h["mv"], rate, (h["mv_pos"] + n * if_sr / 4800.0) / if_sr, self._buf, len(self._buf))
        else:
            if self.typ == "MRZ":
                n = min(n, lib().sonde_mrz_dec_frame_bits(self._h))
            k = self._fn(self._h, soft.ctypes.data, n, self._buf, len(self._buf))
        if k < 0:
            raise SondeError(f"{self.typ}: decoder call failed ({k})")
        return self._buf.raw[:k].decode(errors="replace")

    def lms_rs_stats(self):
        """LMS6 only: (RS results taken from device records, decoded here instead) over the decoded(rec, rs=..) calls so far (sonde_lms6_dec_rs_stats)"""
        u, m = C.c_int64(0), C.c_int64(0)
        fn = lib().sonde_lms6_dec_rs_stats
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        fn(self._h, C.byref(u), C.byref(m))
        return u.value, m.value

    def decoded(self, rec: dict, if_sr: int = 48000, rs=None) -> str:
        """one dict of Engine.fetch_family(): the characters the reference decoder prints for that hit, from the device's bytes and verdicts (no block code runs
        here).  A record the device did not decode (decoded = 0: a hit cut short by the end of input, or device decoding switched off) goes through hit() on its
        soft bits.  LMS6: so does a record longer than the block this decoder reads (an LMS6 decoder on an LMS-X engine, in the block of the change) — it has to
        carry its soft bits (Engine.fetch_family's need_soft); a record no longer than that is what hit() would have decoded (an LMS-X decoder still on an LMS6
        engine reads the 4096 bits that exist)."""
        if not rec["decoded"]:
            return self.hit(rec, if_sr)
        if self.typ == "LMS6":
            ecc = _I(0)
            vit = lib().sonde_lms6_dec_vit(self._h, C.byref(ecc))
            if vit != rec["vit"] or ecc.value == 3:
                raise SondeError(f"LMS6: the record was decoded with vit = {rec['vit']}, this decoder has vit = {vit}, ecc = {ecc.value}")
            n = rec["nbits"]
            if n > self.lms_block_bits():
                if "soft" not in rec:
                    raise SondeError(f"LMS6: a record of {n} bits for a decoder that reads {self.lms_block_bits()}: its soft bits are needed (fetch_family's need_soft)")
                return self.hit(rec, if_sr)
            rate = self._lms_rate(rec["mv_pos"], if_sr)
            rs = rs if rs is not None else rec.get("rs")
            t_end = (rec["mv_pos"] + n * if_sr / 4800.0) / if_sr
            if rs is not None:                                             # the device's RS(255,223) record beside the hit (Engine.fetch_family under rs=True)
                fn = lib().sonde_lms6_dec_block_rs
                fn.argtypes = [C.c_void_p, C.c_char_p, _I, _I, C.c_float, C.c_float, C.c_double, C.POINTER(Lms6Rs), C.c_char_p, C.c_size_t]
                k = fn(self._h, rec["bytes"][:rec["blen"]], rec["blen"], rec["len"], rec["mv"], rate, t_end, C.byref(rs), self._buf, len(self._buf))
            else:
                fn = lib().sonde_lms6_dec_block_bytes
                fn.argtypes = [C.c_void_p, C.c_char_p, _I, _I, C.c_float, C.c_float, C.c_double, C.c_char_p, C.c_size_t]
                k = fn(self._h, rec["bytes"][:rec["blen"]], rec["blen"], rec["len"], rec["mv"], rate, t_end, self._buf, len(self._buf))
            if k < 0:
                raise SondeError(f"LMS6: sonde_lms6_dec_block_bytes failed ({k})")
            return self._buf.raw[:k].decode(errors="replace")
        L, p, d, v = lib(), self.f["prefix"], rec["data"], rec["v"]
        if self.typ == "MEISEI":
            L.sonde_meisei_dec_decoded.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]
            k = L.sonde_meisei_dec_decoded(self._h, d[:75], rec["aux"], self._buf, len(self._buf))
        elif self.typ == "IMET5":
            L.sonde_imet54_dec_decoded.argtypes = [C.c_void_p, C.c_char_p] + [_I] * 5 + [C.c_char_p, C.c_size_t]
            k = L.sonde_imet54_dec_decoded(self._h, d[:108], v[0], v[1], v[2], v[3], v[4], self._buf, len(self._buf))
        elif self.typ == "MTS01":
            L.sonde_mts01_dec_decoded.argtypes = [C.c_void_p, C.c_char_p, _I, _I, C.c_char_p, C.c_size_t]
            k = L.sonde_mts01_dec_decoded(self._h, d[:131], v[0], v[2], self._buf, len(self._buf))
        elif self.typ == "RS92":
            L.sonde_rs92_dec_corrected.argtypes = [C.c_void_p, C.c_char_p, _I, C.c_char_p, C.c_size_t]
            k = L.sonde_rs92_dec_corrected(self._h, d[:240], v[0], self._buf, len(self._buf))
        elif self.typ == "MRZ":
            # the device gave the CRC verdict under both frame lengths (k_mrz_hits): this decoder's state says which one it would have read the hit with
            if v[5] != self.bits_ofs:
                raise SondeError(f"MRZ: the record was decoded with --ofs {v[5]}, this decoder has --ofs {self.bits_ofs}")
            nb = L.sonde_mrz_dec_frame_bits(self._h) + 22
            L.sonde_mrz_dec_decoded.argtypes = [C.c_void_p, C.c_char_p, _I, _I, C.c_char_p, C.c_size_t]
            k = L.sonde_mrz_dec_decoded(self._h, d[:52], nb, v[0] if nb == 408 else v[1], self._buf, len(self._buf))
        else:
            raise SondeError(f"{self.typ}: hits of this type are not decoded on the device")
        if k < 0:
            raise SondeError(f"{self.typ}: sonde_{p}_dec_decoded failed ({k})")
        return self._buf.raw[:k].decode(errors="replace")

    def lms_type(self):
        """LMS6 only: ("LMS6" | "LMSX" = the description the decoder wants its demodulator on, whether the last block made it change)"""
        ch = _I(0)
        L = lib()
        L.sonde_lms6_dec_type.argtypes = [C.c_void_p, C.POINTER(_I)]
        t = L.sonde_lms6_dec_type(self._h, C.byref(ch))
        return ("LMSX" if (t & 0xFF) == 10 else "LMS6"), bool(ch.value)

    @staticmethod
    def json_objects(text: str):
        return [json.loads(l) for l in text.splitlines() if l.startswith("{")]


def rs92_text_batch(decoders, records, solver, if_sr: int = 48000):
    """FamilyDecoder.decoded for the records of Engine.fetch_family() on an RS92 engine, with the position solve's 4-satellite subset search of all of them on the
    device (gps.GpsSolver; None = the host's search): decoders[channel] = that channel's RS92 FamilyDecoder (a dict or a sequence), records in fetch order.  A
    channel's records pass through its decoder in order, several of one channel in rounds.  -> the text of each record, the same characters as
    decoders[rec["channel"]].decoded(rec) gives one record at a time.  A record the device did not decode (decoded = 0) goes through hit() in its place."""
    from . import gps
    texts, run = [None] * len(records), []

    def flush():
        if run:
            got = gps.text_batch(solver, [decoders[records[i]["channel"]]._h for i in run], [records[i]["data"][:240] for i in run], [records[i]["v"][0] for i in run])
            for i, t in zip(run, got):
                texts[i] = t
            run.clear()
    for i, rec in enumerate(records):
        d = decoders[rec["channel"]]
        if d.typ != "RS92":
            raise SondeError("rs92_text_batch: an RS92 decoder per channel")
        if rec["decoded"]:
            run.append(i)
        else:
            flush()
            texts[i] = d.hit(rec, if_sr)
    flush()
    return texts
