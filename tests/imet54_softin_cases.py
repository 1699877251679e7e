"""Streams and arbiters shared by tests/test_softin_imet54_emu.py (the device iMet-54 soft-bit consumer under the CPU wave emulator), tests/test_imet54_decoded.py and
tests/test_gpu_softin_imet54.py (the same source as k_softin_imet54 on the device): symbol streams built from tools/synth.py frames, the host tier
sonde_imet54_dec_push_soft (pinned to the compiled reference by tests/test_imet54_native.py) as arbiter, and the emulator driver tests/emu/softin_imet54_emu.cpp.

The arbiter prints text only.  With `-r [--ecc]` a frame is its 108 bytes as hex, the tag [OK] / [ok] / [oo] / [NO] / [no] and, with --ecc and ecc_frm != 0,
`# (ecc_frm) [ecc_tlm]`.  ecc_std of a complete frame always equals ecc_frm (print_frame sets both in the same loop), so the line gives all three sums, and the tag
gives the two check-sum verdicts as far as the text depends on them.  Fed a symbol at a time, the arbiter prints a frame at the frame's last symbol: the header
matched 2200 symbols before that.  The arbiter does not print mv: the expected score is ref_score() — the reference's expression (float products, double sums in
order, sum / sqrt(normx * 40), rounded to float) on the 40 symbols the reference's ring holds at the hit, i.e. the last 40 symbols of the stream with the frame
bodies the arbiter found taken out (ring_at)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from tools import synth
from radiosonde_auto_rx_amd.family import Imet54Opts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_SRC = os.path.join(EMU_DIR, "softin_imet54_emu.cpp")
EMU_SO = os.path.join(EMU_DIR, "libsoftin_imet54_emu.so")
DEPS = [EMU_SRC, os.path.join(EMU_DIR, "wave_emu.h"), os.path.join(CSRC, "sonde_softin_imet54_dev.h"), os.path.join(CSRC, "sonde_softin_wave_dev.h"),
        os.path.join(CSRC, "sonde_rs_dev.h"), os.path.join(ROOT, "include", "sonde_hip.h")]
REF = os.path.join(ROOT, "oracle", "_ref", "imet54mod")
HEADER = "0000000001" "0101010101" "0001001001" "0001001001"          # the 40 header symbols `imet54mod` searches for: 00 AA 24 24 as 8N1
HDR = np.array([int(c) for c in HEADER], np.uint8)
NSYM = 2200                                                 # symbols of a frame behind the header
STAGE_MAX = 12288                                           # M10_STAGE_MAX of sonde_softin_wave_dev.h
CUTS = [4800, 1000, 251, 1, 9, 10, 11, 39, 40, 41, 63, 64, 65]
PRE, IDLE = 60, 30                                          # preamble and idle symbols of the short on-air frames the cases use


class Rec(C.Structure):
    """SoftinImet54Rec (csrc/sonde_softin_imet54_dev.h)"""
    _fields_ = [("channel", C.c_int32), ("mv", C.c_float), ("hdr_bit", C.c_uint64), ("inv", C.c_int32), ("ecc_frm", C.c_int32), ("ecc_tlm", C.c_int32),
                ("ecc_std", C.c_int32), ("crc_std", C.c_int32), ("crc_cont", C.c_int32), ("frame", C.c_uint8 * 108), ("pad", C.c_uint8 * 4)]


class EmuState(C.Structure):
    """EmuImet54State (tests/emu/softin_imet54_emu.cpp)"""
    _fields_ = [("mode", C.c_int), ("inv", C.c_int), ("done", C.c_int), ("carry_n", C.c_int), ("mv", C.c_float), ("pad", C.c_int), ("bits_in", C.c_uint64),
                ("hdr_bit", C.c_uint64), ("carry", C.c_float * 10), ("hist", C.c_float * 40)]


def load_emu(src=EMU_SRC, so=EMU_SO, deps=DEPS, flags=()):
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = so + ".%d.tmp" % os.getpid()
        # (-ffp-contract=off: the score is the reference's expression, every product and sum rounded on its own)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", *flags, "-o", tmp, src])
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.emu_imet54_run.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Rec), C.c_int,
                                 C.POINTER(C.c_int), C.POINTER(EmuState)]
    L.emu_imet54_end.argtypes = [C.c_char_p, C.c_int, C.POINTER(Rec)]
    L.emu_imet54_header_mask.restype = C.c_uint64
    return L


def load_host():
    from radiosonde_auto_rx_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    L = C.CDLL(engine.LIB_PATH)
    L.sonde_imet54_dec_create.argtypes = [C.POINTER(Imet54Opts), C.POINTER(C.c_void_p)]
    L.sonde_imet54_dec_destroy.argtypes = [C.c_void_p]
    L.sonde_imet54_dec_push_soft.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]
    L.sonde_imet54_dec_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_char_p, C.c_size_t]
    L.sonde_imet54_dec_decoded.argtypes = [C.c_void_p, C.c_char_p] + [C.c_int32] * 5 + [C.c_char_p, C.c_size_t]
    return L


def host_dec(H, **kw):
    h = C.c_void_p()
    if isinstance(kw.get("version"), str):
        kw["version"] = kw["version"].encode()
    o = Imet54Opts(**kw)
    assert H.sonde_imet54_dec_create(C.byref(o), C.byref(h)) == 0
    return h


# ---------------------------------------------------------------- records
def tag_of(r):
    """the tag print_frame gives a record (imet54mod.c crc tag: [OK] std, [ok] continuous, [oo] no codeword of the standard frame touched, [NO] / [no] by byte 0x52)"""
    g = (lambda k: r[k]) if isinstance(r, dict) else (lambda k: getattr(r, k))
    fr = bytes(g("frame"))
    if "crc" in (r if isinstance(r, dict) else ()):
        std, cont = r["crc"] == 1, r["crc"] == 2
    else:
        std, cont = bool(g("crc_std")), bool(g("crc_cont"))
    return "[OK]" if std else "[ok]" if cont else "[oo]" if g("ecc_std") == 0 else "[NO]" if fr[0x52] == 0xF8 else "[no]"


def raw_line(r, ecc=1):
    """the `-r [--ecc]` line of a record (a Rec or a fetch_imet54 dict)"""
    g = (lambda k: r[k]) if isinstance(r, dict) else (lambda k: getattr(r, k))
    line = bytes(g("frame")).hex().upper() + " " + tag_of(r)
    if ecc and g("ecc_frm") != 0:
        line += " # (%d) [%d]" % (g("ecc_frm"), g("ecc_tlm"))
    return line


def key(r, ecc=1):
    """(hdr_bit, frame, ecc_frm, ecc_tlm, ecc_std, tag) of a Rec, a fetch_imet54 dict or an arbiter tuple: what must agree exactly with the arbiter.  Without --ecc
    the arbiter prints no sums: hdr_bit, frame and tag then."""
    if isinstance(r, tuple):
        return r[:6] if ecc else r[:2] + r[5:6]
    g = (lambda k: r[k]) if isinstance(r, dict) else (lambda k: getattr(r, k))
    k = (g("hdr_bit"), bytes(g("frame")), g("ecc_frm"), g("ecc_tlm"), g("ecc_std"), tag_of(r))
    return k if ecc else k[:2] + k[5:6]


def full(r):
    """everything of a Rec the emulator must reproduce under any cut, mv bit for bit"""
    return (r.hdr_bit, bytes(r.frame), r.ecc_frm, r.ecc_tlm, r.ecc_std, r.crc_std, r.crc_cont, r.inv, struct.pack("<f", r.mv))


def mv_within_one_ulp(a, b):
    """two floats (the device's double divide and sqrt come ahead of the rounding to float: one ulp, as the M20 suite allows)"""
    ia, ib = struct.unpack("<i", struct.pack("<f", a))[0], struct.unpack("<i", struct.pack("<f", b))[0]
    return (ia < 0) == (ib < 0) and abs(ia - ib) <= 1


def parse_raw_line(line, ecc=1):
    """`-r [--ecc]` line -> (frame bytes, ecc_frm, ecc_tlm, tag)"""
    hexs, _, rest = line.partition(" ")
    fr = bytes.fromhex(hexs)
    assert len(fr) == 108, line
    tag = rest[:4]
    assert tag in ("[OK]", "[ok]", "[oo]", "[NO]", "[no]"), line
    if "#" in rest:
        assert ecc
        frm = int(rest.split("(")[1].split(")")[0]); tlm = int(rest.split("[")[2].split("]")[0])
    else:
        frm = tlm = 0
    return fr, frm, tlm, tag


_arb = {}


def host_frames(H, s, inv=0, softinv=False, aut=0, ecc=1, cache=None):
    """the arbiter: [(hdr_bit, frame bytes, ecc_frm, ecc_tlm, ecc_std, tag, `-r` line)] of the host tier over the whole stream, a symbol at a time (the frame is
    printed at its last symbol)"""
    if cache is not None and cache in _arb:
        return _arb[cache]
    s = np.ascontiguousarray(s, np.float32)
    h = host_dec(H, raw=1, ecc=ecc, inv=inv, aut=aut)
    out, buf = [], C.create_string_buffer(1024)
    base = s.ctypes.data
    for i in range(len(s)):
        n = H.sonde_imet54_dec_push_soft(h, base + 4 * i, 1, int(softinv), 0, buf, 1024)
        assert n >= 0
        if n:
            line = buf.raw[:n].decode().rstrip("\n")
            fr, frm, tlm, tag = parse_raw_line(line, ecc)
            out.append((i + 1 - NSYM, fr, frm, tlm, frm, tag, line))
    H.sonde_imet54_dec_destroy(h)
    if cache is not None:
        _arb[cache] = out
    return out


def host_text(H, s, inv=0, softinv=False, **kw):
    """what the host tier prints for the whole stream under the options kw"""
    s = np.ascontiguousarray(s, np.float32)
    h = host_dec(H, inv=inv, **kw)
    buf = C.create_string_buffer(1 << 20)
    n = H.sonde_imet54_dec_push_soft(h, s.ctypes.data, len(s), int(softinv), 0, buf, len(buf))
    assert n >= 0
    H.sonde_imet54_dec_destroy(h)
    return buf.raw[:n].decode()


def emu_frames(E, s, calls, inv=0, softinv=False, aut=0, ecc=1, cap=64):
    """the emulated consumer over the stream cut into calls (the last length repeats): Recs, frames dropped for want of room, end state"""
    s = np.ascontiguousarray(s, np.float32)
    buf = (Rec * (len(s) // NSYM + 2))()
    cl = (C.c_int * len(calls))(*calls)
    dropped, end = C.c_int(0), EmuState()
    n = E.emu_imet54_run(s.ctypes.data, len(s), cl, len(calls), int(softinv), int(inv), int(aut), int(ecc), cap, buf, len(buf), C.byref(dropped), C.byref(end))
    assert 0 <= n < len(buf), n
    for i in range(n):
        assert buf[i].channel == 0
    return [buf[i] for i in range(n)], dropped.value, end


def state(end):
    """the end state as far as it means anything: pending symbols and the frame position only inside a frame"""
    inside = end.mode == 1
    return (end.mode, end.inv, end.bits_in, [struct.pack("<f", v) for v in end.hist],
            (end.done, end.carry_n, [struct.pack("<f", v) for v in list(end.carry)[:end.carry_n]], end.hdr_bit, struct.pack("<f", end.mv)) if inside else None)


def ref_score(win):
    """corr_softhdb on 40 symbols (demod_mod.c:1692-1735): float products, double sums in order, sum / sqrt(normx * 40.0), rounded to float"""
    win = np.asarray(win, np.float32)
    assert len(win) == 40
    sm, nx = 0.0, 0.0
    for v, b in zip(win, HDR):
        y = np.float32(1.0 if b else -1.0)
        sm += float(np.float32(y * v)); nx += float(np.float32(v * v))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(np.float64(sm) / np.sqrt(np.float64(nx) * 40.0))


def ring_at(s, hdr_bits, at, softinv=False):
    """the reference's ring when `at` symbols have been read: the last 40 symbols seen while searching — the stream without the frame bodies behind hdr_bits —
    oldest first, zeros where the stream has not filled it"""
    s = np.asarray(s, np.float32) * np.float32(-1.0 if softinv else 1.0)
    keep = np.ones(len(s), bool)
    for hb in hdr_bits:
        keep[hb:hb + NSYM] = False
    keep[at:] = False
    seq = np.concatenate([np.zeros(40, np.float32), s[keep]])
    return seq[-40:]


# ---------------------------------------------------------------- frames and streams
def frame(k, **kw):
    return synth.imet54_frame(k, **kw)


def fbits(fr):
    """the 2200 bits of a frame behind the header"""
    return synth.imet54_frame_bits(fr)


def cwbit(j, i):
    """where bit i of codeword j lies among the 2200 frame bits: data bit j % 8 of character 3 + 8 (j / 8) + i"""
    return 10 * (3 + 8 * (j // 8) + i) + 1 + j % 8


def chars_of(bits):
    """the 220 characters of 2200 frame bits: data bit k of a character in bit k"""
    b = np.asarray(bits, np.uint8).reshape(220, 10)[:, 1:9]
    return bytes(int(sum(int(v) << k for k, v in enumerate(row))) for row in b)


def soft(sym, rng=None, jitter=(1.0, 1.0)):
    s = 2.0 * np.asarray(sym, np.float64) - 1.0
    if rng is not None:
        s = s * rng.uniform(jitter[0], jitter[1], len(s))
    return s.astype(np.float32)


def noise(rng, n, sigma=0.3):
    return rng.normal(0.0, sigma, n).astype(np.float32)


def onair(bits, pre=PRE, idle=IDLE):
    """preamble 00 AA .., the header, the frame bits, idle ones"""
    p = np.array([int(c) for c in ("0000000001" "0101010101") * ((pre + 19) // 20)], np.uint8)[:pre]
    return np.concatenate([p, HDR, np.asarray(bits, np.uint8), np.ones(idle, np.uint8)])


def damaged_bits(k, rng, nmax=2, **kw):
    """frame k with 0 .. nmax flipped bits in every codeword"""
    b = fbits(frame(k, **kw)).copy()
    for j in range(216):
        for i in rng.choice(8, int(rng.integers(0, nmax + 1)), replace=False):
            b[cwbit(j, int(i))] ^= 1
    return b


def hamming_bits():
    """name -> (2200 frame bits, ecc): the Hamming cases of the end-of-frame step"""
    c = {}
    base = fbits(frame(3))
    c["no_error"] = (base.copy(), 1)
    b = base.copy()
    for i in range(8):
        b[cwbit(10 + 9 * i, i)] ^= 1                                            # a flip in each of the 8 positions, codewords 10, 19, .., 73 (every row once)
    c["one_flip_each"] = (b, 1)
    for i in range(8):
        b = base.copy(); b[cwbit(5, i)] ^= 1
        c["flip_cw5_bit%d" % i] = (b, 1)
    b = base.copy(); b[cwbit(20, 1)] ^= 1; b[cwbit(20, 4)] ^= 1
    c["two_flips"] = (b, 1)
    for j in (0, 87, 88, 103, 104):
        b = base.copy(); b[cwbit(j, 0)] ^= 1; b[cwbit(j, 3)] ^= 1
        b[cwbit(40, 2)] ^= 1                                                    # and a repaired codeword ahead of 87
        c["f0_at_%d" % j] = (b, 1)
    for j in (87, 88, 103, 104):                                               # a repaired codeword on either side of both bounds
        b = base.copy(); b[cwbit(j, j % 8)] ^= 1
        c["fix_at_%d" % j] = (b, 1)
    b = base.copy(); b[2190:2200] = 1
    c["char220_set"] = (b, 1)
    b = base.copy(); b[2190:2200] = [1, 0, 1, 1, 0, 1, 0, 0, 1, 0]
    c["char220_mixed"] = (b, 1)
    b = base.copy(); b[cwbit(30, 6)] ^= 1
    c["ecc_off_damaged"] = (b, 0)
    c["ecc_off_clean"] = (base.copy(), 0)
    return c


def checksum_bits():
    """name -> (2200 frame bits, ecc): the check-sum cases; a byte flip re-encodes the frame, so no codeword is damaged by it"""
    c = {}
    for check in ("std", "cont", "none"):
        c["check_" + check] = (fbits(frame(4, check=check)), 1)
        for p in (0, 51, 52, 99, 100, 105, 107):
            f = bytearray(frame(4, check=check)); f[p] ^= 0x5A
            c["check_%s_flip%d" % (check, p)] = (fbits(bytes(f)), 1)
    f = bytearray(frame(5, check="none")); f[0x52] = 0x17
    c["none_not_f8"] = (fbits(bytes(f)), 1)                                     # [oo]: nothing repaired
    for name, fr in (("none_f8_repaired", frame(5, check="none")), ("none_not_f8_repaired", bytes(f))):
        b = fbits(fr).copy(); b[cwbit(7, 5)] ^= 1
        c[name] = (b, 1)                                                        # [NO] / [no]: ecc_std = 1
    b = fbits(frame(5, check="none")).copy(); b[cwbit(7, 5)] ^= 1
    c["none_ecc_off"] = (b, 0)
    c["std_ecc_off"] = (fbits(frame(5)), 0)
    return c


def eof_frames():
    """"eof_" + name -> (2200 frame bits, ecc): the frames of hamming_bits() and checksum_bits() that also run as streams (the end-of-frame step alone covers all)"""
    out = {}
    for name, v in list(hamming_bits().items()) + list(checksum_bits().items()):
        if name.startswith("flip_cw5_bit") or name.startswith("check_") and "flip" in name and not name.endswith(("flip52", "flip100")):
            continue
        out["eof_" + name] = v
    return out


# the stream cases and their options (inv = -i, softinv = --softinv, aut = --auto; --ecc on).  Kept apart from the streams, which need the host library to be built:
# a test module must not load libsonde_hip.so while it is collected (tests/conftest.py: PyTorch's HIP runtime has to come first in a GPU process), so the modules
# parametrise over case_opts() and build cases() inside their tests.
STREAM_OPTS = {"clean": {}, "sigma03": {}, "back_to_back": {}, "inverted_inv": dict(inv=1), "inverted_softinv": dict(softinv=True), "inverted_neither": {},
               "inverted_auto": dict(aut=1), "auto_flips_back": dict(aut=1), "zero_symbols": {}, "zero_symbols_inv": dict(inv=1), "flips_3": {}, "flips_4": {},
               "edge_below": {}, "edge_above": {}, "zero_window": {}, "ring_behind_frame": {}, "dropped_then_20": {}}


def case_opts():
    """name -> (inv, softinv, aut, ecc) of every case, without building a stream"""
    o = {k: (v.get("inv", 0), v.get("softinv", False), v.get("aut", 0), 1) for k, v in STREAM_OPTS.items()}
    o.update({k: (0, False, 0, ecc) for k, (_, ecc) in eof_frames().items()})
    return o


def _find_edge(H, flipped, rng_tail):
    """amplitudes a_lo < a_hi, adjacent floats, of one matching header symbol of a header with four flipped symbols (score exactly 0.8f at amplitude 1): the
    host framer finds the header at a_hi and not at a_lo.  (31 + a) / sqrt(40 (39 + a^2)) rises with a up to 39 / 31."""
    def found(a):
        s = soft(onair(fbits(frame(6)), pre=0))
        s[flipped] = -s[flipped]
        s[0] = np.float32(-a)                                                  # header symbol 0 is a 0: -1 at unit amplitude
        h = host_dec(H, raw=1, ecc=1)
        buf = C.create_string_buffer(4096)
        s = np.ascontiguousarray(np.concatenate([s, rng_tail]), np.float32)
        n = H.sonde_imet54_dec_push_soft(h, s.ctypes.data, len(s), 0, 0, buf, 4096)
        H.sonde_imet54_dec_destroy(h)
        return n > 0
    lo, hi = np.float32(1.0), np.float32(1.1)
    assert not found(lo) and found(hi)
    while np.nextafter(lo, np.float32(2.0)) < hi:
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        if found(mid):
            hi = mid
        else:
            lo = mid
    return lo, hi


def case_streams(H):
    """name -> dict(s, inv, softinv, aut, ecc, n = frames the arbiter must give)"""
    c = {}
    rng = np.random.default_rng(54)
    tail = lambda n=70: noise(rng, n, 0.05)                                        # noqa: E731
    # 1. clean, and sigma 0.3
    c["clean"] = dict(s=np.concatenate([tail(33)] + [soft(onair(fbits(frame(k)))) for k in range(3)] + [tail()]), n=3)
    c["sigma03"] = dict(s=np.concatenate([tail(17)] + [soft(onair(fbits(frame(k, check=("std", "cont", "none")[k])))) for k in range(3)] + [tail()]), n=3)
    c["sigma03"]["s"] = c["sigma03"]["s"] + noise(rng, len(c["sigma03"]["s"]), 0.3)
    # 2. back to back: the next header directly behind character 220
    c["back_to_back"] = dict(s=np.concatenate([tail(5)] + [soft(onair(fbits(frame(10 + k)), pre=0, idle=0)) for k in range(3)] + [tail()]), n=3)
    # 3. polarity
    pol = np.concatenate([tail(33), soft(onair(fbits(frame(7))), rng, (0.8, 1.2)), tail(140), soft(onair(fbits(frame(8))), rng, (0.8, 1.2)), tail(37)])
    c["inverted_inv"] = dict(s=-pol, inv=1, n=2)
    c["inverted_softinv"] = dict(s=-pol, softinv=True, n=2)
    c["inverted_neither"] = dict(s=-pol, n=0)
    c["inverted_auto"] = dict(s=-pol, aut=1, n=2, end_inv=1)
    half = np.concatenate([tail(21), soft(onair(fbits(frame(11))), rng, (0.8, 1.2)), tail(45)])
    c["auto_flips_back"] = dict(s=np.concatenate([-half, half]), aut=1, n=2, end_inv=0)
    # 4. exact zeros (and -0.0) where a data bit is 1: s >= 0 decides 1, then ^ inv
    b = fbits(frame(9))
    s = soft(onair(b), rng, (0.8, 1.2))
    ones = [PRE + 40 + p for p in range(2200) if b[p] and 1 <= p % 10 <= 8]
    for n_, p in enumerate(ones[5::97]):
        s[p] = np.float32(0.0) if n_ % 2 == 0 else np.float32(-0.0)
    c["zero_symbols"] = dict(s=np.concatenate([tail(50), s, tail()]), n=1)
    c["zero_symbols_inv"] = dict(s=np.concatenate([tail(50), -s, tail()]), inv=1, n=1)
    # 5. the threshold: 3 flipped header symbols score 34 / 40, 4 score 32 / 40 = 0.8 -> 0.8f, not greater
    for flips in (3, 4):
        s = soft(onair(fbits(frame(6)), pre=0))
        idx = np.array([3, 12, 26, 37][:flips])
        s[idx] = -s[idx]
        c["flips_%d" % flips] = dict(s=np.concatenate([tail(40), s, tail()]), n=1 if flips == 3 else 0)
    # ... and one symbol's amplitude moved until the host framer changes its mind: adjacent floats on both sides of the threshold
    t = tail()
    lo, hi = _find_edge(H, np.array([3, 12, 26, 37]), t)
    for name, a in (("edge_below", lo), ("edge_above", hi)):
        s = soft(onair(fbits(frame(6)), pre=0))
        s[[3, 12, 26, 37]] = -s[[3, 12, 26, 37]]
        s[0] = -a
        c[name] = dict(s=np.concatenate([s, t]), n=0 if name == "edge_below" else 1, amp=float(a))
    # 6. windows of exact zeros: 0 / 0 is no hit
    c["zero_window"] = dict(s=np.concatenate([np.zeros(45, np.float32), soft(onair(fbits(frame(14)), pre=20)), np.zeros(75, np.float32), soft(onair(fbits(frame(15)), pre=0)), tail()]), n=2)
    # 7. the ring behind a frame is the header it was found by: K symbols y right behind character 220 complete h1[K:] ++ y to a hit, where h1 is a header that is
    #    nearly silent wherever it disagrees with itself K symbols on — built by search with the arbiter over K (smallest first) so that the frame's own last
    #    symbols in the ring's place, or an emptied ring, give none.  The 220th character, which belongs to no block, is the inverse of the header's second one.
    b16 = fbits(frame(16)).copy(); b16[2190:2200] = 1 - HDR[10:20]
    for K in range(1, 40):
        h1 = soft(HDR)
        h1[[i for i in range(K, 40) if HDR[i] != HDR[i - K]]] *= np.float32(0.001)
        base = np.concatenate([tail(12), soft(onair([], pre=20, idle=0))[:20], h1, soft(b16)])
        y = soft(HDR[40 - K:])
        s = np.concatenate([base, y, soft(fbits(frame(17))), tail()])
        got = host_frames(H, s)
        if len(got) == 2 and got[0][0] == 72 and got[1][0] == len(base) + K:
            fed = np.concatenate([base[-(40 - K):], y])                            # what the ring would hold had the frame's symbols been fed into it
            emptied = np.concatenate([np.zeros(40 - K, np.float32), y])
            if not abs(ref_score(fed)) > np.float32(0.8) and not abs(ref_score(emptied)) > np.float32(0.8):
                c["ring_behind_frame"] = dict(s=s, n=2, K=K, at=len(base))
                break
    # 8. a dropped hit leaves the ring as it stands: a header of the other polarity whose last 20 symbols are nearly silent where they disagree with the first 20
    #    of a header of the right one, then the last 20 symbols of that: the second window is half of the dropped one
    first = -soft(HDR)
    clash = [20 + i for i in range(20) if first[20 + i] != soft(HDR)[i]]
    first[clash] *= np.float32(0.001)
    c["dropped_then_20"] = dict(s=np.concatenate([tail(30), first, soft(HDR[20:]), soft(fbits(frame(18))), tail()]), n=1, hdr_bit=30 + 60)
    for v in c.values():
        v.setdefault("inv", 0); v.setdefault("softinv", False); v.setdefault("aut", 0); v.setdefault("ecc", 1)
    # 9. the Hamming and check-sum frames of the end-of-frame step as streams (what the device suite runs)
    for name, (bits, ecc) in eof_frames().items():
        c[name] = dict(s=np.concatenate([tail(20), soft(onair(bits, pre=20), rng, (0.8, 1.2)), tail()]), n=1, inv=0, softinv=False, aut=0, ecc=ecc)
    assert {k: (v["inv"], v["softinv"], v["aut"], v["ecc"]) for k, v in c.items()} == case_opts()
    return c


_cases = None


def cases(H=None):
    global _cases
    if _cases is None:
        _cases = case_streams(H or load_host())
    return _cases


def stream_names():
    """the cases that are about the stream (searched, cut, replayed); the eof_ ones are single frames for the end-of-frame step"""
    return sorted(STREAM_OPTS)


def long_stream():
    """six frames at sigma 0.3, longer than the staging buffer"""
    rng = np.random.default_rng(540)
    s = np.concatenate([soft(onair(fbits(frame(20 + k)))) for k in range(6)] + [np.zeros(60, np.float32)])
    return s + noise(rng, len(s), 0.3)


def cap_stream(nframes=5):
    """frames back to back for one channel"""
    return np.concatenate([soft(onair(fbits(frame(30 + k)), pre=0, idle=0)) for k in range(nframes)])


def random_cuts(n, seed, lo=1, hi=5200):
    rng = np.random.default_rng(seed)
    out, tot = [], 0
    while tot < n:
        k = int(rng.integers(lo, hi))
        out.append(k); tot += k
    return out
