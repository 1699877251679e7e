"""Streams and arbiters shared by tests/test_softin_mts01_emu.py (the device MTS01 soft-bit consumer under the CPU wave emulator), tests/test_mts01_decoded.py and
tests/test_gpu_softin_mts01.py (the same source as k_softin_mts01 on the device): symbol streams built from tools/synth.py frames, the host tier
sonde_mts01_dec_push_soft (pinned to the compiled reference by the family suites) as arbiter, and the emulator driver tests/emu/softin_mts01_emu.cpp.

The arbiter prints text only: with `-r` the 131 bytes as hex, ` # [crcdat:crcval]` and the verdict — everything a record holds but hdr_bit and mv.  Fed a symbol at a
time it prints a frame at the frame's last symbol: the header matched 1048 symbols before that.  model_frame() makes the same line from the symbols behind the hit
and a CRC-16 computed here; host_frames() asserts for every frame that the model's line IS the arbiter's.  The expected score is ref_score() — the reference's
expression (float products, double sums in order, sum / sqrt(normx * 32), rounded to float) on the 32 symbols the reference's ring holds at the hit, i.e. the last
32 of the stream with the frame bodies the arbiter found taken out (ring_at)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from tools import synth
from radiosonde_auto_rx_amd.family import Mts01Opts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_SRC = os.path.join(EMU_DIR, "softin_mts01_emu.cpp")
EMU_SO = os.path.join(EMU_DIR, "libsoftin_mts01_emu.so")
DEPS = [EMU_SRC, os.path.join(EMU_DIR, "wave_emu.h"), os.path.join(CSRC, "sonde_softin_mts01_dev.h"), os.path.join(CSRC, "sonde_softin_wave_dev.h"),
        os.path.join(CSRC, "sonde_rs_dev.h"), os.path.join(ROOT, "include", "sonde_hip.h")]
REF = os.path.join(ROOT, "oracle", "_ref", "mts01mod")
HEADER = "10101010" "10101010" "10110100" "00101011"         # the 32 header symbols `mts01mod` searches for: AA AA B4 2B
HDR = np.array([int(c) for c in HEADER], np.uint8)
HL = 32
NSYM = 1048                                                 # symbols = bits of a frame behind the header
FRAME = HL + NSYM                                           # 1080: the spacing of back-to-back frames
STAGE_MAX = 12288                                           # M10_STAGE_MAX of sonde_softin_wave_dev.h
CUTS = [2400, 1000, 251, 1, 2, 31, 32, 33, 63, 64, 65]
F08 = np.float32(0.8)


class Rec(C.Structure):
    """SoftinMts01Rec (csrc/sonde_softin_mts01_dev.h)"""
    _fields_ = [("channel", C.c_int32), ("mv", C.c_float), ("hdr_bit", C.c_uint64), ("crcval", C.c_uint16), ("crcdat", C.c_uint16), ("crc_ok", C.c_uint8),
                ("bytes", C.c_uint8 * 131)]


class EmuState(C.Structure):
    """EmuMts01State (tests/emu/softin_mts01_emu.cpp)"""
    _fields_ = [("mode", C.c_int), ("done", C.c_int), ("mv", C.c_float), ("pad", C.c_int), ("bits_in", C.c_uint64), ("hdr_bit", C.c_uint64),
                ("hist", C.c_float * 32), ("w", C.c_uint32 * 33), ("pad2", C.c_int)]


def load_emu(src=EMU_SRC, so=EMU_SO, deps=DEPS, flags=()):
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = so + ".%d.tmp" % os.getpid()
        # (-ffp-contract=off: the score is the reference's expression, every product and sum rounded on its own)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", *flags, "-o", tmp, src])
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.emu_mts01_run.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(Rec), C.c_int, C.POINTER(C.c_int), C.POINTER(EmuState)]
    L.emu_mts01_crc.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    L.emu_mts01_header_mask.restype = C.c_uint64
    return L


def load_host():
    from radiosonde_auto_rx_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    L = C.CDLL(engine.LIB_PATH)
    L.sonde_mts01_dec_create.argtypes = [C.POINTER(Mts01Opts), C.POINTER(C.c_void_p)]
    L.sonde_mts01_dec_destroy.argtypes = [C.c_void_p]
    L.sonde_mts01_dec_push_soft.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]
    L.sonde_mts01_dec_decoded.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]
    return L


def host_dec(H, **kw):
    h = C.c_void_p()
    if isinstance(kw.get("version"), str):
        kw["version"] = kw["version"].encode()
    o = Mts01Opts(**kw)
    assert H.sonde_mts01_dec_create(C.byref(o), C.byref(h)) == 0
    return h


# ---------------------------------------------------------------- the model of a frame
def crc16_re(data, init=0xFFFF, reverse=True):
    rem = init
    for b in bytes(data):
        rem ^= b << 8
        for _ in range(8):
            rem = ((rem << 1) ^ 0x8005) & 0xFFFF if rem & 0x8000 else (rem << 1) & 0xFFFF
    return int("%s" % format(rem, "016b")[::-1], 2) if reverse else rem


def verdict(by131):
    """(crcval, crcdat, crc_ok) of 131 frame bytes: crc16_re over bytes 1 .. 128 against bytes[130] << 8 | bytes[129]"""
    f = bytes(by131)
    val, dat = crc16_re(f[1:129]), f[130] << 8 | f[129]
    return val, dat, int(val == dat)


def line_of(by131, val, ok):
    f = bytes(by131)
    return "".join("%02X " % v for v in f) + " # [%04X:%04X]" % (f[130] << 8 | f[129], val) + " # [%s]" % ("OK" if ok else "NO")


def model_frame(sym):
    """(bytes131, crcval, crcdat, crc_ok, the `-r` line) of the 1048 symbols behind a hit: a bit per symbol, (s >= 0), read raw"""
    by = bytes(np.packbits((np.asarray(sym, np.float32) >= 0).astype(np.uint8)))
    val, dat, ok = verdict(by)
    return by, val, dat, ok, line_of(by, val, ok)


def _g(r):
    return (lambda k: r[k]) if isinstance(r, dict) else (lambda k: getattr(r, k))


def raw_line(r):
    """the `-r` line of a record (a Rec or a fetch_mts01 dict) from its bytes, ITS CRC value and ITS verdict"""
    g = _g(r)
    return line_of(bytes(g("bytes")), g("crcval"), g("crc_ok"))


def key(r):
    """(hdr_bit, the 131 bytes, crcval, crcdat, crc_ok) of a Rec, a fetch_mts01 dict or an arbiter tuple: what must agree exactly with the arbiter"""
    if isinstance(r, tuple):
        return r[:5]
    g = _g(r)
    return (g("hdr_bit"), bytes(g("bytes")), g("crcval"), g("crcdat"), g("crc_ok"))


def full(r):
    """everything of a Rec the emulator must reproduce under any cut, mv bit for bit"""
    return key(r) + (struct.pack("<f", r.mv),)


def mv_within_one_ulp(a, b):
    """two floats (the device's double divide and sqrt come ahead of the rounding to float: one ulp, as the other device suites allow)"""
    ia, ib = struct.unpack("<i", struct.pack("<f", a))[0], struct.unpack("<i", struct.pack("<f", b))[0]
    return (ia < 0) == (ib < 0) and abs(ia - ib) <= 1


def ref_score(win):
    """corr_softhdb on 32 symbols (demod_mod.c:1692-1735): float products, double sums in order, sum / sqrt(normx * 32.0), rounded to float"""
    win = np.asarray(win, np.float32)
    assert len(win) == HL
    sm, nx = 0.0, 0.0
    for v, b in zip(win, HDR):
        y = np.float32(1.0 if b else -1.0)
        sm += float(np.float32(y * v)); nx += float(np.float32(v * v))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(np.float64(sm) / np.sqrt(np.float64(nx) * 32.0))


def ring_at(s, hdr_bits, at, softinv=False):
    """the reference's ring when `at` symbols have been read: the last 32 seen while searching — the stream without the frame bodies behind hdr_bits — oldest
    first, zeros where the stream has not filled it"""
    s = np.asarray(s, np.float32) * np.float32(-1.0 if softinv else 1.0)
    keep = np.ones(len(s), bool)
    for hb in hdr_bits:
        keep[hb:hb + NSYM] = False
    keep[at:] = False
    seq = np.concatenate([np.zeros(HL, np.float32), s[keep]])
    return seq[-HL:]


_arb = {}


def host_frames(H, s, softinv=False, cache=None):
    """the arbiter: [(hdr_bit, bytes131, crcval, crcdat, crc_ok, `-r` line)] of the host tier over the whole stream, a symbol at a time"""
    if cache is not None and cache in _arb:
        return _arb[cache]
    s = np.ascontiguousarray(s, np.float32)
    h = host_dec(H, raw=1)
    out, buf = [], C.create_string_buffer(2048)
    base = s.ctypes.data
    sg = s * np.float32(-1.0 if softinv else 1.0)
    for i in range(len(s)):
        n = H.sonde_mts01_dec_push_soft(h, base + 4 * i, 1, int(softinv), 0, buf, 2048)
        assert n >= 0
        if n:
            line = buf.raw[:n].decode().rstrip("\n")
            hb = i + 1 - NSYM
            by, val, dat, ok, mline = model_frame(sg[hb:hb + NSYM])
            assert mline == line, (hb, mline, line)                           # the model is the arbiter's, frame by frame
            out.append((hb, by, val, dat, ok, line))
    H.sonde_mts01_dec_destroy(h)
    if cache is not None:
        _arb[cache] = out
    return out


def host_text(H, s, softinv=False, **kw):
    """what the host tier prints for the whole stream under the options kw"""
    s = np.ascontiguousarray(s, np.float32)
    h = host_dec(H, **kw)
    buf = C.create_string_buffer(1 << 20)
    n = H.sonde_mts01_dec_push_soft(h, s.ctypes.data, len(s), int(softinv), 0, buf, len(buf))
    assert n >= 0
    H.sonde_mts01_dec_destroy(h)
    return buf.raw[:n].decode("latin-1")                      # (a frame that failed its CRC prints whatever bytes it holds: a character per byte)


def emu_frames(E, s, calls, softinv=False, cap=64):
    """the emulated consumer over the stream cut into calls (the last length repeats): Recs, frames dropped for want of room, end state"""
    s = np.ascontiguousarray(s, np.float32)
    buf = (Rec * (len(s) // NSYM + 2))()
    cl = (C.c_int * len(calls))(*calls)
    dropped, end = C.c_int(0), EmuState()
    n = E.emu_mts01_run(s.ctypes.data, len(s), cl, len(calls), int(softinv), cap, buf, len(buf), C.byref(dropped), C.byref(end))
    assert 0 <= n < len(buf), n
    for i in range(n):
        assert buf[i].channel == 0
    return [buf[i] for i in range(n)], dropped.value, end


def state(end):
    """the end state as far as it means anything: the bits so far and the frame position only inside a frame"""
    inside = end.mode == 1
    words = [int(end.w[k]) & (0xFFFFFFFF if 32 * k + 32 <= end.done else (1 << max(end.done - 32 * k, 0)) - 1) for k in range(33)]
    return (end.mode, end.bits_in, [struct.pack("<f", v) for v in end.hist], (end.done, words, end.hdr_bit, struct.pack("<f", end.mv)) if inside else None)


# ---------------------------------------------------------------- frames and streams
def frame_of(dat128, byte0=0x80, crc=None):
    """the 1048 bits of byte0, 128 data bytes and their CRC (low byte first)"""
    dat = bytes(dat128)
    assert len(dat) == 128
    re = crc16_re(dat) if crc is None else crc
    return np.unpackbits(np.frombuffer(bytes([byte0]) + dat + bytes([re & 0xFF, re >> 8]), np.uint8))


def fbits(k):
    return synth.mts01_frame_bits(k)


def onair(frames, lead=40, gap=152 - 32):
    """header and frame, one after the other, behind `lead` idle symbols 1010 .. and with `gap` of them between two frames"""
    parts = []
    for k, fb in enumerate(frames):
        n = gap if k else lead
        parts += [np.tile(np.array([1, 0], np.uint8), (n + 1) // 2)[:n], HDR, np.asarray(fb, np.uint8)]
    return np.concatenate(parts)


def soft(sym, rng=None, jitter=(1.0, 1.0)):
    s = 2.0 * np.asarray(sym, np.float64) - 1.0
    if rng is not None:
        s = s * rng.uniform(jitter[0], jitter[1], len(s))
    return s.astype(np.float32)


def noise(rng, n, sigma=0.3):
    return rng.normal(0.0, sigma, n).astype(np.float32)


# the stream cases and their options (softinv = --softinv).  Kept apart from the streams, which need the host library to be built: a test module must not load
# libsonde_hip.so while it is collected (tests/conftest.py: PyTorch's HIP runtime has to come first in a GPU process).
STREAM_OPTS = {"clean": {}, "sigma03": {}, "inverted": {}, "inverted_softinv": dict(softinv=True), "edge_under": {}, "edge_exact": {}, "edge_above": {},
               "back_to_back": {}, "no_nul": {}, "early_nul": {}, "byte0_changed": {}, "zero_symbols": {}, "zero_window": {}, "ring_behind_frame": {}}


def case_opts():
    """name -> softinv of every case, without building a stream"""
    return {k: v.get("softinv", False) for k, v in STREAM_OPTS.items()}


FLIP3 = np.array([4, 13, 27])
EDGE_LEAD = 16


def _edge_stream(a, t):
    """(the header's window is s[EDGE_LEAD:EDGE_LEAD + 32]; header symbol 0 is a 1)"""
    s = soft(onair([fbits(6)], lead=EDGE_LEAD))
    s[EDGE_LEAD + FLIP3] = -s[EDGE_LEAD + FLIP3]
    s[EDGE_LEAD] = np.float32(a)
    return np.concatenate([s, t])


def _find_edge(H, t):
    """amplitudes of header symbol 0 of a header with three flipped symbols.  The score (25 + a) / sqrt(32 (31 + a^2)) rises with a on [-1, 1] from 24 / 32 to
    26 / 32.  -> (under, exact, above): above is the smallest float at which the host framer finds the header, exact the float below it (the score there rounds
    to 0.8f itself), under the largest at which the score is below 0.8f"""
    def found(a):
        s = np.ascontiguousarray(_edge_stream(a, t), np.float32)
        h = host_dec(H, raw=1)
        buf = C.create_string_buffer(4096)
        n = H.sonde_mts01_dec_push_soft(h, s.ctypes.data, len(s), 0, 0, buf, 4096)
        H.sonde_mts01_dec_destroy(h)
        return n > 0
    lo, hi = np.float32(-1.0), np.float32(1.0)
    assert not found(lo) and found(hi)
    while np.nextafter(lo, np.float32(2.0)) < hi:
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        if found(mid):
            hi = mid
        else:
            lo = mid
    under = lo
    for _ in range(4000):
        if ref_score(_edge_stream(under, t)[EDGE_LEAD:EDGE_LEAD + HL]) < F08:
            break
        under = np.nextafter(under, np.float32(-2.0))
    return under, lo, hi


def case_streams(H):
    """name -> dict(s, softinv, n = frames the arbiter must give, ok = their verdicts)"""
    c = {}
    rng = np.random.default_rng(7100)
    tail = lambda n=70: noise(rng, n, 0.05)                                        # noqa: E731
    # 1. clean frames a second apart, and at sigma 0.3
    c["clean"] = dict(s=np.concatenate([soft(onair([fbits(0), fbits(1), fbits(2)])), tail()]), n=3, ok=[1, 1, 1])
    s = np.concatenate([soft(onair([fbits(3), fbits(4), fbits(5)], lead=23)), tail()])
    c["sigma03"] = dict(s=s + noise(rng, len(s), 0.3), n=3, ok=[1, 1, 1])
    # 2. polarity: every hit counts and the bits are read raw, so the inverted stream gives inverted bits and a failing CRC; --softinv puts it right
    pol = np.concatenate([soft(onair([fbits(7), fbits(8)], lead=33), rng, (0.8, 1.2)), tail(37)])
    c["inverted"] = dict(s=-pol, n=2, ok=[0, 0])
    c["inverted_softinv"] = dict(s=-pol, softinv=True, n=2, ok=[1, 1])
    # 3. the threshold: three flipped header symbols and one symbol's amplitude moved until the host framer changes its mind
    t = tail()
    under, exact, above = _find_edge(H, t)
    for name, a in (("edge_under", under), ("edge_exact", exact), ("edge_above", above)):
        c[name] = dict(s=_edge_stream(a, t), n=int(name == "edge_above"), ok=[1] * int(name == "edge_above"), amp=float(a))
    # 4. back to back: the next header right behind a frame's last bit
    c["back_to_back"] = dict(s=np.concatenate([soft(onair([fbits(10), fbits(11), fbits(12), fbits(13)], lead=0, gap=0)), tail()]), n=4, ok=[1, 1, 1, 1])
    # 5. the text: 128 bytes without a NUL (the string runs into the CRC bytes), and a NUL among the first fields
    full_ = ("B7654321,1,77,240615120001,7300,41.000001,29.000002,2345.6,200.1,15.2,0,21.50,22.50,55,0,0," + "9" * 128)[:128].encode()
    early = np.packbits(fbits(14))[1:129].tobytes()
    early = early[:9] + b"\0" + early[10:]
    c["no_nul"] = dict(s=np.concatenate([soft(onair([frame_of(full_)])), tail()]), n=1, ok=[1])
    c["early_nul"] = dict(s=np.concatenate([soft(onair([frame_of(early)])), tail()]), n=1, ok=[1])
    # 6. byte 0 is not under the CRC
    c["byte0_changed"] = dict(s=np.concatenate([soft(onair([frame_of(np.packbits(fbits(15))[1:129].tobytes(), byte0=0x3C)])), tail()]), n=1, ok=[1])
    # 7. exact zeros and -0.0 on frame symbols: s >= 0 is true for both
    s = soft(onair([fbits(16)], lead=50), rng, (0.8, 1.2))
    for n_, p in enumerate(range(50 + HL + 5, len(s), 23)):
        s[p] = np.float32(0.0) if n_ % 2 == 0 else np.float32(-0.0)
    c["zero_symbols"] = dict(s=np.concatenate([s, tail()]), n=1, ok=[0])
    # 8. windows of exact zeros: 0 / 0 is no hit
    c["zero_window"] = dict(s=np.concatenate([np.zeros(53, np.float32), soft(onair([fbits(17)], lead=8)), np.zeros(75, np.float32), soft(onair([fbits(18)], lead=8)),
                                              tail()]), n=2, ok=[1, 1])
    # 9. the ring behind a frame is the header it was found by: K symbols y right behind the frame complete h1[K:] ++ y to a hit, where h1 is a header that is
    #    nearly silent wherever it disagrees with itself K symbols on — built by search with the arbiter over K (smallest first) so that the frame's own last
    #    symbols in the ring's place, or an emptied ring, give none.
    body1, body2 = soft(fbits(19)), soft(fbits(20))
    lead = soft(np.tile(np.array([1, 0], np.uint8), 6))
    for K in range(1, HL):
        h1 = soft(HDR)
        h1[[i for i in range(K, HL) if HDR[i] != HDR[i - K]]] *= np.float32(0.001)
        base = np.concatenate([lead, h1, body1])
        y = soft(HDR[HL - K:])
        s = np.concatenate([base, y, body2, tail()])
        fed = np.concatenate([base[-(HL - K):], y])                               # what the ring would hold had the frame's symbols been fed into it
        emptied = np.concatenate([np.zeros(HL - K, np.float32), y])
        if abs(ref_score(fed)) > F08 or abs(ref_score(emptied)) > F08:
            continue
        got = host_frames(H, s)
        if len(got) == 2 and got[0][0] == 12 + HL and got[1][0] == len(base) + K:
            c["ring_behind_frame"] = dict(s=s, n=2, ok=[1, 1], K=K, at=len(base))
            break
    for k, v in c.items():
        v["softinv"] = case_opts()[k]
    assert set(c) == set(STREAM_OPTS), set(STREAM_OPTS) - set(c)
    return c


_cases = None


def cases(H=None):
    global _cases
    if _cases is None:
        _cases = case_streams(H or load_host())
    return _cases


def long_stream():
    """twelve frames at sigma 0.3 in a call longer than the staging buffer"""
    rng = np.random.default_rng(7112)
    s = np.concatenate([soft(onair([fbits(k) for k in range(20, 32)], lead=9, gap=40)), np.zeros(60, np.float32)])
    return s + noise(rng, len(s), 0.3)


def cap_stream(nframes=5):
    """frames back to back for one channel"""
    return soft(onair([fbits(40 + k) for k in range(nframes)], lead=0, gap=0))


def random_cuts(n, seed, lo=1, hi=2700):
    rng = np.random.default_rng(seed)
    out, tot = [], 0
    while tot < n:
        k = int(rng.integers(lo, hi))
        out.append(k); tot += k
    return out
