"""Streams and arbiters shared by tests/test_softin_mrz_emu.py (the device MRZ soft-bit consumer under the CPU wave emulator), tests/test_mrz_decoded.py and
tests/test_gpu_softin_mrz.py (the same source as k_softin_mrz on the device): half-symbol streams built from tools/synth.py frames, the host tier
sonde_mrz_dec_push_soft (pinned to the compiled reference by the family suites) as arbiter, and the emulator driver tests/emu/softin_mrz_emu.cpp.

The arbiter prints text only.  Fed a half symbol at a time it prints a frame at the frame's last half symbol; the frame length in effect for that frame is what
sonde_mrz_dec_frame_bits said before the push, so the header matched 2 (nbits - 22) half symbols before that.  The bits the records are compared with come from
model_frame(): the Manchester rule on those half symbols under the polarity the hit's score implies, the bytes from bit --ofs on, the frame type and a CRC-16
computed here; host_frames() asserts for every frame that the line made from the model IS the arbiter's line (`-r`: bytes and verdict; `-R`: the bits).  The
arbiter does not print mv: the expected score is ref_score() — the reference's expression (float products, double sums in order, sum / sqrt(normx * 44), rounded
to float) on the 44 half symbols the reference's ring holds at the hit, i.e. the last 44 of the stream with the frame bodies the arbiter found taken out (ring_at).

One thing the reference does that a reader may not expect: once a lat / lon frame has passed its CRC the frame length is 384 bits, and an ECEF frame cut at 384
bits has its last three bytes and its CRC word read as zero — it cannot pass, so the reference stays at 384 for good on real ECEF frames.  The way back to 408 is a
frame that passes as an ECEF frame AT 384 bits: bytes 3 .. 44 followed by their own CRC and a zero byte leave the register at zero (crafted_frame()).  The
reference PROGRAM ends right there (mp3h1mod.c:1238 takes a frame shorter than the new length for the end of input); the host tier, and the consumer, which have
no end of input, read on with 408 bits.  The case says so with ref_n: the compiled reference prints that many of the case's frames."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from tools import synth
from radiosonde_auto_rx_amd.family import MrzOpts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_SRC = os.path.join(EMU_DIR, "softin_mrz_emu.cpp")
EMU_SO = os.path.join(EMU_DIR, "libsoftin_mrz_emu.so")
DEPS = [EMU_SRC, os.path.join(EMU_DIR, "wave_emu.h"), os.path.join(CSRC, "sonde_softin_mrz_dev.h"), os.path.join(CSRC, "sonde_softin_wave_dev.h"),
        os.path.join(CSRC, "sonde_rs_dev.h"), os.path.join(ROOT, "include", "sonde_hip.h")]
REF = os.path.join(ROOT, "oracle", "_ref", "mp3h1mod")
HEADER = "1001" * 9 + "10101010"                             # the 44 header half symbols `mp3h1mod` searches for: AA AA and 101111 in Manchester
HDR = np.array([int(c) for c in HEADER], np.uint8)
HDR22 = [1, 0] * 9 + [1, 1, 1, 1]
HL = 44
LEN_ECEF, LEN_LATLON = 408, 384
STAGE_MAX = 12288                                           # M10_STAGE_MAX of sonde_softin_wave_dev.h
CUTS = [2400, 1000, 251, 1, 2, 43, 44, 45, 63, 64, 65]
F082 = np.float32(0.82)


class Rec(C.Structure):
    """SoftinMrzRec (csrc/sonde_softin_mrz_dev.h)"""
    _fields_ = [("channel", C.c_int32), ("mv", C.c_float), ("hdr_bit", C.c_uint64), ("nbits", C.c_int32), ("inv", C.c_uint8), ("crc_ok", C.c_uint8),
                ("crclen", C.c_uint8), ("pad", C.c_uint8), ("crcval", C.c_uint16), ("crcdat", C.c_uint16), ("bits", C.c_uint8 * 52)]


class EmuState(C.Structure):
    """EmuMrzState (tests/emu/softin_mrz_emu.cpp)"""
    _fields_ = [("mode", C.c_int), ("done", C.c_int), ("inv", C.c_int), ("bitfrm_len", C.c_int), ("mv", C.c_float), ("carry", C.c_float), ("bits_in", C.c_uint64),
                ("hdr_bit", C.c_uint64), ("hist", C.c_float * 44), ("w", C.c_uint32 * 13), ("pad", C.c_int)]


def load_emu(src=EMU_SRC, so=EMU_SO, deps=DEPS, flags=()):
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = so + ".%d.tmp" % os.getpid()
        # (-ffp-contract=off: the score is the reference's expression, every product and sum rounded on its own)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", *flags, "-o", tmp, src])
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.emu_mrz_run.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int] + [C.c_int] * 6 + [C.POINTER(Rec), C.c_int, C.POINTER(C.c_int), C.POINTER(EmuState)]
    L.emu_mrz_crc.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    L.emu_mrz_header_mask.restype = C.c_uint64
    return L


def load_host():
    from radiosonde_auto_rx_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    L = C.CDLL(engine.LIB_PATH)
    L.sonde_mrz_dec_create.argtypes = [C.POINTER(MrzOpts), C.POINTER(C.c_void_p)]
    L.sonde_mrz_dec_destroy.argtypes = [C.c_void_p]
    L.sonde_mrz_dec_frame_bits.argtypes = [C.c_void_p]
    L.sonde_mrz_dec_push_soft.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]
    L.sonde_mrz_dec_decoded.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]
    return L


def host_dec(H, **kw):
    h = C.c_void_p()
    if isinstance(kw.get("version"), str):
        kw["version"] = kw["version"].encode()
    o = MrzOpts(**kw)
    assert H.sonde_mrz_dec_create(C.byref(o), C.byref(h)) == 0
    return h


def dec_opts(c, **kw):
    """a case's options as fields of MrzOpts: -r (or -R), -i, --auto, --ofs"""
    o = dict(raw=2 if c["raw2"] else 1, inv=int(c["inv"]), aut=int(c["aut"]))
    if c["ofs"] is not None:
        o.update(bits_ofs=c["ofs"], bits_ofs_given=1)
    o.update(kw)
    return o


# ---------------------------------------------------------------- the model of a frame
def crc16rev(data):
    rem = 0xFFFF
    for b in bytes(data):
        rem ^= b
        for _ in range(8):
            rem = (rem >> 1) ^ 0xA001 if rem & 1 else rem >> 1
    return rem


def verdict(frame51):
    """(crclen, crcval, crcdat, crc_ok) of 51 frame bytes: the frame type from bytes 30 / 31, CRC over crclen bytes from byte 3 against the word behind them"""
    f = bytes(frame51)
    crclen = 42 if f[30:32] == b"\xff\xff" else 45
    val, dat = crc16rev(f[3:3 + crclen]), f[crclen + 3] | f[crclen + 4] << 8
    return crclen, val, dat, int(val == dat)


def frame_bytes(bits, nbits, ofs):
    """bits2bytes from bit ofs on: (nbits - ofs) // 8 bytes MSB first, zeros up to 51"""
    frmlen = (nbits - ofs) // 8
    b = bytes(np.packbits(np.asarray(bits[ofs:ofs + 8 * frmlen], np.uint8)))
    return b + bytes(51 - len(b)), frmlen


def manchester(sym, inv):
    """bit j from half symbols 2 j, 2 j + 1: s = s2 - s1 in float, (s >= 0), inverted unless inv"""
    sym = np.asarray(sym, np.float32)
    s = (sym[1::2] - sym[0::2]).astype(np.float32)
    return ((s >= 0).astype(np.uint8) ^ (0 if inv else 1)).astype(np.uint8)


def pack(bits):
    b = np.zeros(416, np.uint8)
    b[:len(bits)] = bits
    return bytes(np.packbits(b))


def model_frame(sym, nbits, inv, ofs, raw2):
    """(bits52, crc_ok, crclen, the `-r` / `-R` line) of the 2 (nbits - 22) half symbols behind a hit"""
    bits = HDR22 + [int(b) for b in manchester(sym, inv)]
    assert len(bits) == nbits
    if raw2:
        return pack(bits), 0, 0, "".join(str(b) for b in bits)
    fr, frmlen = frame_bytes(bits, nbits, ofs)
    crclen, _, _, ok = verdict(fr)
    return pack(bits), ok, crclen, "".join("%02X " % v for v in fr[:frmlen]) + " " + ("[OK]" if ok else "[NO]")


def _g(r):
    return (lambda k: r[k]) if isinstance(r, dict) else (lambda k: getattr(r, k))


def raw_line(r, ofs=None, raw2=False):
    """the `-r` (`-R`) line of a record (a Rec or a fetch_mrz dict) from its bits and ITS verdict"""
    g = _g(r)
    bits = np.unpackbits(np.frombuffer(bytes(g("bits")), np.uint8))[:g("nbits")]
    if raw2:
        return "".join(str(int(b)) for b in bits)
    fr, frmlen = frame_bytes(bits, g("nbits"), 8 if ofs is None else ofs)
    return "".join("%02X " % v for v in fr[:frmlen]) + " " + ("[OK]" if g("crc_ok") else "[NO]")


def key(r):
    """(hdr_bit, nbits, inv, the bits, crc_ok, crclen) of a Rec, a fetch_mrz dict or an arbiter tuple: what must agree exactly with the arbiter"""
    if isinstance(r, tuple):
        return r[:6]
    g = _g(r)
    return (g("hdr_bit"), g("nbits"), g("inv"), bytes(g("bits")), g("crc_ok"), g("crclen"))


def full(r):
    """everything of a Rec the emulator must reproduce under any cut, mv bit for bit"""
    return key(r) + (struct.pack("<f", r.mv), r.crcval, r.crcdat)


def mv_within_one_ulp(a, b):
    """two floats (the device's double divide and sqrt come ahead of the rounding to float: one ulp, as the other device suites allow)"""
    ia, ib = struct.unpack("<i", struct.pack("<f", a))[0], struct.unpack("<i", struct.pack("<f", b))[0]
    return (ia < 0) == (ib < 0) and abs(ia - ib) <= 1


def ref_score(win):
    """corr_softhdb on 44 half symbols (demod_mod.c:1692-1735): float products, double sums in order, sum / sqrt(normx * 44.0), rounded to float"""
    win = np.asarray(win, np.float32)
    assert len(win) == HL
    sm, nx = 0.0, 0.0
    for v, b in zip(win, HDR):
        y = np.float32(1.0 if b else -1.0)
        sm += float(np.float32(y * v)); nx += float(np.float32(v * v))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(np.float64(sm) / np.sqrt(np.float64(nx) * 44.0))


def ring_at(s, frames, at, softinv=False):
    """the reference's ring when `at` half symbols have been read: the last 44 seen while searching — the stream without the frame bodies behind the arbiter's
    (hdr_bit, nbits, ..) — oldest first, zeros where the stream has not filled it"""
    s = np.asarray(s, np.float32) * np.float32(-1.0 if softinv else 1.0)
    keep = np.ones(len(s), bool)
    for f in frames:
        keep[f[0]:f[0] + 2 * (f[1] - 22)] = False
    keep[at:] = False
    seq = np.concatenate([np.zeros(HL, np.float32), s[keep]])
    return seq[-HL:]


_arb = {}


def host_frames(H, s, softinv=False, inv=0, aut=0, raw2=False, ofs=None, cache=None, **_):
    """the arbiter: [(hdr_bit, nbits, inv, bits52, crc_ok, crclen, line)] of the host tier over the whole stream, a half symbol at a time"""
    if cache is not None and cache in _arb:
        return _arb[cache]
    s = np.ascontiguousarray(s, np.float32)
    h = host_dec(H, **dec_opts(dict(raw2=raw2, inv=inv, aut=aut, ofs=ofs)))
    out, buf = [], C.create_string_buffer(2048)
    base = s.ctypes.data
    sg = s * np.float32(-1.0 if softinv else 1.0)
    for i in range(len(s)):
        nbits = H.sonde_mrz_dec_frame_bits(h) + 22                           # the length in effect for a frame that ends with this half symbol
        n = H.sonde_mrz_dec_push_soft(h, base + 4 * i, 1, int(softinv), 0, buf, 2048)
        assert n >= 0
        if n:
            line = buf.raw[:n].decode().rstrip("\n")
            hb = i + 1 - 2 * (nbits - 22)
            pol = int(ref_score(ring_at(s, out, hb, softinv)) < 0)            # an accepted hit has the sign of the polarity in effect
            bits, ok, crclen, mline = model_frame(sg[hb:hb + 2 * (nbits - 22)], nbits, pol, 8 if ofs is None else ofs, raw2)
            assert mline == line, (hb, mline, line)                           # the model is the arbiter's, frame by frame
            out.append((hb, nbits, pol, bits, ok, crclen, line))
    H.sonde_mrz_dec_destroy(h)
    if cache is not None:
        _arb[cache] = out
    return out


def host_text(H, s, softinv=False, **kw):
    """what the host tier prints for the whole stream under the options kw"""
    s = np.ascontiguousarray(s, np.float32)
    h = host_dec(H, **kw)
    buf = C.create_string_buffer(1 << 20)
    n = H.sonde_mrz_dec_push_soft(h, s.ctypes.data, len(s), int(softinv), 0, buf, len(buf))
    assert n >= 0
    H.sonde_mrz_dec_destroy(h)
    return buf.raw[:n].decode()


def emu_frames(E, s, calls, softinv=False, inv=0, aut=0, raw2=False, ofs=None, cap=64, **_):
    """the emulated consumer over the stream cut into calls (the last length repeats): Recs, frames dropped for want of room, end state"""
    s = np.ascontiguousarray(s, np.float32)
    buf = (Rec * (len(s) // 700 + 2))()
    cl = (C.c_int * len(calls))(*calls)
    dropped, end = C.c_int(0), EmuState()
    n = E.emu_mrz_run(s.ctypes.data, len(s), cl, len(calls), int(softinv), int(inv), int(aut), int(raw2), 8 if ofs is None else ofs, cap, buf, len(buf),
                      C.byref(dropped), C.byref(end))
    assert 0 <= n < len(buf), n
    for i in range(n):
        assert buf[i].channel == 0
    return [buf[i] for i in range(n)], dropped.value, end


def state(end):
    """the end state as far as it means anything: polarity and frame length always; the pending half symbol, the bits so far and the position only inside a frame"""
    inside = end.mode == 1
    nb = 22 + end.done // 2
    words = [int(end.w[k]) & (0xFFFFFFFF if 32 * k + 32 <= nb else (1 << max(nb - 32 * k, 0)) - 1) for k in range(13)]
    return (end.mode, end.inv, end.bitfrm_len, end.bits_in, [struct.pack("<f", v) for v in end.hist],
            (end.done, struct.pack("<f", end.carry) if end.done & 1 else None, words, end.hdr_bit, struct.pack("<f", end.mv)) if inside else None)


# ---------------------------------------------------------------- frames and streams
def fsym(fr):
    """the half symbols (0 / 1) of AA + the frame bytes, MSB first, in Manchester (1 -> 10, 0 -> 01): 816 for an ECEF frame, 768 for a lat / lon one"""
    bits = np.unpackbits(np.frombuffer(bytes([0xAA]) + bytes(fr), np.uint8))
    return np.stack([bits, 1 - bits], 1).reshape(-1).astype(np.uint8)


def ecef(k):
    return synth.mrz_frame(k)


def latlon(k):
    return synth.mrz_frame(k, latlon=True)


def crafted_frame(k):
    """47 bytes that pass as an ECEF frame when read at 384 bits: bytes 3 .. 44 of an ECEF frame, their CRC at 45 / 46 — the zero byte the cut leaves at 47 keeps
    the register at zero, and the CRC word read behind it is zero as well"""
    f = bytearray(synth.mrz_frame(k)[:47])
    f[45:47] = crc16rev(f[3:45]).to_bytes(2, "little")
    assert verdict(bytes(f) + bytes(4)) == (45, 0, 0, 1)
    return bytes(f)


def soft(sym, rng=None, jitter=(1.0, 1.0)):
    s = 2.0 * np.asarray(sym, np.float64) - 1.0
    if rng is not None:
        s = s * rng.uniform(jitter[0], jitter[1], len(s))
    return s.astype(np.float32)


def noise(rng, n, sigma=0.3):
    return rng.normal(0.0, sigma, n).astype(np.float32)


def idle(rng, n):
    """n idle half symbols at full amplitude: 0101 .. (zero bits), the last four 0110.  The header's 1001 1001 .. repeats every four half symbols, so next to
    silence, or next to idle symbols that happen to continue it, the reference finds a header four half symbols early — or four late, on the ring a frame left —
    (two flipped and four silent half symbols still score 0.95) and reads a frame two bits off; 0101 behind a frame and 0110 in front of one make those windows
    miss by six.  (rng: not used, the pattern is fixed)"""
    sym = np.tile(np.array([0, 1], np.uint8), (n + 1) // 2)[:n]
    if n >= 4:
        sym[-4:] = (0, 1, 1, 0)
    return soft(sym)


def train(rng, frames, lead=33, gap=60, end=70, jitter=None):
    """frames with an idle gap in front of each (a lat / lon frame read at 408 bits takes 48 half symbols of what follows it) and a quiet tail in which no header
    is found"""
    parts = []
    for k, fr in enumerate(frames):
        parts += [idle(rng, gap if k else lead), soft(fsym(fr), rng if jitter else None, jitter or (1.0, 1.0))]
    if end:
        parts.append(idle(rng, end))
    return np.concatenate(parts)


# the stream cases and their options.  Kept apart from the streams, which need the host library to be built: a test module must not load libsonde_hip.so while it
# is collected (tests/conftest.py: PyTorch's HIP runtime has to come first in a GPU process), so the modules parametrise over case_opts() and build cases()
# inside their tests.
_D = dict(softinv=False, inv=0, aut=0, raw2=False, ofs=None)
STREAM_OPTS = {"clean_ecef": {}, "clean_latlon": {}, "switch": {}, "switch_back": {}, "ffff_bad_crc": {}, "raw2_never_switches": dict(raw2=True), "ofs_0": dict(ofs=0),
               "ofs_9": dict(ofs=9), "ofs_64": dict(ofs=64), "inverted_plain": {}, "inverted_i": dict(inv=1), "inverted_softinv": dict(softinv=True),
               "inverted_auto": dict(aut=1), "dropped_then_true": {}, "edge_under": {}, "edge_exact": {}, "edge_above": {}, "zero_window": {}, "equal_halves": {},
               "equal_halves_inv": dict(inv=1), "ring_behind_frame": {}, "sigma03": {}}


def case_opts():
    """name -> options of every case, without building a stream"""
    return {k: dict(_D, **v) for k, v in STREAM_OPTS.items()}


FLIP3 = np.array([5, 18, 31])


EDGE_LEAD = 16


def _edge_stream(a, t):
    """(the header's window is s[EDGE_LEAD:EDGE_LEAD + 44])"""
    s = soft(fsym(ecef(6)))
    s[FLIP3] = -s[FLIP3]
    s[0] = np.float32(a)
    return np.concatenate([idle(np.random.default_rng(16), EDGE_LEAD), s, t])


def _find_edge(H, t):
    """amplitudes of header half symbol 0 (a 1: +1 at unit amplitude) of a header with three flipped half symbols.  The score (37 + a) / sqrt(44 (43 + a^2)) rises
    with a on [-1, 0] from 36 / 44 = 0.818 to 0.85.  -> (under, exact, above): above is the smallest float at which the host framer finds the header, exact the
    float below it (the score there rounds to 0.82f itself: a float step of a moves the score by 2e-9), under the largest at which the score is below 0.82f"""
    def found(a):
        s = np.ascontiguousarray(_edge_stream(a, t), np.float32)
        h = host_dec(H, raw=1)
        buf = C.create_string_buffer(4096)
        n = H.sonde_mrz_dec_push_soft(h, s.ctypes.data, len(s), 0, 0, buf, 4096)
        H.sonde_mrz_dec_destroy(h)
        return n > 0
    lo, hi = np.float32(-1.0), np.float32(0.0)
    assert not found(lo) and found(hi)
    while np.nextafter(lo, np.float32(2.0)) < hi:
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        if found(mid):
            hi = mid
        else:
            lo = mid
    under = lo
    for _ in range(4000):
        if ref_score(_edge_stream(under, t)[EDGE_LEAD:EDGE_LEAD + HL]) < F082:
            break
        under = np.nextafter(under, np.float32(-2.0))
    return under, lo, hi


def case_streams(H):
    """name -> dict(s, options, n = frames the arbiter must give)"""
    c = {}
    rng = np.random.default_rng(3100)
    tail = lambda n=70: idle(rng, n)                                               # noqa: E731
    # 1. clean frames of both types; lat / lon: the first is read at 408 bits, passes, and the ones behind it are read at 384
    c["clean_ecef"] = dict(s=train(rng, [ecef(0), ecef(1), ecef(2)]), n=3, nbits=[408, 408, 408], ok=[1, 1, 1])
    c["clean_latlon"] = dict(s=train(rng, [latlon(3), latlon(4), latlon(5)], lead=21), n=3, nbits=[408, 384, 384], ok=[1, 1, 1])
    # 2. the length of the next frame follows the verdict: ECEF, lat / lon (read at 408, good: 384 from here on), an ECEF frame read at 384 bits (cannot pass) and
    #    another; and with a frame that passes as ECEF at 384 bits in their place the one behind it is read at 408 again
    c["switch"] = dict(s=train(rng, [ecef(7), latlon(8), ecef(9), ecef(10)], lead=17), n=4, nbits=[408, 408, 384, 384], ok=[1, 1, 0, 0])
    c["switch_back"] = dict(s=train(rng, [ecef(7), latlon(8), crafted_frame(9), ecef(10), latlon(11)], lead=29), n=5, nbits=[408, 408, 384, 408, 408], ok=[1, 1, 1, 1, 1], ref_n=3)
    # 3. FF FF at 30 / 31 and a bad CRC: no switch, the ECEF frame behind it is read at 408 and passes
    bad = bytearray(latlon(12)); bad[16] ^= 0x10
    c["ffff_bad_crc"] = dict(s=train(rng, [bytes(bad), ecef(13)], lead=40), n=2, nbits=[408, 408], ok=[0, 1])
    # 4. -R: the reference never looks at the bytes, so the length stays 408 for ever
    c["raw2_never_switches"] = dict(s=train(rng, [ecef(14), latlon(15), ecef(16)]), n=3, nbits=[408, 408, 408], ok=[0, 0, 0])
    # 5. --ofs: the bytes start elsewhere (0: the preamble byte first; 9: a bit late; 64: 43 bytes, the CRC word beyond them)
    for ofs in (0, 9, 64):
        c["ofs_%d" % ofs] = dict(s=c["clean_ecef"]["s"], n=3, nbits=[408, 408, 408], ok=[0, 0, 0])
    # 6. polarity: the inverted stream as it is (every hit dropped), with -i, with --softinv, and with --auto (flips at the first hit and stays flipped)
    pol = train(rng, [ecef(17), ecef(18)], jitter=(0.8, 1.2))
    c["inverted_plain"] = dict(s=-pol, n=0, nbits=[], ok=[])
    for name in ("inverted_i", "inverted_softinv", "inverted_auto"):
        c[name] = dict(s=-pol, n=2, nbits=[408, 408], ok=[1, 1])
    # 7. a hit of the wrong polarity is dropped and the ring goes on: the true header begins four half symbols BEFORE the dropped hit, inside its window — its
    #    first four half symbols, at amplitude 1.5, stand in for the inverted header's last four (two agree, two do not: 40 / sqrt(44 * 49) = 0.861 the wrong way
    #    round).  Three more of its half symbols are flipped, so that with them it scores 40 / sqrt(44 * 49) = 0.861 and without them — a ring emptied or stopped
    #    at the dropped hit — 34 / sqrt(44 * 40) = 0.810.  Both hits lie in the same round of 64 positions of a single call; the idle symbols in front are inverted
    #    too, so that no window before the dropped hit scores.
    t_hdr = soft(HDR)
    t_hdr[:4] *= np.float32(1.5)
    t_hdr[[10, 21, 33]] *= np.float32(-1.0)
    c["dropped_then_true"] = dict(s=np.concatenate([-idle(rng, 30), -soft(HDR)[:40], t_hdr, soft(fsym(ecef(19)))[HL:], tail()]), n=1, nbits=[408], ok=[1], at=30 + HL,
                                  true_at=30 + 40 + HL)
    # 8. the threshold: three flipped header half symbols and one half symbol's amplitude moved until the host framer changes its mind
    t = tail()
    under, exact, above = _find_edge(H, t)
    for name, a in (("edge_under", under), ("edge_exact", exact), ("edge_above", above)):
        c[name] = dict(s=_edge_stream(a, t), n=int(name == "edge_above"), nbits=[408] * int(name == "edge_above"), ok=[1] * int(name == "edge_above"), amp=float(a))
    # 9. windows of exact zeros: 0 / 0 is no hit
    c["zero_window"] = dict(s=np.concatenate([np.zeros(53, np.float32), idle(rng, 8), soft(fsym(ecef(20))), idle(rng, 8), np.zeros(75, np.float32), idle(rng, 8), soft(fsym(ecef(21))), tail()]), n=2,
                            nbits=[408, 408], ok=[1, 1])
    # 10. bits with equal halves (s = +0: a 1 before the polarity step) and with s1 = +0, s2 = -0 (s = -0, which is >= 0 as well), in both polarities
    s = soft(fsym(ecef(22)), rng, (0.8, 1.2))
    for n_, p in enumerate(range(HL + 6, len(s) - 1, 22)):
        s[p:p + 2] = (np.float32(0.37), np.float32(0.37)) if n_ % 2 == 0 else (np.float32(0.0), np.float32(-0.0))
    c["equal_halves"] = dict(s=np.concatenate([idle(rng, 50), s, tail()]), n=1, nbits=[408], ok=[0])
    si = -c["equal_halves"]["s"]
    for n_, p in enumerate(range(HL + 6, len(s) - 1, 22)):
        if n_ % 2:
            si[50 + p:50 + p + 2] = (np.float32(0.0), np.float32(-0.0))
    c["equal_halves_inv"] = dict(s=si, n=1, nbits=[408], ok=[0])
    # 11. the ring behind a frame is the header it was found by: K half symbols y right behind the frame complete h1[K:] ++ y to a hit, where h1 is a header that is
    #     nearly silent wherever it disagrees with itself K half symbols on — built by search with the arbiter over K (smallest first) so that the frame's own last
    #     half symbols in the ring's place, or an emptied ring, give none.
    body1, body2 = soft(fsym(ecef(23)))[HL:], soft(fsym(ecef(24)))[HL:]
    for K in range(1, HL):
        h1 = soft(HDR)
        h1[[i for i in range(K, HL) if HDR[i] != HDR[i - K]]] *= np.float32(0.001)
        base = np.concatenate([idle(np.random.default_rng(12), 12), h1, body1])
        y = soft(HDR[HL - K:])
        s = np.concatenate([base, y, body2, tail()])
        fed = np.concatenate([base[-(HL - K):], y])                               # what the ring would hold had the frame's half symbols been fed into it
        emptied = np.concatenate([np.zeros(HL - K, np.float32), y])
        if abs(ref_score(fed)) > F082 or abs(ref_score(emptied)) > F082:
            continue
        got = host_frames(H, s)
        if len(got) == 2 and got[0][0] == 12 + HL and got[1][0] == len(base) + K:
            c["ring_behind_frame"] = dict(s=s, n=2, nbits=[408, 408], ok=[1, 1], K=K, at=len(base))
            break
    # 12. noise
    s = train(rng, [ecef(25), latlon(26), latlon(27)], lead=17, jitter=(0.9, 1.1))
    c["sigma03"] = dict(s=s + noise(rng, len(s), 0.3), n=3, nbits=[408, 408, 384], ok=[1, 1, 1])
    for k, v in c.items():
        for o, d in case_opts()[k].items():
            v[o] = d
    assert set(c) == set(STREAM_OPTS), set(STREAM_OPTS) - set(c)
    return c


def opts(c):
    return {k: c[k] for k in _D}


_cases = None


def cases(H=None):
    global _cases
    if _cases is None:
        _cases = case_streams(H or load_host())
    return _cases


def stream_names():
    return sorted(STREAM_OPTS)


def long_stream():
    """sixteen frames at sigma 0.3 in a call longer than the staging buffer: ECEF, then lat / lon from the fifth on"""
    rng = np.random.default_rng(3116)
    s = train(rng, [ecef(k) for k in range(4)] + [latlon(k) for k in range(4, 16)], lead=9)
    return s + noise(rng, len(s), 0.3)


def cap_streams():
    """(first call, second call): five frames — ECEF, ECEF, lat / lon (read at 408: the switch), lat / lon, lat / lon — then one more lat / lon frame, which is
    read at 384 bits only if the switch happened behind the frames a capacity of two drops"""
    rng = np.random.default_rng(3105)
    first = train(rng, [ecef(30), ecef(31), latlon(32), latlon(33), latlon(34)], lead=11, end=0)
    second = train(rng, [latlon(35)], lead=60)
    return first, second


def random_cuts(n, seed, lo=1, hi=2700):
    rng = np.random.default_rng(seed)
    out, tot = [], 0
    while tot < n:
        k = int(rng.integers(lo, hi))
        out.append(k); tot += k
    return out
