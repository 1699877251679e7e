"""Streams and arbiters shared by tests/test_softin_rs92_emu.py (the device RS92 soft-bit consumer under the CPU wave emulator) and tests/test_gpu_softin_rs92.py (the
same source as k_softin_rs92 on the device): symbol streams built from tools/synth_rs92.py frames, the host tier sonde_rs92_dec_push_soft (pinned to the compiled
reference by tests/test_rs92_native.py / tests/test_rs92_fields.py) as arbiter, and the emulator driver tests/emu/softin_rs92_emu.cpp.

The arbiter prints text only.  With `-r -v` a frame is its 240 bytes as hex, [OK] / [NO] and (n) / (-): that gives the bytes and rs_decode's value — exactly where
it is >= 0, as "negative" where it is not (-1 / -2 / -3 print alike; the wave decoder's codes are pinned by tests/test_rs_dev_emu.py).  Fed a symbol at a time, the
arbiter prints a frame at the frame's last symbol: the header matched 4680 symbols before that.  A record is compared as key(): (ec, hdr_bit, frame bytes) exactly;
mv, which the arbiter does not print, is compared between emulator and device within one float ulp (the device's double divide and sqrt come ahead of the rounding)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from tools import synth_rs92 as R
from radiosonde_auto_rx_amd.family import Rs92Opts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_SRC = os.path.join(EMU_DIR, "softin_rs92_emu.cpp")
EMU_SO = os.path.join(EMU_DIR, "libsoftin_rs92_emu.so")
DEPS = [EMU_SRC, os.path.join(EMU_DIR, "wave_emu.h"), os.path.join(CSRC, "sonde_softin_rs92_dev.h"), os.path.join(CSRC, "sonde_softin_wave_dev.h"),
        os.path.join(CSRC, "sonde_rs_dev.h"), os.path.join(ROOT, "include", "sonde_hip.h")]
REF = os.path.join(ROOT, "oracle", "_ref", "rs92mod")
HEADER = "10100110011001101001" "1010011001100110100110101010100110101001"      # the 60 raw header symbols `rs92mod` searches for: 2A 2A 10
NSYM = 234 * 20                                             # symbols of a frame behind the header
ONAIR = 240 * 20                                            # symbols of a frame on air: 2A 2A 2A, the header, the body
STAGE_MAX = 12288                                           # M10_STAGE_MAX of sonde_softin_wave_dev.h
CUTS = [1, 19, 20, 21, 59, 60, 61, 4679, 4680, 4681, 4800]
AUTORX = dict(verbose=1, aux=1, ecc=2, gps_vel=4, json=1, ptu=1, gpsepoch=-1)       # rs92mod -vx -v --crc --ecc --vel --json --ptu (inv = -i per case)


class Rec(C.Structure):
    """SoftinRs92Rec (csrc/sonde_softin_rs92_dev.h)"""
    _fields_ = [("channel", C.c_int32), ("ec", C.c_int32), ("mv", C.c_float), ("pad", C.c_int32), ("hdr_bit", C.c_uint64), ("frame", C.c_uint8 * 240)]


class EmuState(C.Structure):
    """EmuRs92State (tests/emu/softin_rs92_emu.cpp)"""
    _fields_ = [("mode", C.c_int), ("done", C.c_int), ("carry_n", C.c_int), ("mv", C.c_float), ("bits_in", C.c_uint64), ("hdr_bit", C.c_uint64),
                ("carry", C.c_float * 20), ("hist", C.c_float * 60)]


def load_emu(src=EMU_SRC, so=EMU_SO, deps=DEPS, flags=()):
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = so + ".%d.tmp" % os.getpid()
        # (-ffp-contract=off: the score is the reference's expression, every product and sum rounded on its own)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", *flags, "-o", tmp, src])
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.emu_rs92_run.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Rec), C.c_int, C.POINTER(C.c_int), C.POINTER(EmuState)]
    L.emu_rs92_ecc.argtypes = [C.c_void_p]
    return L


def load_host():
    from radiosonde_auto_rx_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    L = C.CDLL(engine.LIB_PATH)
    L.sonde_rs92_dec_create.argtypes = [C.POINTER(Rs92Opts), C.POINTER(C.c_void_p)]
    L.sonde_rs92_dec_destroy.argtypes = [C.c_void_p]
    L.sonde_rs92_dec_load_ephemeris.argtypes = [C.c_void_p, C.c_char_p]
    L.sonde_rs92_dec_load_almanac.argtypes = [C.c_void_p, C.c_char_p]
    L.sonde_rs92_dec_push_soft.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]
    L.sonde_rs92_dec_bytes.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_char_p, C.c_size_t]
    L.sonde_rs92_dec_corrected.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_char_p, C.c_size_t]
    return L


def host_dec(H, ephemeris=None, almanac=None, **kw):
    h = C.c_void_p()
    o = Rs92Opts(**kw)
    assert H.sonde_rs92_dec_create(C.byref(o), C.byref(h)) == 0
    if ephemeris:
        assert H.sonde_rs92_dec_load_ephemeris(h, os.fsencode(ephemeris)) == 0
    if almanac:
        assert H.sonde_rs92_dec_load_almanac(h, os.fsencode(almanac)) == 0
    return h


# ---------------------------------------------------------------- records
def key(r):
    """what must agree exactly with the arbiter; r: a Rec, a dict of SoftinDev.fetch_rs92, or an arbiter tuple"""
    if isinstance(r, tuple):
        return r[:3]
    ec, hb, fr = (r["ec"], r["hdr_bit"], r["frame"]) if isinstance(r, dict) else (r.ec, r.hdr_bit, bytes(r.frame))
    return (ec if ec >= 0 else -1, hb, bytes(fr))


def full(r):
    """(ec, hdr_bit, frame, bits of mv) of a Rec or a fetch_rs92 dict: what emulator and device must share, mv within one ulp"""
    ec, hb, fr, mv = (r["ec"], r["hdr_bit"], r["frame"], r["mv"]) if isinstance(r, dict) else (r.ec, r.hdr_bit, bytes(r.frame), r.mv)
    return (ec, hb, bytes(fr), struct.pack("<f", mv))


def mv_within_one_ulp(a, b):
    ia, ib = struct.unpack("<i", a[3])[0], struct.unpack("<i", b[3])[0]
    return (ia < 0) == (ib < 0) and abs(ia - ib) <= 1


def parse_raw_line(line):
    """`-r -v` line -> (ec or -1, frame bytes)"""
    hexs, _, rest = line.partition(" ")
    fr = bytes.fromhex(hexs)
    assert len(fr) == 240 and ("[OK]" in rest or "[NO]" in rest)
    if "[NO]" in rest:
        assert "(-)" in rest
        return -1, fr
    return (int(rest.split("(")[1].split(")")[0]) if "(" in rest else 0), fr


_arb = {}


def host_frames(H, s, inv=0, softinv=False, cache=None):
    """the arbiter: [(ec, hdr_bit, frame bytes, `-r -v` line)] of the host tier over the whole stream, a symbol at a time (the frame is printed at its last symbol)"""
    if cache is not None and cache in _arb:
        return _arb[cache]
    s = np.ascontiguousarray(s, np.float32)
    h = host_dec(H, raw=1, verbose=1, inv=inv)
    out, buf = [], C.create_string_buffer(1024)
    base = s.ctypes.data
    for i in range(len(s)):
        n = H.sonde_rs92_dec_push_soft(h, base + 4 * i, 1, int(softinv), 0, buf, 1024)
        assert n >= 0
        if n:
            line = buf.raw[:n].decode().rstrip("\n")
            ec, fr = parse_raw_line(line)
            out.append((ec, i + 1 - NSYM, fr, line))
    H.sonde_rs92_dec_destroy(h)
    if cache is not None:
        _arb[cache] = out
    return out


def host_text(H, s, inv=0, softinv=False, ephemeris=None, almanac=None, **kw):
    """what the host tier prints for the whole stream under auto_rx's options (or kw)"""
    s = np.ascontiguousarray(s, np.float32)
    o = dict(AUTORX, inv=inv)
    o.update(kw)
    h = host_dec(H, ephemeris, almanac, **o)
    buf = C.create_string_buffer(1 << 20)
    n = H.sonde_rs92_dec_push_soft(h, s.ctypes.data, len(s), int(softinv), 0, buf, len(buf))
    assert n >= 0
    H.sonde_rs92_dec_destroy(h)
    return buf.raw[:n].decode()


def emu_frames(E, s, calls, inv=0, softinv=False, cap=64):
    """the emulated consumer over the stream cut into calls (the last length repeats): Recs, frames dropped for want of room, end state"""
    s = np.ascontiguousarray(s, np.float32)
    buf = (Rec * (len(s) // NSYM + 2))()
    cl = (C.c_int * len(calls))(*calls)
    dropped, end = C.c_int(0), EmuState()
    n = E.emu_rs92_run(s.ctypes.data, len(s), cl, len(calls), int(softinv), int(inv), cap, buf, len(buf), C.byref(dropped), C.byref(end))
    assert 0 <= n < len(buf), n
    for i in range(n):
        assert buf[i].channel == 0
    return [buf[i] for i in range(n)], dropped.value, end


def state(end):
    """the end state as far as it means anything: pending symbols and the frame position only inside a frame"""
    inside = end.mode == 1
    return (end.mode, end.bits_in, list(end.hist), (end.done, end.carry_n, list(end.carry)[:end.carry_n], end.hdr_bit, struct.pack("<f", end.mv)) if inside else None)


def raw_line(frame, ec):
    """the `-r -v` line of a record (rs92mod.c print_frame)"""
    return bytes(frame).hex() + " " + (" [OK]" if ec >= 0 else " [NO]") + (" (%d)" % ec if ec > 0 else " (-)" if ec < 0 else "")


# ---------------------------------------------------------------- streams
_eph = None


def ephs():
    global _eph
    if _eph is None:
        _eph = R.constellation()
    return _eph


def rinex_file(dirname):
    p = os.path.join(str(dirname), "brdc.nav")
    if not os.path.exists(p):
        open(p, "wb").write(R.rinex_nav(ephs(), extra_toe=(-7200.0,)))
    return p


_frames = {}


def frames(n=24, frame0=2000):
    if (n, frame0) not in _frames:
        _frames[(n, frame0)] = R.flight(n, ephs(), frame0=frame0)
    return _frames[(n, frame0)]


def fsym(k):
    """the 4800 on-air symbols of flight frame k"""
    return R.frame_symbols(frames()[k])


def soft(sym, rng=None, jitter=(1.0, 1.0)):
    s = 2.0 * np.asarray(sym, np.float64) - 1.0
    if rng is not None:
        s = s * rng.uniform(jitter[0], jitter[1], len(s))
    return s.astype(np.float32)


def noise(rng, n, sigma=0.3):
    return rng.normal(0.0, sigma, n).astype(np.float32)


HDR = np.array([int(c) for c in HEADER], np.uint8)


def damage(s, at, byte_idx, rng, bits=range(1, 9)):
    """swap the symbol pairs of some of the given bits (1..8: data, 0 / 9: start / stop) of the frame bytes byte_idx; `at`: where the frame's on-air symbols begin"""
    for b in byte_idx:
        pick = [int(x) for x in bits if rng.integers(0, 2)] or [int(list(bits)[0])]
        for bit in pick:
            p = at + 20 * b + 2 * bit
            s[p], s[p + 1] = s[p + 1], s[p]
    return s


def case_streams():
    """name -> dict(s, inv, softinv, n = frames the arbiter must give, ec = their values where the case names them)"""
    c = {}
    rng = np.random.default_rng(92)
    tail = lambda n=90: noise(rng, n, 0.05)                                        # noqa: E731
    # 1. clean back-to-back, unit amplitude: the window over 2A 2A 2A scores 44 / 60, which a threshold of 0.7 takes for the header 60 symbols early
    c["back_to_back"] = dict(s=np.concatenate([soft(fsym(0)), soft(fsym(1)), soft(fsym(2)), tail()]), n=3, ec=[0, 0, 0])
    # 2. 5 flipped header symbols: 50 / 60, found; 6: 48 / 60 = 0.8 -> 0.8f, not greater: not found
    for flips in (5, 6):
        s = soft(fsym(3))
        idx = 60 + np.array([3, 11, 18, 26, 37, 52][:flips])
        s[idx] = -s[idx]
        c["flips_%d" % flips] = dict(s=np.concatenate([noise(rng, 40, 0.05), s, tail()]), n=1 if flips == 5 else 0, ec=[0] if flips == 5 else [])
    # 3. the empty ring: behind a frame only 2A 10 of the header (40 / sqrt(40 * 60) = 0.8165 on a zeroed ring, (4 + 40) / 60 on the ring the header left); then a whole
    #    header of the other polarity with 2A 10 directly behind (dropped and zeroed: 0.8165; with the ring left as it was (40 - 4) / 60 = 0.6)
    c["empty_ring"] = dict(s=np.concatenate([soft(fsym(4)), soft(fsym(5)[80:]), -soft(HDR), soft(fsym(6)[80:]), tail()]), n=3, ec=[0, 0, 0])
    # 4. polarity: the inverted stream with -i, with --softinv, with neither (every header dropped, the ring emptied each time)
    pol = np.concatenate([noise(rng, 33, 0.05), soft(fsym(7), rng, (0.8, 1.2)), noise(rng, 140, 0.05), soft(fsym(8), rng, (0.8, 1.2)), tail(37)])
    c["inverted_inv"] = dict(s=-pol, inv=1, n=2, ec=[0, 0])
    c["inverted_softinv"] = dict(s=-pol, softinv=True, n=2, ec=[0, 0])
    c["inverted_neither"] = dict(s=-pol, n=0, ec=[], last_drop=33 + ONAIR + 140 + 120)
    # 5. byte errors in bytes 6..239, parity bytes and the last message byte (215) among them, made by swapping the symbol pairs of data bits
    for nerr, seed in ((1, 1), (12, 2), (13, 3)):
        r2 = np.random.default_rng(500 + seed)
        s = soft(fsym(9 + nerr % 3), r2, (0.8, 1.2))
        fixed = {1: [215], 12: [215, 216, 239, 6], 13: [215, 217, 238, 6]}[nerr]
        others = [int(b) for b in r2.permutation(np.arange(7, 215)) if b not in fixed][:nerr - len(fixed)]
        damage(s, 0, fixed + others, r2)
        c["errors_%d" % nerr] = dict(s=np.concatenate([noise(rng, 21, 0.05), s, tail()]), n=1, ec=[nerr if nerr <= 12 else -1])
    r2 = np.random.default_rng(77)
    c["startstop_only"] = dict(s=np.concatenate([noise(rng, 5, 0.05), damage(soft(fsym(12), r2, (0.8, 1.2)), 0, [6, 50, 215, 216, 239], r2, bits=(0, 9)), tail()]), n=1, ec=[0])
    # 6. pairs of two equal symbols, zeros among them: s2 - s1 = 0 decides 1, then ^ inv
    s = soft(fsym(13), rng, (0.8, 1.2))
    for byte, bit, v in ((20, 1, 0.0), (20, 5, 0.25), (99, 8, -0.5), (150, 3, 0.0), (215, 2, 0.0), (230, 7, 1.0)):
        s[20 * byte + 2 * bit] = s[20 * byte + 2 * bit + 1] = np.float32(v)
    s[20 * 150 + 6] = np.float32(-0.0)
    c["zero_pairs"] = dict(s=np.concatenate([noise(rng, 50, 0.05), s, tail()]), n=1)
    c["zero_pairs_inv"] = dict(s=np.concatenate([noise(rng, 50, 0.05), -s, tail()]), inv=1, n=1)
    # 7. 60 exact zeros ahead of a header: 0 / 0, not a hit
    c["zero_window"] = dict(s=np.concatenate([noise(rng, 50, 0.05), np.zeros(60, np.float32), soft(fsym(14)[60:]), np.zeros(75, np.float32), soft(fsym(15)[60:]), tail()]), n=2, ec=[0, 0])
    for v in c.values():
        v.setdefault("inv", 0); v.setdefault("softinv", False)
    return c


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = case_streams()
    return _cases


def cap_stream(nframes=22):
    """4 + 16 + 2 frames back to back for one channel: a consumer of one channel holds 20 records a call"""
    return np.concatenate([soft(fsym(k % 24)) for k in range(nframes)])


def random_cuts(n, seed, lo=1, hi=5200):
    rng = np.random.default_rng(seed)
    out, tot = [], 0
    while tot < n:
        k = int(rng.integers(lo, hi))
        out.append(k); tot += k
    return out
