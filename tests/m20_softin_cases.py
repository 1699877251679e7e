"""Streams and arbiters shared by tests/test_softin_m20_emu.py (the device M20 soft-bit consumer under the CPU wave emulator) and tests/test_gpu_softin_m20.py (the same
source as k_softin_m20 on the device): symbol streams built from tools/synth.py frames, the host framer (sonde_softin_create(SONDE_M20) / sonde_softin_set_m10_skip / push /
fetch_m20 — pinned byte for byte to the compiled reference by tests/test_m20_fields.py) and the emulator driver tests/emu/softin_m20_emu.cpp.

A record is compared as the tuple of rec(): nbits, len, cs_ok, cs_calc, blk_ok, fw, mv_pos, the bits of mv and the 172 frame bytes."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from tools import synth
from radiosonde_auto_rx_amd.engine import SondeM20Frame, SONDE_M20

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_SRC = os.path.join(EMU_DIR, "softin_m20_emu.cpp")
EMU_SO = os.path.join(EMU_DIR, "libsoftin_m20_emu.so")
DEPS = [EMU_SRC, os.path.join(EMU_DIR, "wave_emu.h"), os.path.join(CSRC, "sonde_softin_mxx_dev.h"), os.path.join(CSRC, "sonde_softin_wave_dev.h"), os.path.join(CSRC, "sonde_rs_dev.h"), os.path.join(ROOT, "include", "sonde_hip.h")]
REF = os.path.join(ROOT, "oracle", "_ref", "m20mod")
HEADER = "10011001100110010100110010011001"                # the 32 raw header symbols `m20mod` searches for
NSYM = 2 * (101 + 64) * 8                                   # symbols of a frame behind the header
STAGE_MAX = 12288                                           # M10_STAGE_MAX of sonde_softin_wave_dev.h


class EmuState(C.Structure):
    """EmuM20State (tests/emu/softin_m20_emu.cpp)"""
    _fields_ = [(n, C.c_int) for n in ("mode", "inv", "mpos", "mhalf", "mbit0", "mskip")] + [("ms1", C.c_float), ("mv", C.c_float), ("bits_in", C.c_uint64), ("hdr_bit", C.c_uint64)]


def load_emu():
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in DEPS):
        tmp = EMU_SO + ".%d.tmp" % os.getpid()
        # (-ffp-contract=off: the score is the reference's expression, every product and sum rounded on its own)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", tmp, EMU_SRC])
        os.replace(tmp, EMU_SO)
    L = C.CDLL(EMU_SO)
    L.emu_m20_run.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(SondeM20Frame), C.c_int, C.POINTER(C.c_int), C.POINTER(EmuState)]
    L.emu_m20_verdicts.argtypes = [C.c_void_p, C.POINTER(SondeM20Frame)]
    return L


def load_host():
    from radiosonde_auto_rx_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    L = C.CDLL(engine.LIB_PATH)
    L.sonde_softin_create.argtypes = [C.c_int32] * 5 + [C.POINTER(C.c_void_p)]
    L.sonde_softin_destroy.argtypes = [C.c_void_p]
    L.sonde_softin_push.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    L.sonde_softin_set_m10_skip.argtypes = [C.c_void_p, C.c_int32]
    L.sonde_softin_fetch_m20.argtypes = [C.c_void_p, C.POINTER(SondeM20Frame), C.c_int32]
    L.sonde_m20_rawline.argtypes = [C.POINTER(SondeM20Frame), C.c_int, C.c_char_p, C.c_size_t]
    L.sonde_m20_frame_finish.argtypes = [C.POINTER(SondeM20Frame)]
    return L


def rec(f):
    """what must agree exactly (mv by its bits); f: a SondeM20Frame or a dict of SoftinDev.fetch_m20"""
    g = (lambda k: f[k]) if isinstance(f, dict) else (lambda k: getattr(f, k))
    fr = g("frame")
    return (g("nbits"), g("len"), g("cs_ok"), g("cs_calc"), g("blk_ok"), g("fw"), g("mv_pos"), struct.pack("<f", g("mv")), bytes(fr))


def rec_no_mv(r):
    return r[:7] + r[8:]


def mv_of(r):
    return struct.unpack("<f", r[7])[0]


def mv_within_one_ulp(a, b):
    """two records' scores: equal, or neighbours among the floats (the device's double divide / sqrt ahead of the rounding to float)"""
    ia, ib = struct.unpack("<i", a[7])[0], struct.unpack("<i", b[7])[0]
    return (ia < 0) == (ib < 0) and abs(ia - ib) <= 1


def host_frames(H, s, skip, softinv=False):
    """the arbiter: records and `-r -v` lines of the host framer over the whole stream"""
    s = np.ascontiguousarray(s, np.float32)
    h = C.c_void_p()
    assert H.sonde_softin_create(SONDE_M20, 0, int(softinv), 0, 0, C.byref(h)) == 0
    assert H.sonde_softin_set_m10_skip(h, int(skip)) == 0
    assert H.sonde_softin_push(h, s.ctypes.data, len(s)) == 0
    buf = (SondeM20Frame * (len(s) // 2672 + 2))()
    n = H.sonde_softin_fetch_m20(h, buf, len(buf))
    assert 0 <= n < len(buf)
    H.sonde_softin_destroy(h)
    return [rec(buf[i]) for i in range(n)], [rawline(H, buf[i]) for i in range(n)]


def rawline(H, f, verbose=1):
    line = C.create_string_buffer(420)
    n = H.sonde_m20_rawline(C.byref(f), verbose, line, 420)
    assert n >= 0
    return line.raw[:n].decode()


def emu_frames(E, s, calls, skip, softinv=False, cap=64, H=None):
    """the emulated consumer over the stream cut into calls (the last length repeats): records, frames dropped for want of room, end state [, lines]"""
    s = np.ascontiguousarray(s, np.float32)
    buf = (SondeM20Frame * (len(s) // 2672 + 2))()
    cl = (C.c_int * len(calls))(*calls)
    dropped, end = C.c_int(0), EmuState()
    n = E.emu_m20_run(s.ctypes.data, len(s), cl, len(calls), int(softinv), int(skip), cap, buf, len(buf), C.byref(dropped), C.byref(end))
    assert 0 <= n < len(buf), n
    for i in range(n):
        assert buf[i].channel == 0
    st = {k: getattr(end, k) for k, _ in EmuState._fields_}
    if H is None:
        return [rec(buf[i]) for i in range(n)], dropped.value, st
    return [rec(buf[i]) for i in range(n)], dropped.value, st, [rawline(H, buf[i]) for i in range(n)]


def frame_symbols(data, preamble=True):
    """0 / 1 symbols of one frame of 165 bytes: [44 symbols of the 1001 idle pattern,] the 32 header symbols, 1320 Manchester pairs in the differential code (a 1 repeats
    the pair before it, a 0 flips it).  The decoder reads the frame's first bit against '0', which never gives a 1: byte 0 is below 0x80 whatever is sent."""
    assert len(data) == 165 and data[0] < 0x80
    bits = np.unpackbits(np.frombuffer(bytes(data), np.uint8))
    m, pairs = 0, [1, 0]
    for b in bits[1:]:
        m = m if b else 1 - m
        pairs += [1 - m, m]
    sym = np.array(([1, 0, 0, 1] * 11 if preamble else []) + [int(c) for c in HEADER] + pairs, np.uint8)
    if preamble and data[0] >> 6 == 1:                     # (tools/synth.py sends the same for the frames it can send: those that begin 01)
        assert np.array_equal(sym, synth.m10_symbols(data=bytes(data)))
    return sym


def m20_bytes(k=0, *, length=0x45, fw=6, blk="ok", good=True, seed=None):
    """165 frame bytes: tools/synth.m20_frame in front, random bytes behind, then the length byte, the firmware byte and the frame checksum where m20mod looks for them
    (length >= 0x45: firmware at 0x43, below: at length - 2; checksum at min(length, 0x45 + 64) - 1)"""
    rng = np.random.default_rng(7000 + k if seed is None else seed)
    f = bytearray(synth.m20_frame(k, fw=6, blk=blk, rng=np.random.default_rng(7100 + k)) + bytes(rng.integers(0, 256, 165 - 70, dtype=np.uint8)))
    f[0] = length
    flen = min(length, 0x45 + 64)
    pos_fw = 0x43 if length >= 0x45 else length - 2
    if pos_fw > 0x17:                                      # (in front of that it would lie in the block or on the length byte)
        f[pos_fw] = fw
    pc = flen - 1
    if pc >= 1:
        cs = synth.m10_checksum(bytes(f[:pc]))
        if not good:
            cs ^= 0x0101
        f[pc] = cs >> 8; f[pc + 1] = cs & 0xFF
    return bytes(f)


def soft(sym, rng=None, jitter=(1.0, 1.0), sigma=0.0):
    s = 2.0 * np.asarray(sym, np.float64) - 1.0
    if rng is not None:
        s = s * rng.uniform(jitter[0], jitter[1], len(s)) + (rng.normal(0.0, sigma, len(s)) if sigma else 0.0)
    return s.astype(np.float32)


def noise(rng, n, sigma=0.3):
    return rng.normal(0.0, sigma, n).astype(np.float32)


def dense_stream(nframes, seed=11, lead=0):
    """frames back to back, one every 2672 symbols: header + frame, no preamble, nothing between (what -vvv / no-skip can decode and the skip cannot)"""
    rng = np.random.default_rng(seed)
    parts = [noise(rng, lead)] if lead else []
    for k in range(nframes):
        parts.append(soft(frame_symbols(m20_bytes(k), preamble=False), rng, (0.8, 1.2), 0.05))
    parts.append(noise(rng, 60))
    return np.concatenate(parts)


def threshold_stream(flips, amp=1.0, scaled=5, seed=3):
    """a clean header with `flips` symbols flipped and symbol `scaled` of it multiplied by amp (score (32 - 2 flips) / 32 at amp 1), a frame behind it, a noise lead of
    small amplitude in front: whether the header is found is the threshold's decision alone"""
    rng = np.random.default_rng(seed)
    s = soft(frame_symbols(m20_bytes(1), preamble=False))
    idx = [3, 11, 18, 26, 30][:flips]
    assert scaled not in idx
    s[idx] = -s[idx]
    s[scaled] = np.float32(s[scaled] * np.float32(amp))
    return np.concatenate([noise(rng, 40, 0.05), s, noise(rng, 50, 0.05)])


def edge_amplitudes(host):
    """amplitudes of one header symbol (three others flipped) around the one at which the score crosses 0.8, found by bisection with the host framer as arbiter:
    the two neighbouring floats at the crossing, two more float steps on either side, and the amplitudes that move the score by about 5e-4"""
    def found(a):
        return len(host_frames(host, threshold_stream(3, amp=a), 1)[0]) == 1
    lo, hi = np.float32(0.0), np.float32(1.0)
    assert not found(lo) and found(hi)
    while np.nextafter(lo, np.float32(2)) < hi:
        mid = np.float32((lo + hi) / 2)
        if mid == lo or mid == hi:
            break
        if found(mid):
            hi = mid
        else:
            lo = mid
    amps = [lo, hi]
    for _ in range(2):
        amps = [np.nextafter(amps[0], np.float32(-1))] + amps + [np.nextafter(amps[-1], np.float32(2))]
    return [np.float32(lo - 0.02), np.float32(lo - 0.005)] + amps + [np.float32(hi + 0.005), np.float32(hi + 0.02)], lo, hi


def variant_frames():
    """name -> (165 frame bytes, expected len / fw / cs_ok / blk_ok or None where the arbiter alone says) of the length and check variants a symbol stream can carry"""
    v = {
        "len_45": (m20_bytes(0), dict(len=0x46, fw=6, cs_ok=1, blk_ok=1)),
        "len_43": (m20_bytes(1, length=0x43), dict(len=0x44, fw=6, cs_ok=1, blk_ok=1)),
        "len_7f": (m20_bytes(2, length=0x7F), dict(len=0x80, fw=6, cs_ok=1, blk_ok=1)),
        "len_0": (m20_bytes(3, length=0), dict(len=1, fw=0, cs_ok=1, blk_ok=1)),
        "len_1": (m20_bytes(4, length=1), dict(len=2, fw=0, cs_ok=0)),
        "len_2": (m20_bytes(5, length=2), dict(len=3, cs_ok=1)),
        "fw_8": (m20_bytes(6, fw=8), dict(len=0x46, fw=8, cs_ok=1)),
        "fw_21": (m20_bytes(7, fw=0x21), dict(len=0x46, fw=0, cs_ok=1)),
        "fw_20": (m20_bytes(8, fw=0x20), dict(len=0x46, fw=0x20, cs_ok=1)),
        "blk_zero": (m20_bytes(9, blk="zero"), dict(blk_ok=-1, cs_ok=1)),
        "blk_bad": (m20_bytes(10, blk="bad"), dict(blk_ok=0, cs_ok=1)),
        "cs_bad": (m20_bytes(11, good=False), dict(cs_ok=0, blk_ok=1)),
    }
    return v


def variant_stream(data, seed=5, header_in_payload=False):
    """noise, one frame with its preamble, noise; header_in_payload: 32 symbols in the middle of the frame are overwritten with the header pattern"""
    rng = np.random.default_rng(seed)
    s = soft(frame_symbols(data), rng, (0.8, 1.2), 0.05)
    if header_in_payload:
        at = 44 + 32 + 1000
        s[at:at + 32] = soft([int(c) for c in HEADER])
    return np.concatenate([noise(rng, 77), s, noise(rng, 300)])


def equal_pair_stream(seed=6):
    """a frame in which some pairs consist of two equal symbols (s2 - s1 = 0, also as -0.0 + 0.0 and 0.25 - 0.25): the reference decides `>= 0`, a 1"""
    rng = np.random.default_rng(seed)
    s = soft(frame_symbols(m20_bytes(13)), rng, (0.8, 1.2))
    for k, v in ((100, 0.0), (101, 0.25), (377, -0.5), (900, 0.0)):
        at = 44 + 32 + 2 * k
        s[at] = s[at + 1] = np.float32(v)
    s[44 + 32 + 2 * 900] = np.float32(-0.0)
    return np.concatenate([noise(rng, 50), s, noise(rng, 100)])


def skip_end_stream(gap, seed=9):
    """a frame, `gap` symbols of noise, then a header and its frame with nothing in front: the skip drops 5 * 808 - 1320 = 2720 symbols behind the first frame, and the
    ring is not fed meanwhile — with a gap of 2720 the second header is seen whole, with 2719 its first symbol is lost"""
    rng = np.random.default_rng(seed)
    a = soft(frame_symbols(m20_bytes(14)), rng, (0.9, 1.1))
    b = soft(frame_symbols(m20_bytes(15), preamble=False))
    return np.concatenate([noise(rng, 30), a, noise(rng, gap, 0.05), b, noise(rng, 80)])
