"""Shared by tests/test_m20_hits_emu.py and tests/test_gpu_m20_hits.py: constructed M20 hit records (hard bits, valid bits, channel, header score) for the per-hit
device decoder of base-rate and mixed engines (radiosonde_auto_rx_amd/csrc/sonde_m20_hits_dev.h), the emulator binding (tests/emu/m20_hits_emu.cpp), and the arbiter:
a numpy restatement of mxx_bytes (sonde_engine.cpp: differential decoding into the channel's persistent characters, terminator, bits2bytes) followed by the library's
own sonde_m20_frame_finish for the verdicts.

A record is (name, bits [165] u8 — 8 hard bits a byte, LSB first —, nbits, channel, mv).  Every single case has a channel of its own; the `chain` records share one.
The first character of a frame is never '1' (the first bit is compared with the value '0' = 0x30, m20mod.c:1321,1348), so the top bit of frame byte 0 does not
survive the way through the bits: a length byte L arrives as L & 0x7F.  The length-byte cases therefore exist twice: as records (LEN_CASES, what the kernel sees),
and as plain frame bytes for the verdict function alone (verdict_frames(), where the clamp at 0x85 is reachable)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tools import synth
from radiosonde_auto_rx_amd.engine import SondeM20Frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_SRC = os.path.join(EMU_DIR, "m20_hits_emu.cpp")
EMU_SO = os.path.join(EMU_DIR, "libm20_hits_emu.so")
REPLAY_SRC = os.path.join(EMU_DIR, "m20_hits_replay.cpp")
DEPS = [EMU_SRC, os.path.join(EMU_DIR, "wave_emu.h"), os.path.join(ROOT, "include", "sonde_hip.h")] + \
       [os.path.join(CSRC, h) for h in ("sonde_m20_hits_dev.h", "sonde_softin_mxx_dev.h", "sonde_softin_wave_dev.h", "sonde_rs_dev.h")]
NBYTES, NBITS, CHARS = 165, 1320, 1328
LENGTHS = (0x00, 0x01, 0x44, 0x45, 0x46, 0x85, 0x86, 0xFF)
SHORT = (0, 7, 8, 700, 1319)


def load_emu():
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in DEPS):
        tmp = EMU_SO + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", tmp, EMU_SRC])
        os.replace(tmp, EMU_SO)
    L = C.CDLL(EMU_SO)
    L.emu_m20_hits_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_void_p, C.POINTER(SondeM20Frame),
                                   C.POINTER(C.c_uint)]
    L.emu_m20_verdicts.argtypes = [C.c_void_p, C.POINTER(SondeM20Frame)]
    return L


# ---------------------------------------------------------------- frames and their hard bits
def frame165(k, *, length=None, msb_lost=True, good=True, **kw):
    """165 frame bytes: tools/synth.m20_frame in front, random bytes behind.  length: the length byte, with the frame checksum where print_frame() then looks for it
    (good: the right one); msb_lost: the place is that of length & 0x7F, what the length byte is behind the differential code."""
    rng = np.random.default_rng(2000 + k)
    f = bytearray(synth.m20_frame(k, rng=np.random.default_rng(20_000 + k), good_checksum=good, **kw) + bytes(rng.integers(0, 256, NBYTES - 70, dtype=np.uint8)))
    if length is not None:
        f[0] = length
        b0 = length & 0x7F if msb_lost else length                          # the byte the decoder has in front
        pc = min(b0, 0x45 + 64) - 1                                         # (print_frame() clamps the aux length to 64 bytes, m20mod.c:891-894)
        if pc >= 2:                                                         # (below that the checksum would lie on the length byte itself)
            cs = synth.m10_checksum(bytes([b0]) + bytes(f[1:pc])) ^ (0 if good else 0x0101)
            f[pc] = cs >> 8; f[pc + 1] = cs & 0xFF
    return bytes(f)


def hard_bits(frame, first=0):
    """the 1320 Manchester-sliced bits whose differential decoding gives the frame's bits, MSB first per byte (a '1' = the same level as the bit before; the frame's
    first bit cannot be said this way), packed 8 a byte, LSB first, as FrameRec.frame holds them"""
    d = np.unpackbits(np.frombuffer(bytes(frame), np.uint8))
    toggles = 1 - d.astype(np.int64)
    toggles[0] = first
    return np.packbits((np.cumsum(toggles) & 1).astype(np.uint8), bitorder="little")


_records = {}


def records():
    """[(name, bits, nbits, channel, mv)] in launch order, and the number of channels"""
    if "r" in _records:
        return _records["r"]
    recs, ch = [], 0

    def single(name, frame, nbits=NBITS, first=0):
        nonlocal ch
        recs.append((name, hard_bits(frame, first), nbits, ch, np.float32(0.5 + 0.01 * ch) * (-1 if ch % 3 == 1 else 1)))
        ch += 1
    single("good", frame165(1))
    single("bad_checksum", frame165(2, good=False))
    single("blk_zero", frame165(3, blk="zero"))
    single("blk_bad", frame165(4, blk="bad"))
    single("fw8", frame165(5, fw=8))
    single("fw6_first_bit_1", frame165(6, fw=6), first=1)
    for L in LENGTHS:
        single("len_%02x" % L, frame165(10 + L % 7, length=L))
    single("len_45_bad", frame165(9, length=0x45, good=False))
    for nb in SHORT:
        single("nbits_%d" % nb, frame165(30 + nb % 5), nbits=nb)
    # three records of one channel in a row, full, short, full, with other channels' records between them; the same short record on a fresh channel
    chain = ch
    ch += 1
    a, b, c = frame165(41), frame165(42), frame165(43, good=False)
    recs.append(("chain_full_1", hard_bits(a), NBITS, chain, np.float32(0.81)))
    single("between_1", frame165(44))
    recs.append(("chain_short", hard_bits(b, 1), 700, chain, np.float32(-0.82)))
    single("between_2", frame165(45, blk="zero"))
    recs.append(("chain_full_2", hard_bits(c), NBITS, chain, np.float32(0.83)))
    single("short_fresh", b, nbits=700, first=1)
    _records["r"] = (recs, ch)
    return _records["r"]


def verdict_frames():
    """{name: 172 frame bytes} for m20_wave_verdicts alone: every length byte of LENGTHS as it stands, checksum good and bad"""
    out = {}
    for L in LENGTHS:
        for good in (True, False):
            out["len_%02x_%s" % (L, "good" if good else "bad")] = frame165(50 + L % 11, length=L, msb_lost=False, good=good) + bytes(7)
    return out


# ---------------------------------------------------------------- the arbiter
def arbiter(recs, n_channels, chars=None):
    """mxx_bytes(e, r, 101 + 64, ..) restated, then the library's sonde_m20_frame_finish -> ([SondeM20Frame], the channels' characters afterwards)"""
    from radiosonde_auto_rx_amd.engine import lib
    fin = lib().sonde_m20_frame_finish
    fin.argtypes = [C.POINTER(SondeM20Frame)]
    chars = np.zeros((n_channels, CHARS), np.uint8) if chars is None else chars
    out = []
    for _, bits, nb, ch, mv in recs:
        nv = min(int(nb), NBITS)
        b = np.unpackbits(np.asarray(bits, np.uint8), bitorder="little")[:nv].astype(np.int64)
        chars[ch, :nv] = 0x31 ^ (np.concatenate([[0x30], b[:-1]])[:nv] ^ b)       # the first bit against '0'
        chars[ch, nv] = 0
        f = SondeM20Frame()
        f.channel, f.nbits, f.mv, f.mv_pos = int(ch), nv, float(mv), 0
        C.memmove(f.frame, np.packbits(chars[ch, :NBITS] == 0x31).tobytes(), NBYTES)      # bits2bytes: big endian, anything but '1' is 0
        assert fin(C.byref(f)) == 0
        out.append(f)
    return out, chars


def finish(frame172):
    """sonde_m20_frame_finish on plain frame bytes -> SondeM20Frame (all other fields 0)"""
    from radiosonde_auto_rx_amd.engine import lib
    fin = lib().sonde_m20_frame_finish
    fin.argtypes = [C.POINTER(SondeM20Frame)]
    f = SondeM20Frame()
    C.memmove(f.frame, bytes(frame172), 172)
    assert fin(C.byref(f)) == 0
    return f


# ---------------------------------------------------------------- the emulated launch
def pack(recs, max_frames=None, start=0):
    """records (counter values start, start + 1, ..) -> the by-slot arrays of a ring of max_frames slots (a later record overwrites the slot of an earlier one)"""
    mf = max_frames or len(recs)
    bits, nbits, chan, mv = np.zeros((mf, NBYTES), np.uint8), np.zeros(mf, np.int32), np.zeros(mf, np.int32), np.zeros(mf, np.float32)
    for i, (_, b, nb, ch, m) in enumerate(recs):
        s = (start + i) % mf
        bits[s], nbits[s], chan[s], mv[s] = b, nb, ch, m
    return bits, nbits, chan, mv


def emu_run(E, recs, n_channels, *, grid=1, max_frames=None, start=0, chars=None):
    """the records through one emulated launch -> ([SondeM20Frame] in counter order, characters afterwards, {done, ticket} afterwards)"""
    mf = max_frames or len(recs)
    bits, nbits, chan, mv = pack(recs, mf, start)
    chars = np.zeros((n_channels, CHARS), np.uint8) if chars is None else chars
    out = (SondeM20Frame * mf)()
    C.memset(out, 0xEE, C.sizeof(out))
    done = (C.c_uint * 2)(start, 0)
    rc = E.emu_m20_hits_run(bits.ctypes.data, nbits.ctypes.data, chan.ctypes.data, mv.ctypes.data, n_channels, mf, start + len(recs), grid, chars.ctypes.data, out, done)
    assert rc == 0, rc
    first = max(start, start + len(recs) - mf)
    return [SondeM20Frame.from_buffer_copy(out[c % mf]) for c in range(first, start + len(recs))], chars, (done[0], done[1])


def key(f):
    """all 208 bytes of a record"""
    return bytes(f)
