"""Shared by tests/test_lms6_rs_emu.py, tests/test_lms6_dec_block_rs.py and tests/test_gpu_lms6_rs.py: the cases for the device RS(255,223) decoder of LMS6 / LMS-X
blocks (radiosonde_auto_rx_amd/csrc/sonde_rs223_dev.h), the emulator binding (tests/emu/lms6_rs_emu.cpp) and the model of a record.

The word-level oracle is the compiled reference, oracle/_ref/libref_ecc.so: ref_ecc_decode(2, ..) is rs_decode of the CCSDS code.  model_record() assembles a
sonde_lms6_rs_t from it and frmsync_X (four byte compares at 5 / 40 / 45) the way proc_frame would have called it.  Everything is bit-exact: no tolerances.

Words are numpy uint8[255] in the reference's coefficient order (parity 0 .. 31, message 32 .. 254); a block carries its codeword reversed from offset `at` on:
cw[254 - j] = block[at + j].  Codewords come from sonde_ecc_encode(SONDE_ECC_RS255CCSDS), frames from tools/synth.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from tools import synth
from radiosonde_auto_rx_amd.engine import lib
from radiosonde_auto_rx_amd.family import Lms6Rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_SRC = os.path.join(EMU_DIR, "lms6_rs_emu.cpp")
EMU_SO = os.path.join(EMU_DIR, "liblms6_rs_emu.so")
REFLIB = os.path.join(ROOT, "oracle", "_ref", "libref_ecc.so")
DEPS = [EMU_SRC, os.path.join(EMU_DIR, "wave_emu.h"), os.path.join(ROOT, "include", "sonde_hip.h"), os.path.join(ROOT, "include", "sonde_ecc.h")] + \
       [os.path.join(CSRC, h) for h in ("sonde_rs223_dev.h", "sonde_rs_dev.h", "sonde_ecc.cpp")]
CCSDS = 2                                                    # SONDE_ECC_RS255CCSDS, and the reference harness's number of the same code
T = 16
BB_LEN = 308
SYNC_X = bytes([0x24, 0x46, 0x05, 0x00])
WORD_SEED = 22310                                            # found with the reference (see _check_words): the words beyond t give each failure code


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def have_ref():
    return os.path.exists(REFLIB)


_ref = []


def ref():
    if not _ref:
        _ref.append(C.CDLL(REFLIB))
    return _ref[0]


def load_emu():
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in DEPS):
        tmp = EMU_SO + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-shared", "-fPIC", "-o", tmp, EMU_SRC])
        os.replace(tmp, EMU_SO)
    L = C.CDLL(EMU_SO)
    L.emu_rs223_decode.argtypes = [C.POINTER(C.c_uint8)] * 3
    L.emu_lms6_rs_run.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(Lms6Rs)]
    return L


# ---------------------------------------------------------------- the reference and the emulator on one word
def ref_decode(word):
    """rs_decode of the reference -> (return value, the word afterwards, err_pos[16], err_val[16]); positions and values zero behind the count and on failure, which
    is what the device reports (the reference leaves what its Chien loop had found before it gave up)"""
    w = np.ascontiguousarray(word, np.uint8).copy()
    ep, ev = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    r = ref().ref_ecc_decode(CCSDS, _u8(w), _u8(ep), _u8(ev))
    n = max(r, 0)
    assert n <= T
    ep[n:] = 0; ev[n:] = 0
    return r, w, ep[:T].copy(), ev[:T].copy()


def emu_decode(E, word):
    w = np.ascontiguousarray(word, np.uint8).copy()
    ep, ev = np.full(T, 0xEE, np.uint8), np.full(T, 0xEE, np.uint8)
    r = E.emu_rs223_decode(_u8(w), _u8(ep), _u8(ev))
    return r, w, ep, ev


_codec = []


def encode(msg223):
    """the codeword of 223 message bytes: sonde_ecc_encode(SONDE_ECC_RS255CCSDS)"""
    L = lib()
    if not _codec:
        L.sonde_ecc_create.restype = C.c_void_p
        L.sonde_ecc_create.argtypes = [C.c_int]
        L.sonde_ecc_encode.argtypes = [C.c_void_p, C.POINTER(C.c_uint8)]
        _codec.append(L.sonde_ecc_create(CCSDS))
    cw = np.zeros(255, np.uint8)
    cw[32:] = np.asarray(msg223, np.uint8)
    assert L.sonde_ecc_encode(_codec[0], _u8(cw)) == 0
    return cw


def damage(cw, nerr, rng, lo=0, hi=255):
    w = cw.copy()
    for p in rng.choice(np.arange(lo, hi), size=nerr, replace=False):
        w[p] ^= rng.integers(1, 256)
    return w


# ---------------------------------------------------------------- word cases
_words = []


def word_cases():
    """[(name, word, errors put in)] — about 300 words, seeded"""
    if _words:
        return _words
    rng = np.random.default_rng(WORD_SEED)
    new = lambda: encode(rng.integers(0, 256, 223))              # noqa: E731
    out = []
    for nerr, reps in ((0, 4), (1, 20), (2, 20), (15, 25), (16, 30), (17, 50), (18, 40), (19, 30), (24, 25), (40, 20)):
        for k in range(reps):
            out.append(("random_%d_%d" % (nerr, k), damage(new(), nerr, rng), nerr))
    # single errors at both ends and on both sides of the message / parity boundary of the BLOCK: block byte 5 + j is cw[254 - j], so the last message byte is cw[32]
    # and the first parity byte cw[31]; the indices the issue names (0, 254, 222 / 223) as codeword indices as well
    for p in (0, 254, 222, 223, 31, 32):
        w = new(); w[p] ^= 0x5A
        out.append(("single_at_%d" % p, w, 1))
    w = new(); w[222] ^= 0x11; w[223] ^= 0x22
    out.append(("pair_222_223", w, 2))
    for k in range(3):
        out.append(("parity_only_16_%d" % k, damage(new(), 16, rng, 0, 32), 16))
    out.append(("parity_only_17", damage(new(), 17, rng, 0, 32), 17))
    out.append(("all_zero", np.zeros(255, np.uint8), 0))
    out.append(("all_ff", np.full(255, 0xFF, np.uint8), 255))
    for v in (1, 0x80, 0xFF):
        w = new(); w[100] ^= v
        out.append(("value_%02x" % v, w, 1))
    # a block cut short: its last 255 - k bytes are zero, which are the LOWEST coefficients of the word
    for k in (250, 240, 223, 100, 30, 1):
        w = new(); nz = int(np.count_nonzero(w[:255 - k])); w[:255 - k] = 0
        out.append(("short_block_%d" % k, w, nz))
    # a miscorrection by construction: d = the codeword of a single message byte has weight 33 (the code's minimum distance); c + 17 of d's symbols is 17 errors from c
    # and 16 from c + d, so the decoder lands on c + d
    for k, at in enumerate((40, 200)):
        m = np.zeros(223, np.uint8); m[at] = 0x37 + k
        d = encode(m)
        nz = np.flatnonzero(d)
        assert len(nz) == 33
        w = new()
        take = rng.choice(nz, size=17, replace=False)
        w[take] ^= d[take]
        out.append(("miscorrected_%d" % k, w, 17))
    _words.extend(out)
    if have_ref():
        _check_words(out)
    return _words


def _check_words(words):
    """what the case list must contain, by the reference: every failure code among the words beyond t, and a word with more than t errors that rs_decode 'repairs'"""
    codes, mis = set(), 0
    for name, w, nerr in words:
        if nerr > T:
            r = ref_decode(w)[0]
            codes.add(r if r < 0 else "ok")
            mis += r > 0
    assert {-1, -2, -3} <= codes, "WORD_SEED: the words beyond t give only %r; search another seed" % codes
    assert mis >= 1


# ---------------------------------------------------------------- block records and their model
def syncx_at(bb):
    """frmsync_X (lms6Xmod.c:815-827): the position of 24 46 05 00 among 5 / 40 / 45, 0 when it is at none of them"""
    for at in (5, 40, 45):
        if bytes(bb[at:at + 4]) == SYNC_X:
            return at
    return 0


def _hyp(h, at, r=0, pos=None, val=None):
    h.at, h.err = at, r
    for i in range(T):
        h.pos[i] = int(pos[i]) if pos is not None else 0
        h.val[i] = int(val[i]) if val is not None else 0


def _run(bb, at, h):
    r, w, pos, val = ref_decode(bb[at:at + 255][::-1])
    _hyp(h, at, r, pos, val)
    return r, w[::-1]


def model_record(block, blen, decoded=1):
    """the sonde_lms6_rs_t of one block record, assembled from the reference's rs_decode and frmsync_X"""
    o = Lms6Rs()
    if not decoded or blen <= 0:
        return o
    bb = np.zeros(320, np.uint8)
    bb[:min(blen, BB_LEN)] = np.frombuffer(bytes(block), np.uint8)[:min(blen, BB_LEN)]
    at_x = syncx_at(bb) if blen > 100 else 0
    if at_x:
        _run(bb, at_x, o.hX)
    r6, w6 = _run(bb, 5, o.h6)
    if r6 > 0:
        bb[5:260] = w6
        at_6x = syncx_at(bb) if blen > 100 else 0
        if at_6x:
            _run(bb, at_6x, o.h6X)
    else:
        _hyp(o.h6X, -1)
    return o


def rs_bytes(r):
    return bytes(memoryview(r))


def emu_records(E, blocks, blens, decoded=None, *, grid=1, extra=0, fill=0xEE):
    """the records through the emulated launch -> (list of Lms6Rs, the `extra` records behind them as bytes: still `fill` when nothing wrote there)"""
    n = len(blocks)
    by = np.zeros((max(n, 1), BB_LEN), np.uint8)
    for i, b in enumerate(blocks):
        by[i] = np.frombuffer(bytes(b), np.uint8)
    keep = by.copy()
    bl = np.ascontiguousarray(list(blens) + [0] * (1 - min(n, 1)), np.int32)
    dec = None if decoded is None else np.ascontiguousarray(list(decoded) + [0] * (1 - min(n, 1)), np.int32)
    out = (Lms6Rs * (n + extra + 1))()
    C.memset(out, fill, C.sizeof(out))
    rc = E.emu_lms6_rs_run(by.ctypes.data, BB_LEN, bl.ctypes.data, None if dec is None else dec.ctypes.data, n, grid, out)
    assert rc == 0, rc
    assert (by == keep).all()                                     # the input is read only
    tail = bytes(memoryview(out))[n * C.sizeof(Lms6Rs):(n + extra) * C.sizeof(Lms6Rs)]
    return [Lms6Rs.from_buffer_copy(out[i]) for i in range(n)], tail


def word_block(word):
    """a word embedded in a block at offset 5, a full LMS6 block otherwise: (bytes[308], blen = 260)"""
    bb = np.zeros(BB_LEN, np.uint8)
    bb[0:5] = [0x00, 0x58, 0xF3, 0x3F, 0xB8]
    bb[5:260] = np.asarray(word, np.uint8)[::-1]
    return bb, 260


def frame_block(frame, at, blen):
    """a block whose codeword starts at `at`: 223 frame bytes and their 32 parity bytes, reversed (tools/synth.py: lms6_onair_bits)"""
    fr = np.frombuffer(bytes(frame), np.uint8)
    bb = np.zeros(BB_LEN, np.uint8)
    bb[0:5] = [0x00, 0x58, 0xF3, 0x3F, 0xB8]
    bb[at:at + 223] = fr
    bb[at + 223:at + 255] = synth.rs255_223_ccsds_parity(fr[::-1])[::-1]
    bb[blen:] = 0
    return bb


_blocks = []


def block_cases():
    """[(name, bytes[308], blen, decoded)]"""
    if _blocks:
        return _blocks
    rng = np.random.default_rng(22304)
    out = []

    def hurt(bb, n, lo=5, hi=260):
        b = bb.copy()
        for p in rng.choice(np.arange(lo, hi), size=n, replace=False):
            b[p] ^= rng.integers(1, 256)
        return b

    l6 = [frame_block(synth.lms6_frame(k), 5, 260) for k in range(4)]
    out.append(("lms6_clean", l6[0], 260, 1))
    out.append(("lms6_3_errors", hurt(l6[1], 3), 260, 1))
    out.append(("lms6_16_errors", hurt(l6[2], 16), 260, 1))
    out.append(("lms6_20_errors", hurt(l6[3], 20), 260, 1))
    for at in (5, 40, 45):
        x = frame_block(synth.lmsx_frame(at), at, 300)
        out.append(("lmsx_at%d_clean" % at, x, 300, 1))
        out.append(("lmsx_at%d_5_errors" % at, hurt(x, 5, at + 4, at + 255), 300, 1))
        out.append(("lmsx_at%d_19_errors" % at, hurt(x, 19, at + 4, at + 255), 300, 1))
        y = x.copy(); y[at + 1] ^= 0x01                           # sfX = 3: one sync byte wrong
        out.append(("lmsx_at%d_sync_damaged" % at, y, 300, 1))
    x5 = frame_block(synth.lmsx_frame(7), 5, 300)
    out.append(("lmsx_blen_100", np.where(np.arange(BB_LEN) < 100, x5, 0).astype(np.uint8), 100, 1))      # blen > 100 fails: hX does not run
    out.append(("lmsx_blen_101", np.where(np.arange(BB_LEN) < 101, x5, 0).astype(np.uint8), 101, 1))
    out.append(("blen_0", np.zeros(BB_LEN, np.uint8), 0, 1))
    out.append(("not_decoded", hurt(l6[0], 2), 260, 0))
    out.append(("noise", rng.integers(0, 256, BB_LEN).astype(np.uint8), 300, 1))
    out.append(("noise_short", np.where(np.arange(BB_LEN) < 37, rng.integers(0, 256, BB_LEN), 0).astype(np.uint8), 37, 1))
    # h6X != hX: a valid codeword at 5 that reads 24 46 05 00 at 40; in the raw bytes that sync is damaged, so hX finds nothing, h6 repairs it, and the type-10 branch
    # of a block that falls through sees the sync
    fr = bytearray(synth.lms6_frame(9)); fr[35:39] = SYNC_X
    z = frame_block(bytes(fr), 5, 300)
    z[41] ^= 0x40
    out.append(("h6x_differs", hurt(z, 4, 60, 255), 300, 1))
    # the same with the sync at 5 damaged: the repaired block is a clean LMS-X block at 5
    z = x5.copy(); z[6] ^= 0x02
    out.append(("h6x_differs_at5", hurt(z, 2, 20, 255), 300, 1))
    # filled up to more than one pass of a two-workgroup launch over 65 records: the blocks above with other damage
    base = [l6[0], l6[1], frame_block(synth.lmsx_frame(1), 5, 300), frame_block(synth.lmsx_frame(2), 40, 300), frame_block(synth.lmsx_frame(3), 45, 300)]
    k = 0
    while len(out) < 70:
        b = base[k % len(base)]
        n = int(rng.integers(0, 22))
        out.append(("more_%d_%d_errors" % (k, n), hurt(b, n, 5, 300), 300 if k % len(base) >= 2 else 260, 1))
        k += 1
    _blocks.extend(out)
    if have_ref():
        _check_blocks(out)
    return _blocks


def _check_blocks(blocks):
    by = {name: (b, blen, dec) for name, b, blen, dec in blocks}
    m = model_record(*by["h6x_differs"])
    assert m.hX.at == 0 and m.h6.err > 0 and m.h6X.at == 40, (m.hX.at, m.h6.err, m.h6X.at)
    m = model_record(*by["h6x_differs_at5"])
    assert m.hX.at == 0 and m.h6.err > 0 and (m.h6X.at, m.h6X.err) == (5, 0)
    assert model_record(*by["lmsx_blen_100"]).hX.at == 0 and model_record(*by["lmsx_blen_101"]).hX.at == 5
    assert [model_record(*by["lmsx_at%d_clean" % at]).hX.at for at in (5, 40, 45)] == [5, 40, 45]
    assert [model_record(*by["lmsx_at%d_sync_damaged" % at]).hX.at for at in (5, 40, 45)] == [0, 0, 0]
    assert rs_bytes(model_record(*by["not_decoded"])) == bytes(120) == rs_bytes(model_record(*by["blen_0"]))
