"""Shared by tests/test_lms6_hits_emu.py and tests/test_gpu_lms6_hits.py: constructed LMS6 / LMS-X header hits for the per-hit device decoder of generic engines
(radiosonde_auto_rx_amd/csrc/sonde_lms6_hits_dev.h), the emulator binding (tests/emu/lms6_hits_emu.cpp), and both ways from a hit to text — the arbiter
sonde_lms6_dec_block on the soft bits (FamilyDecoder.hit) and sonde_lms6_dec_block_bytes on the device's record (FamilyDecoder.decoded), each through a decoder
object that has seen the same history, since the type in effect (and with it the block length) depends on the blocks before.

A hit is (name, soft values as the engine stores them, header score mv).  The engine stores a hit in the polarity in effect: the raw values negated when mv < 0,
which FamilyDecoder.hit and the device undo.  The model of a record is tests/lms6_vit_model.decode_block(block_sb(raw values, mv, vit)): plain numpy, pinned to
the reference by tests/test_softin_lms6_emu.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import lms6_vit_model as V
from tools import synth
from radiosonde_auto_rx_amd.family import FAMILY, FamilyDecoder, Lms6Hit, lms6_hit_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_SRC = os.path.join(EMU_DIR, "lms6_hits_emu.cpp")
EMU_SO = os.path.join(EMU_DIR, "liblms6_hits_emu.so")
REPLAY_SRC = os.path.join(EMU_DIR, "lms6_hits_replay.cpp")
DEPS = [EMU_SRC, os.path.join(EMU_DIR, "wave_emu.h"), os.path.join(ROOT, "include", "sonde_hip.h")] + \
       [os.path.join(CSRC, h) for h in ("sonde_lms6_hits_dev.h", "sonde_vit_dev.h", "sonde_softhdr_dev.h", "sonde_family_hits_dev.h", "sonde_softin_meisei_dev.h",
                                        "sonde_softin_imet54_dev.h", "sonde_softin_mts01_dev.h", "sonde_softin_rs92_dev.h", "sonde_softin_wave_dev.h", "sonde_rs_dev.h")]
KIND = 6                                                     # SONDE_LMS6
NB6, NBX = FAMILY["LMS6"]["generic"]["nbits"], FAMILY["LMSX"]["generic"]["nbits"]      # 4096, 4720
BLK6, BLKX = 260 * 16, 300 * 16                              # on-air bits from one block's start to the next
BB_LEN = 308
IF_SR = 48000
# the decoder's options a text is compared under: `-r` with --vit, and the receivers' JSON form (FamilyDecoder starts from FAMILY["LMS6"]["kw"]: --vit2)
RAW = dict(raw=1, ecc=1, vit=1, json=0)
JSON = dict(FAMILY["LMS6"]["kw"])
OPT_VIT = {"raw": (RAW, 1), "json": (JSON, 2)}


def load_emu():
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in DEPS):
        tmp = EMU_SO + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", tmp, EMU_SRC])
        os.replace(tmp, EMU_SO)
    L = C.CDLL(EMU_SO)
    L.emu_lms6_hits_run.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_uint, C.c_uint, C.c_int, C.POINTER(Lms6Hit),
                                    C.POINTER(C.c_uint)]
    return L


def rec_key(r):
    """every field of a record (an Lms6Hit or its dict), mv by its bits"""
    d = r if isinstance(r, dict) else lms6_hit_dict(r)
    return (d["channel"], d["kind"], d["nbits"], d["decoded"], d["mv_pos"], np.float32(d["mv"]).tobytes(), d["len"], d["blen"], d["err"], d["vit"], bytes(d["bytes"]))


def emu_run(E, vit, nb, softs, mvs, *, grid=1, max_frames=None, start=0, done0=None, fill=0xEE):
    """the hits (one per counter value start, start + 1, ..) through the emulated launch -> (dicts in counter order, {done, ticket} after).  max_frames < len(softs):
    the ring wraps and only the last max_frames hits are in it, as after an overflow.  The output is `fill` beforehand: a byte nothing wrote shows."""
    n = len(softs)
    mf = max_frames or n
    soft = np.zeros((mf, nb), np.float32)
    nbits, mv = np.zeros(mf, np.int32), np.zeros(mf, np.float32)
    for i, s in enumerate(softs):                                # a later hit overwrites the slot of an earlier one
        slot = (start + i) % mf
        soft[slot] = 0
        soft[slot, :len(s)] = s
        nbits[slot] = len(s)
        mv[slot] = mvs[i]
    out = (Lms6Hit * mf)()
    C.memset(out, fill, C.sizeof(out))
    done = (C.c_uint * 2)(start if done0 is None else done0, 0)
    rc = E.emu_lms6_hits_run(int(vit), int(nb), soft.ctypes.data, nb, nbits.ctypes.data, mv.ctypes.data, mf, start, start + n, grid, out, done)
    assert rc == 0, rc
    first = max(start, start + n - mf)
    return [lms6_hit_dict(out[c % mf]) for c in range(first, start + n)], (done[0], done[1])


def model(soft, mv, vit):
    """what a record of a complete hit must say, from the stored soft values and the header score alone: (bytes[308], blen, err, len)"""
    s = np.asarray(soft, np.float32)
    raw = -s if mv < 0 else s                                    # FamilyDecoder.hit, pol = "raw"
    by, blen, err = V.decode_block(V.block_sb(raw, mv, vit))
    return bytes(by), int(blen), int(err), V.BLOCKSTART + len(s)


# ---------------------------------------------------------------- the constructed hits
def onair_soft(n_blocks, lmsx):
    """+-1 of n_blocks consecutive on-air blocks and two more, so that a hit cut behind any of the first n_blocks headers is whole"""
    return (2.0 * synth.lms6_onair_bits(n_blocks + 2, lmsx).astype(np.float64) - 1.0).astype(np.float32)


def cut(stream, k, blk, nb):
    """the nb raw values behind the header of block k: the header's 64 bits are positions 16 .. 79 of a block"""
    return stream[blk * k + V.BLOCKSTART:blk * k + V.BLOCKSTART + nb].copy()


_hits = {}


def hits(lmsx=False):
    """[(name, stored soft values, mv)] for an engine of the LMS6 (4096 bits) or the LMS-X description (4720 bits)"""
    if lmsx in _hits:
        return _hits[lmsx]
    nb, blk = (NBX, BLKX) if lmsx else (NB6, BLK6)
    rng = np.random.default_rng(600 + int(lmsx))
    s = onair_soft(6, lmsx)
    noisy = lambda k, sigma: (cut(s, k, blk, nb) + rng.normal(0.0, sigma, nb)).astype(np.float32)      # noqa: E731
    b07, b09 = noisy(1, 0.7), noisy(2, 0.9)
    er = noisy(3, 0.75)
    er[rng.random(nb) < 0.15] = 0.0
    out = [
        ("clean", cut(s, 0, blk, nb), 0.97),
        ("sigma07", b07, 0.81),
        ("sigma09", b09, 0.74),
        # the same signal received inverted: the raw values negated, the score negative, the phase of the alternation shifted; the engine stores them flipped back
        ("sigma09_inverted", b09.copy(), -0.74),
        ("clean_inverted", cut(s, 0, blk, nb), -0.97),
        # a negative score in front of values that were not inverted: every raw bit wrong
        ("sigma07_wrong_sign", (-b07).astype(np.float32), -0.81),
        ("mv_zero", cut(s, 4, blk, nb), 0.0),                                       # bc = 1, no flip
        ("all_zero", np.zeros(nb, np.float32), 0.9),                               # ties at every step: `<=` keeps the first candidate, the first minimum
        ("all_neg_zero", np.full(nb, -0.0, np.float32), 0.9),
        ("all_neg_zero_inverted", np.full(nb, -0.0, np.float32), -0.9),
        ("erased", er, 0.78),
        ("noise", rng.normal(0.0, 1.0, nb).astype(np.float32), 0.71),              # deconv stops early: err != 0, a short blen
        ("short", noisy(5, 0.3)[:nb - 1].copy(), 0.9),                             # end of input: left to the host
    ]
    _hits[lmsx] = out
    return out


_recs = {}


def records(E, lmsx, vit):
    """the hit list through one emulated launch (three workgroups) -> records in hit order, computed once"""
    key = (lmsx, vit)
    if key not in _recs:
        hs = hits(lmsx)
        got, done = emu_run(E, vit, NBX if lmsx else NB6, [h[1] for h in hs], [h[2] for h in hs], grid=3)
        assert done == (len(hs), 0)
        _recs[key] = got
    return _recs[key]


# ---------------------------------------------------------------- sequences of blocks through one decoder
def sequence(kind):
    """[(name, stored soft values, mv, mv_pos)] in the order a channel's decoder sees them; the soft values are as long as the engine's description in use at that
    point slices them.  "lms6" / "lmsx": clean and noisy blocks of one type.  "switch": an LMS6 that turns out to be LMS-X and later LMS6 again, with the engine
    following one block late, as the receivers do — an LMS-X decoder still on the LMS6 engine (4096-bit records, the device's bytes count), an LMS6 decoder still
    on the LMS-X engine (4720-bit records, decoded from their soft bits)."""
    rng = np.random.default_rng(77)
    s6, sx = onair_soft(12, False), onair_soft(12, True)
    d6, dx = BLK6 * IF_SR // 4800, int(round(BLKX * IF_SR / 4797.8))               # header to header in IF samples
    out, pos = [], [1000]

    def add(name, lmsx_content, k, nb, sigma=0.0, mv=0.93):
        v = cut(sx if lmsx_content else s6, k, BLKX if lmsx_content else BLK6, nb)
        if sigma:
            v = (v + rng.normal(0.0, sigma, nb)).astype(np.float32)
        out.append((name, v, mv, pos[0]))                        # (mv < 0: received inverted and stored flipped back — the same values)
        pos[0] += dx if lmsx_content else d6

    if kind == "lms6":
        for k in range(4):
            add("lms6_%d" % k, False, k, NB6, sigma=(0.0, 0.0, 0.6, 0.0)[k], mv=(0.93, -0.9, 0.8, 0.9)[k])
        out.append(("noise", rng.normal(0.0, 1.0, NB6).astype(np.float32), 0.71, pos[0]))
        add("lms6_5", False, 5, NB6)
    elif kind == "lmsx":
        for k in range(4):
            add("lmsx_%d" % k, True, k, NBX, sigma=(0.0, 0.0, 0.6, 0.0)[k], mv=(0.93, -0.9, 0.8, 0.9)[k])
        out.append(("noise", rng.normal(0.0, 1.0, NBX).astype(np.float32), 0.71, pos[0]))
        add("lmsx_5", True, 5, NBX)
    else:
        add("lms6_0", False, 0, NB6); add("lms6_1", False, 1, NB6)
        add("x_on_lms6_engine_found", True, 2, NB6)              # the decoder (LMS6, 4096) finds the LMS-X sync in the first 4096 bits and changes
        add("x_on_lms6_engine_after", True, 3, NB6)              # the decoder reads 4720 now, the record has 4096: its bytes are what hit() gives
        add("x_0", True, 4, NBX); add("x_1", True, 5, NBX, sigma=0.5)
        add("lms6_on_x_engine_found", False, 6, NBX)             # the decoder (LMS-X, 4720) finds the LMS6 sync and changes back
        add("lms6_on_x_engine_after", False, 7, NBX)             # the decoder reads 4096 now, the record has 4720: decoded from the soft bits
        add("lms6_2", False, 8, NB6); add("lms6_3", False, 9, NB6)
    return out


def dec_opts(opts, typ):
    return dict(opts, typ=typ, version="test", freq_khz=403000)


def text_by_hit(seq, opts, typ):
    """the arbiter: sonde_lms6_dec_block on the soft bits of every hit in turn, one decoder object -> [(text, lms_type after the hit)]"""
    d = FamilyDecoder("LMS6", **dec_opts(opts, typ))
    out = []
    for _, s, mv, pos in seq:
        t = d.hit(dict(soft=np.asarray(s, np.float32), mv=float(mv), mv_pos=pos), IF_SR)
        out.append((t, d.lms_type()))
    d.close()
    return out


def text_by_record(seq, recs, opts, typ):
    """the device's way: FamilyDecoder.decoded on every record in turn, one decoder object.  A record carries its soft bits where Engine.fetch_family would have
    given them: when it was not decoded, and when it is longer than the decoder reads at that point (need_soft) -> [(text, lms_type after, took the soft bits)]"""
    d = FamilyDecoder("LMS6", **dec_opts(opts, typ))
    out = []
    for (_, s, mv, pos), r in zip(seq, recs):
        r = dict(r, mv_pos=pos)
        soft = not r["decoded"] or r["nbits"] > d.lms_block_bits()
        if soft:
            r["soft"] = np.asarray(s, np.float32)
        t = d.decoded(r, IF_SR)
        out.append((t, d.lms_type(), soft))
    d.close()
    return out


def seq_records(E, seq, vit):
    """the emulator's records of a sequence, in order: one launch per block length"""
    recs = [None] * len(seq)
    for nb in (NB6, NBX):
        idx = [i for i, h in enumerate(seq) if len(h[1]) == nb]
        if idx:
            got, _ = emu_run(E, vit, nb, [seq[i][1] for i in idx], [seq[i][2] for i in idx], grid=len(idx))
            for i, r in zip(idx, got):
                recs[i] = r
    return recs
