"""Shared by tests/test_mrz_hits_emu.py and tests/test_gpu_mrz_hits.py: constructed MRZ header hits for the per-hit device decoder of generic engines
(radiosonde_auto_rx_amd/csrc/sonde_mrz_hits_dev.h), the emulator binding (tests/emu/mrz_hits_emu.cpp), and both ways from a hit to text — the arbiter
sonde_mrz_dec_frame on the soft bits (FamilyDecoder.hit) and sonde_mrz_dec_decoded on the device's record (FamilyDecoder.decoded), each through a decoder object
that has seen the same history, since the frame length a hit is read with (386 or 362 soft bits) depends on the verdicts before it.

A hit is (name, soft values as the engine stores them, header score mv); a sequence is (name, --ofs, hits) and goes through one decoder in order.  A soft value
below zero is a 1 (sonde_mrz_dec_frame: bit = !(s >= 0)), so frame bit b is stored as 1 - 2 b.  Frame byte k of tools/synth.mrz_frame lies at frame bit ofs + 8 k
from the header's first bit; the 22 header bits are not part of a hit, and what a frame does not cover up to bit 408 is the `tail`."""
import ctypes as C
import os
import subprocess

import numpy as np

import mrz_softin_cases as M
from tools import synth
from radiosonde_auto_rx_amd.family import FAMILY, FamilyDecoder, FamilyHit, family_hit_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_SRC = os.path.join(EMU_DIR, "mrz_hits_emu.cpp")
EMU_SO = os.path.join(EMU_DIR, "libmrz_hits_emu.so")
REPLAY_SRC = os.path.join(EMU_DIR, "mrz_hits_replay.cpp")
DEPS = [EMU_SRC, os.path.join(EMU_DIR, "wave_emu.h"), os.path.join(ROOT, "include", "sonde_hip.h")] + \
       [os.path.join(CSRC, h) for h in ("sonde_mrz_hits_dev.h", "sonde_family_hits_dev.h", "sonde_softin_mrz_dev.h", "sonde_softin_meisei_dev.h",
                                        "sonde_softin_imet54_dev.h", "sonde_softin_mts01_dev.h", "sonde_softin_rs92_dev.h", "sonde_softin_wave_dev.h", "sonde_rs_dev.h")]
KIND = 31                                                    # SONDE_MRZ
NB = FAMILY["MRZ"]["generic"]["nbits"]                       # 386
HDRBITS, LEN_ECEF, LEN_LATLON = 22, 408, 384
SHORT = (0, 361, 362, 385)
# the decoder's options a text is compared under: the `-r -v` style and the receivers' JSON form (FamilyDecoder starts from FAMILY["MRZ"]["kw"])
RAW = dict(raw=1, verbose=1, json=0, ptu=0, uniq=0)
JSON = dict(FAMILY["MRZ"]["kw"], verbose=1)


def dec_opts(opts, ofs):
    kw = dict(opts, version="test", freq_khz=403000)
    if ofs != 8:
        kw.update(bits_ofs=ofs, bits_ofs_given=1)
    return kw


def load_emu():
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in DEPS):
        tmp = EMU_SO + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", tmp, EMU_SRC])
        os.replace(tmp, EMU_SO)
    L = C.CDLL(EMU_SO)
    L.emu_mrz_hits_run.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_uint, C.c_uint, C.c_int, C.POINTER(FamilyHit), C.POINTER(C.c_uint)]
    return L


def rec_key(r):
    """every field of a record (a FamilyHit or its dict), mv by its bits"""
    d = r if isinstance(r, dict) else family_hit_dict(r)
    return (d["channel"], d["kind"], d["nbits"], d["decoded"], d["mv_pos"], np.float32(d["mv"]).tobytes(), tuple(d["v"]), bytes(d["aux"]), bytes(d["data"]))


def emu_run(E, ofs, softs, mvs=None, *, grid=1, max_frames=None, start=0, done0=None):
    """the hits (one per counter value start, start + 1, ..) through the emulated launch -> (dicts in counter order, {done, ticket} after).  max_frames < len(softs):
    the ring wraps and only the last max_frames hits are in it, as after an overflow.  The output is 0xEE beforehand: a byte nothing wrote shows."""
    n = len(softs)
    mf = max_frames or n
    soft = np.zeros((mf, NB), np.float32)
    nbits, mv = np.zeros(mf, np.int32), np.zeros(mf, np.float32)
    for i, s in enumerate(softs):                                # a later hit overwrites the slot of an earlier one
        slot = (start + i) % mf
        soft[slot] = 0
        soft[slot, :len(s)] = s
        nbits[slot] = len(s)
        mv[slot] = 0.0 if mvs is None else mvs[i]
    out = (FamilyHit * mf)()
    C.memset(out, 0xEE, C.sizeof(out))
    done = (C.c_uint * 2)(start if done0 is None else done0, 0)
    rc = E.emu_mrz_hits_run(int(ofs), soft.ctypes.data, NB, nbits.ctypes.data, mv.ctypes.data, mf, start, start + n, grid, out, done)
    assert rc == 0, rc
    first = max(start, start + n - mf)
    return [family_hit_dict(out[c % mf]) for c in range(first, start + n)], (done[0], done[1])


def split16(x):
    """(value at 408 bits, value at 384 bits) of v[3] / v[4]"""
    return x & 0xFFFF, (x >> 16) & 0xFFFF


# ---------------------------------------------------------------- hit -> text, both ways, and the decoder's length after every hit
def text_by_frame(hits, opts, ofs=8):
    """the arbiter: sonde_mrz_dec_frame on the soft bits of every hit in turn, one decoder object -> [(text, sonde_mrz_dec_frame_bits after the hit)]"""
    from radiosonde_auto_rx_amd.engine import lib
    d = FamilyDecoder("MRZ", **dec_opts(opts, ofs))
    out = []
    for _, s, mv in hits:
        t = d.hit(dict(soft=np.asarray(s, np.float32), mv=float(mv), mv_pos=0))
        out.append((t, lib().sonde_mrz_dec_frame_bits(d._h)))
    d.close()
    return out


def text_by_record(hits, recs, opts, ofs=8):
    """the device's way: FamilyDecoder.decoded on every record in turn, one decoder object; an undecoded record carries its soft bits as fetch_family gives them
    -> [(text, sonde_mrz_dec_frame_bits after the hit, the frame bits the decoder stood at BEFORE it)]"""
    from radiosonde_auto_rx_amd.engine import lib
    d = FamilyDecoder("MRZ", **dec_opts(opts, ofs))
    out = []
    for (_, s, mv), r in zip(hits, recs):
        r = dict(r)
        if not r["decoded"]:
            r["soft"] = np.asarray(s, np.float32)
            r["mv"] = float(mv)
        before = lib().sonde_mrz_dec_frame_bits(d._h) + HDRBITS
        t = d.decoded(r)
        out.append((t, lib().sonde_mrz_dec_frame_bits(d._h), before))
    d.close()
    return out


# ---------------------------------------------------------------- the constructed hits
def hit_soft(frame, ofs=8, tail=None):
    """386 soft values: the frame's bytes at frame bit ofs + 8 k (what falls on the header bits or behind bit 408 is dropped), `tail` (386 values, default +1 = a
    0 bit) wherever the frame does not reach"""
    s = np.ones(NB, np.float32) if tail is None else np.asarray(tail, np.float32).copy()
    bits = np.unpackbits(np.frombuffer(bytes(frame), np.uint8))
    p = ofs + np.arange(len(bits))
    ok = (p >= HDRBITS) & (p < LEN_ECEF)
    s[p[ok] - HDRBITS] = 1.0 - 2.0 * bits[ok].astype(np.float32)
    return s


def hit_bits(soft):
    """the 408 frame bits the reference makes of a complete hit: the header's 22, then !(s >= 0)"""
    with np.errstate(invalid="ignore"):
        return M.HDR22 + [int(not (v >= 0)) for v in np.asarray(soft, np.float32)]


def model(soft, ofs):
    """what a record of a complete hit must say, from the soft values alone: (data[:52], v[0..5])"""
    bits = hit_bits(soft)
    f408, _ = M.frame_bytes(bits, LEN_ECEF, ofs)
    f384, _ = M.frame_bytes(bits, LEN_LATLON, ofs)
    l8, val8, dat8, ok8 = M.verdict(f408)
    l4, val4, dat4, ok4 = M.verdict(f384)
    assert l8 == l4                                              # bytes 30 / 31 lie inside both lengths
    return M.pack(bits), [ok8, ok4, l8, val8 | val4 << 16, dat8 | dat4 << 16, ofs]


def with_crc(f, crclen):
    f = bytearray(f)
    f[3 + crclen:5 + crclen] = M.crc16rev(f[3:3 + crclen]).to_bytes(2, "little")
    return bytes(f)


_seq = {}


def sequences():
    """[(name, ofs, [(hit name, soft, mv)])].  "main" walks a decoder 408 -> 384 -> 408; "ofs0" / "ofs16" carry frames placed for those offsets."""
    if "s" in _seq:
        return _seq["s"]
    rng = np.random.default_rng(31)
    tail = lambda: rng.normal(0.0, 1.0, NB).astype(np.float32)      # noqa: E731
    E, LL = (lambda k: synth.mrz_frame(k)), (lambda k: synth.mrz_frame(k, latlon=True))      # noqa: E731

    def flipped(s, frame_bit):
        s = s.copy(); s[frame_bit - HDRBITS] *= -1
        return s

    def zeroed(s, value):
        """`value` (+0.0 / -0.0) on a soft value that is a 1 (negative) in the payload: both are read as a 0, so the frame changes"""
        s = s.copy()
        at = 8 + 8 * 10 + int(np.flatnonzero(s[8 + 8 * 10 - HDRBITS:] < 0)[0])
        s[at - HDRBITS] = value
        return s

    fr = bytearray(E(3)); fr[30:32] = b"\xff\xfe"
    ff_fe = hit_soft(with_crc(fr, 45))                           # an ECEF frame one bit away from the lat / lon mark, its CRC good
    main = [
        ("ecef_clean", hit_soft(E(0)), 0.93),                                     # at 408: [OK]
        ("ecef_payload_flip", flipped(hit_soft(E(1)), 8 + 8 * 12 + 3), 0.9),      # [NO] under both lengths
        ("ecef_neg_zero", zeroed(hit_soft(E(2)), -0.0), 0.9),
        ("ecef_pos_zero", zeroed(hit_soft(E(2)), 0.0), 0.9),
        ("ecef_zero_on_a_zero", np.where(hit_soft(E(2)) > 0, np.float32(0.0), hit_soft(E(2))).astype(np.float32), 0.9),      # every 0 bit as +0.0: still [OK]
        ("ecef_ff_fe", ff_fe, 0.9),                                               # crclen 45, [OK]
        ("ecef_into_ffff", flipped(ff_fe, 8 + 8 * 31 + 7), 0.9),                  # bytes 30 / 31 become FF FF: crclen 42
        ("latlon_at_408", hit_soft(LL(4), tail=tail()), 0.91),                    # [OK] at 408 bits with 24 random values behind: the decoder goes to 384
        ("latlon_at_384", hit_soft(LL(5), tail=tail()), 0.92),                    # read at 362 bits: v[1]
        ("ecef_at_384", hit_soft(E(6)), 0.9),                                     # v[0] = 1, v[1] = 0: the decoder reads it cut short, [NO]
        ("latlon_payload_flip", flipped(hit_soft(LL(7), tail=tail()), 8 + 8 * 9 + 1), 0.9),
        ("latlon_out_of_ffff", flipped(hit_soft(LL(8), tail=tail()), 8 + 8 * 30 + 4), 0.9),      # crclen 45
        ("noise", tail(), 0.77),
        ("nan", np.where(np.arange(NB) % 50 == 7, np.float32(np.nan), hit_soft(LL(9))).astype(np.float32), 0.9),      # !(NaN >= 0): a 1
    ]
    main += [("short_%d" % n, hit_soft(LL(10), tail=tail())[:n].copy(), 0.9) for n in SHORT]      # end of input: left to the host, also 362 .. 385
    main += [
        ("latlon_again", hit_soft(LL(11), tail=tail()), 0.9),
        ("crafted_back_to_408", hit_soft(M.crafted_frame(12)), 0.9),              # passes as ECEF at 384 bits: v[1] = 1 with crclen 45
        ("ecef_at_408_again", hit_soft(E(13)), 0.9),
    ]
    # --ofs 0: frame byte k at frame bit 8 k, i.e. the frame sent eight bits early (bytes 0 .. 2 fall on the header and are not checked)
    ofs0 = [("ecef", hit_soft(E(0), 0, tail()), 0.9), ("latlon", hit_soft(LL(1), 0, tail()), 0.9), ("latlon_at_384", hit_soft(LL(2), 0, tail()), 0.9),
            ("ecef_at_384", hit_soft(E(3), 0, tail()), 0.9), ("flip", flipped(hit_soft(LL(4), 0, tail()), 8 * 20), 0.9), ("natural_ecef", hit_soft(E(5)), 0.9)]
    # --ofs 16: eight bits late; the ECEF frame's CRC word then ends behind bit 408 and cannot pass, the lat / lon frame passes at 408 and not at 384
    ofs16 = [("latlon", hit_soft(LL(0), 16, tail()), 0.9), ("latlon_at_384", hit_soft(LL(1), 16, tail()), 0.9), ("ecef", hit_soft(E(2), 16, tail()), 0.9),
             ("natural_latlon", hit_soft(LL(3), tail=tail()), 0.9), ("short", hit_soft(LL(4), 16)[:385].copy(), 0.9)]
    _seq["s"] = [("main", 8, main), ("ofs0", 0, ofs0), ("ofs16", 16, ofs16)]
    return _seq["s"]


def all_hits():
    """the --ofs 8 hits, for launches where the history does not matter"""
    return sequences()[0][2]
