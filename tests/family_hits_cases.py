"""Shared by tests/test_family_hits_emu.py and tests/test_gpu_family_hits.py: constructed header hits of the four kinds a generic engine decodes on the device
(radiosonde_auto_rx_amd/csrc/sonde_family_hits_dev.h), the emulator binding (tests/emu/family_hits_emu.cpp), and both ways from a hit to text — the arbiter
sonde_<kind>_dec_frame on the soft bits, and sonde_<kind>_dec_decoded / sonde_rs92_dec_corrected on the device's record (FamilyDecoder.hit / .decoded).

A hit is (name, soft bits as the engine stores them, header score mv, ecc).  The frame builders are those of the soft-bit consumers' case modules; what a case is
about is asserted from the emulator's record in tests/test_family_hits_emu.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import imet54_softin_cases as I
import meisei_softin_cases as ME
import mts01_softin_cases as MT
import rs92_softin_cases as RS
from radiosonde_auto_rx_amd.family import DEVICE_KINDS, FAMILY, FamilyDecoder, FamilyHit, family_hit_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_SRC = os.path.join(EMU_DIR, "family_hits_emu.cpp")
EMU_SO = os.path.join(EMU_DIR, "libfamily_hits_emu.so")
REPLAY_SRC = os.path.join(EMU_DIR, "family_hits_replay.cpp")
DEPS = [EMU_SRC, os.path.join(EMU_DIR, "wave_emu.h"), os.path.join(ROOT, "include", "sonde_hip.h")] + \
       [os.path.join(CSRC, h) for h in ("sonde_family_hits_dev.h", "sonde_softin_meisei_dev.h", "sonde_softin_imet54_dev.h", "sonde_softin_mts01_dev.h",
                                        "sonde_softin_rs92_dev.h", "sonde_softin_wave_dev.h", "sonde_rs_dev.h")]
KINDS = list(DEVICE_KINDS)                                   # FAMILY keys: MEISEI, IMET5, MTS01, RS92
NB = {k: FAMILY[k]["generic"]["nbits"] for k in KINDS}
# the decoders' options a text is compared under: the `-r -v` style and the receivers' JSON form (FAMILY[kind]["kw"])
# (FamilyDecoder starts from FAMILY[kind]["kw"]: json = 0 is said here, since --json forces --ecc in two of the decoders)
RAW = {"MEISEI": dict(raw=1, verbose=1, ecc=1, json=0, ptu=0), "IMET5": dict(raw=1, verbose=1, ecc=1, json=0, ptu=0), "MTS01": dict(raw=1, verbose=1, json=0),
       "RS92": dict(raw=1, verbose=1, ecc=2, json=0)}
JSON = {k: dict(FAMILY[k]["kw"], verbose=1) for k in KINDS}


def raw_opts(kind, ecc):
    """the `-r -v` options for hits decoded under `ecc` (MTS01 has no --ecc; RS92 always corrects)"""
    return dict(RAW[kind], ecc=int(ecc)) if kind in ("MEISEI", "IMET5") else dict(RAW[kind])


def load_emu():
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in DEPS):
        tmp = EMU_SO + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", tmp, EMU_SRC])
        os.replace(tmp, EMU_SO)
    L = C.CDLL(EMU_SO)
    L.emu_family_run.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_uint, C.c_uint, C.c_int, C.POINTER(FamilyHit),
                                 C.POINTER(C.c_uint)]
    return L


def rec_key(r):
    """every field of a record (a FamilyHit or its dict), mv by its bits"""
    d = r if isinstance(r, dict) else family_hit_dict(r)
    return (d["channel"], d["kind"], d["nbits"], d["decoded"], d["mv_pos"], np.float32(d["mv"]).tobytes(), tuple(d["v"]), bytes(d["aux"]), bytes(d["data"]))


def emu_run(E, kind, ecc, softs, mvs=None, *, grid=1, max_frames=None, start=0, done0=None):
    """the hits (one per counter value start, start + 1, ..) through the emulated launch -> (dicts in counter order, {done, ticket} after).  max_frames < len(softs):
    the ring wraps and only the last max_frames hits are in it, as after an overflow."""
    n = len(softs)
    mf = max_frames or n
    soft = np.zeros((mf, NB[kind]), np.float32)
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
    rc = E.emu_family_run(DEVICE_KINDS[kind], int(ecc), soft.ctypes.data, NB[kind], nbits.ctypes.data, mv.ctypes.data, mf, start, start + n, grid, out, done)
    assert rc == 0, rc
    first = max(start, start + n - mf)
    return [family_hit_dict(out[c % mf]) for c in range(first, start + n)], (done[0], done[1])


# ---------------------------------------------------------------- hit -> text, both ways
def text_by_frame(kind, hits, opts):
    """the arbiter: sonde_<kind>_dec_frame on the soft bits of every hit in turn, one decoder object (FamilyDecoder.hit: the un-flip of a raw-polarity kind included)"""
    d = FamilyDecoder(kind, **_dec_kw(kind, opts))
    out = [d.hit(dict(soft=np.asarray(s, np.float32), mv=float(mv), mv_pos=0)) for _, s, mv, _ in hits]
    d.close()
    return out


def text_by_record(kind, hits, recs, opts):
    """the device's way: FamilyDecoder.decoded on every record in turn, one decoder object; an undecoded record carries its soft bits as fetch_family gives them"""
    d = FamilyDecoder(kind, **_dec_kw(kind, opts))
    out = []
    for (_, s, mv, _), r in zip(hits, recs):
        r = dict(r)
        if not r["decoded"]:
            r["soft"] = np.asarray(s, np.float32)
            r["mv"] = float(mv)
        out.append(d.decoded(r))
    d.close()
    return out


_orbits = {}


def rs92_orbits():
    import tempfile
    if "p" not in _orbits:
        _orbits["p"] = RS.rinex_file(tempfile.mkdtemp(prefix="family_hits_"))
    return _orbits["p"]


def _dec_kw(kind, opts):
    kw = dict(opts, version="test", freq_khz=403000)
    if kind == "RS92" and opts.get("json"):
        kw["ephemeris"] = rs92_orbits()
    return kw


# ---------------------------------------------------------------- the constructed hits
def _pm(bits):
    return (2.0 * np.asarray(bits, np.float64) - 1.0).astype(np.float32)


def meisei_hits(H):
    """every bch_named case (the frame's 1152 half symbols behind the header), exact zeros and -0.0 half symbols, noise, a hit one half symbol short"""
    hits = []
    for name, (bits, ecc, _) in ME.bch_named(H).items():
        hits.append((name, _pm(ME.sym_of_bits(bits)[ME.HL:]), 1.0, ecc))
    rng = np.random.default_rng(611)
    s = _pm(ME.sym_of_bits(ME.frame_bits(6))[ME.HL:])
    z = s.copy()
    at = rng.choice(len(z), 200, replace=False)
    z[at[:100]] = 0.0
    z[at[100:]] = -0.0                                          # s >= 0: both are a 1, so some pairs change their bit and the blocks see errors
    hits.append(("zeros", z, 1.0, 1))
    hits.append(("noise", rng.normal(0, 0.3, len(s)).astype(np.float32), 0.71, 1))
    hits.append(("short", s[:-1].copy(), 1.0, 1))
    hits.append(("clean_after", s.copy(), 1.0, 1))
    return hits


def imet54_hits():
    """the Hamming and check-sum frames of imet54_softin_cases (clean, a repaired codeword on either side of 88 and 104, an uncorrectable one on either side of 88,
    each check sum good alone, ecc off), zeros, noise, a hit one symbol short"""
    hits = [(name, _pm(bits), 1.0, ecc) for name, (bits, ecc) in list(I.hamming_bits().items()) + list(I.checksum_bits().items())]
    rng = np.random.default_rng(54)
    s = _pm(I.fbits(I.frame(7)))
    z = s.copy()
    at = rng.choice(len(z), 120, replace=False)
    z[at[:60]] = 0.0
    z[at[60:]] = -0.0
    hits.append(("zeros", z, 1.0, 1))
    hits.append(("noise", rng.normal(0, 0.3, len(s)).astype(np.float32), 0.72, 1))
    hits.append(("short", s[:-1].copy(), 1.0, 1))
    hits.append(("clean_after", s.copy(), 1.0, 1))
    return hits


def mts01_hits():
    """CRC good and bad, a header of negative score (the engine stored the bits flipped: they are flipped back), zeros, noise, a hit one bit short"""
    rng = np.random.default_rng(71)
    good = [_pm(MT.fbits(k)) for k in range(3)]
    bad = good[1].copy(); bad[8 * 40 + 3] *= -1
    badcrc = good[2].copy(); badcrc[8 * 129 + 1] *= -1
    z = good[0].copy()
    at = rng.choice(len(z), 90, replace=False)
    z[at[:45]] = 0.0
    z[at[45:]] = -0.0
    hits = [("good", good[0], 0.93, 1), ("data_flip", bad, 0.9, 1), ("crc_flip", badcrc, 0.9, 1),
            ("negative_mv", -good[1], -0.91, 1),                # what the engine stores for an inverted signal: un-flipped, the CRC is good
            ("negative_mv_zeros", -z, -0.9, 1), ("zeros", z, 0.9, 1),
            ("positive_mv_inverted_bits", -good[2], 0.9, 1),    # no un-flip: the complement, CRC bad
            ("noise", rng.normal(0, 0.3, len(z)).astype(np.float32), 0.77, 1), ("short", good[0][:-1].copy(), 0.9, 1), ("good_after", good[2], 0.9, 1)]
    return hits


def rs92_bits(frame240):
    """the 2340 bits of a frame behind its 6 header bytes: 8N1, start 0, LSB first, stop 1"""
    by = np.frombuffer(bytes(frame240), np.uint8)[6:]
    bits = np.unpackbits(by[:, None], axis=1, bitorder="little")
    return np.concatenate([np.zeros((len(by), 1), np.uint8), bits, np.ones((len(by), 1), np.uint8)], axis=1).ravel()


def rs92_hits():
    """0, 1, 12 and 13 damaged bytes (12 is RS(255,231)'s limit), damage in the 24 parity bytes, damaged start / stop bits (not looked at), zeros, noise, short"""
    rng = np.random.default_rng(92)
    fr = RS.frames()

    def damaged(k, byte_idx):
        f = bytearray(fr[k])
        for b in byte_idx:
            f[b] ^= int(rng.integers(1, 256))
        return _pm(rs92_bits(f))
    clean = _pm(rs92_bits(fr[0]))
    startstop = _pm(rs92_bits(fr[3])); startstop[0::10] = 1.0; startstop[9::10] = -1.0
    z = clean.copy()
    at = rng.choice(len(z), 150, replace=False)
    z[at[:75]] = 0.0
    z[at[75:]] = -0.0
    msg = lambda n: [int(x) for x in rng.choice(np.arange(6, 216), n, replace=False)]       # noqa: E731
    return [("clean", clean, 1.0, 1), ("one_byte", damaged(1, msg(1)), 1.0, 1), ("twelve_bytes", damaged(2, msg(12)), 1.0, 1),
            ("thirteen_bytes", damaged(3, msg(13)), 1.0, 1), ("parity_bytes", damaged(4, [216, 220, 239]), 1.0, 1),
            ("parity_and_message", damaged(5, msg(6) + [217, 218, 230, 231, 238, 239]), 1.0, 1), ("start_stop_bits", startstop, 1.0, 1), ("zeros", z, 1.0, 1),
            ("noise", rng.normal(0, 0.3, len(z)).astype(np.float32), 0.7, 1), ("short", clean[:-1].copy(), 1.0, 1), ("clean_after", _pm(rs92_bits(fr[6])), 1.0, 1)]


_hits = {}


def hits(kind):
    if kind not in _hits:
        _hits[kind] = {"MEISEI": lambda: meisei_hits(ME.load_host()), "IMET5": imet54_hits, "MTS01": mts01_hits, "RS92": rs92_hits}[kind]()
    return _hits[kind]


def by_ecc(kind):
    """the kind's hits grouped by the --ecc they are decoded under (one launch each): [(ecc, [hit, ..])]"""
    hs = hits(kind)
    return [(e, [h for h in hs if h[3] == e]) for e in sorted({h[3] for h in hs}, reverse=True)]
