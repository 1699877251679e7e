"""Streams and arbiters shared by tests/test_softin_meisei_emu.py (the device Meisei soft-bit consumer under the CPU wave emulator), tests/test_meisei_decoded.py and
tests/test_gpu_softin_meisei.py (the same source as k_softin_meisei on the device): half-symbol streams built from tools/synth.py frames, the host tier
sonde_meisei_dec_push_soft (pinned to the compiled reference by tests/test_meisei_native.py) as arbiter, and the emulator driver tests/emu/softin_meisei_emu.cpp.

The arbiter prints text only.  With `-r --ecc -v` a frame is, per subframe, the 24 header bits and the 12 words of 16 bits as hex and `#......#` with the six block
verdicts.  The parity and check bits are not printed, so the 600 bits the records are compared with come from model_frame(): the biphase-S rule on the 1152 half
symbols behind the arbiter's hit and, per block, the host codec sonde_ecc_decode_bch_gf2t2 (pinned to the reference by tests/test_ecc_codes.py) with the padding
and word-parity rule; host_frames() asserts for every frame that the line made from the model IS the arbiter's line.  Fed a half symbol at a time, the arbiter
prints a frame at the frame's last half symbol: the header matched 1152 half symbols before that.  The arbiter does not print mv: the expected score is
ref_score() — the reference's expression (float products, double sums in order, sum / sqrt(normx * 48), rounded to float) on the 48 half symbols the reference's
ring holds at the hit, i.e. the last 48 of the stream with the frame bodies the arbiter found taken out (ring_at)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from tools import synth
from radiosonde_auto_rx_amd.family import MeiseiOpts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_SRC = os.path.join(EMU_DIR, "softin_meisei_emu.cpp")
EMU_SO = os.path.join(EMU_DIR, "libsoftin_meisei_emu.so")
DEPS = [EMU_SRC, os.path.join(EMU_DIR, "wave_emu.h"), os.path.join(CSRC, "sonde_softin_meisei_dev.h"), os.path.join(CSRC, "sonde_softin_wave_dev.h"),
        os.path.join(CSRC, "sonde_rs_dev.h"), os.path.join(ROOT, "include", "sonde_hip.h")]
REF = os.path.join(ROOT, "oracle", "_ref", "meisei100mod")
HEADER = "101010101011010100101011001101001100101011001101"      # the 48 header half symbols `meisei100mod` searches for: 0x049DCE in biphase-S
HDR = np.array([int(c) for c in HEADER], np.uint8)
HDR24 = [int(c) for c in "000001001001110111001110"]
HL = 48
NSYM = 1152                                                 # half symbols of a frame behind the header
FRAME = HL + NSYM                                           # 1200: the spacing of back-to-back frames
STAGE_MAX = 12288                                           # M10_STAGE_MAX of sonde_softin_wave_dev.h
CUTS = [2400, 1000, 251, 1, 2, 47, 48, 49, 63, 64, 65]
F08 = np.float32(0.8)


class Rec(C.Structure):
    """SoftinMeiseiRec (csrc/sonde_softin_meisei_dev.h)"""
    _fields_ = [("channel", C.c_int32), ("mv", C.c_float), ("hdr_bit", C.c_uint64), ("block_err", C.c_uint8 * 12), ("bits", C.c_uint8 * 75), ("pad", C.c_uint8 * 1)]


class EmuState(C.Structure):
    """EmuMeiseiState (tests/emu/softin_meisei_emu.cpp)"""
    _fields_ = [("mode", C.c_int), ("done", C.c_int), ("mv", C.c_float), ("carry", C.c_float), ("bits_in", C.c_uint64), ("hdr_bit", C.c_uint64),
                ("hist", C.c_float * 48), ("w", C.c_uint32 * 19), ("pad", C.c_int)]


def load_emu(src=EMU_SRC, so=EMU_SO, deps=DEPS, flags=()):
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = so + ".%d.tmp" % os.getpid()
        # (-ffp-contract=off: the score is the reference's expression, every product and sum rounded on its own)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", *flags, "-o", tmp, src])
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.emu_meisei_run.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Rec), C.c_int, C.POINTER(C.c_int),
                                 C.POINTER(EmuState)]
    L.emu_meisei_end.argtypes = [C.c_char_p, C.c_int, C.POINTER(Rec)]
    L.emu_meisei_header_mask.restype = C.c_uint64
    return L


def load_host():
    from radiosonde_auto_rx_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    L = C.CDLL(engine.LIB_PATH)
    L.sonde_meisei_dec_create.argtypes = [C.POINTER(MeiseiOpts), C.POINTER(C.c_void_p)]
    L.sonde_meisei_dec_destroy.argtypes = [C.c_void_p]
    L.sonde_meisei_dec_push_soft.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]
    L.sonde_meisei_dec_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_char_p, C.c_size_t]
    L.sonde_meisei_dec_decoded.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]
    L.sonde_ecc_create.restype = C.c_void_p
    L.sonde_ecc_create.argtypes = [C.c_int]
    L.sonde_ecc_destroy.argtypes = [C.c_void_p]
    L.sonde_ecc_encode.argtypes = [C.c_void_p, C.c_void_p]
    L.sonde_ecc_decode_bch_gf2t2.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def host_dec(H, **kw):
    h = C.c_void_p()
    if isinstance(kw.get("version"), str):
        kw["version"] = kw["version"].encode()
    o = MeiseiOpts(**kw)
    assert H.sonde_meisei_dec_create(C.byref(o), C.byref(h)) == 0
    return h


# ---------------------------------------------------------------- the block rule on the host codec
_bch = {}


def bch(H):
    """the host's BCH(63,51) codec (SONDE_ECC_BCH64 = 3)"""
    if "c" not in _bch:
        _bch["c"] = C.c_void_p(H.sonde_ecc_create(3))
    return _bch["c"]


def block_rule(H, blk46):
    """meisei100mod.c:742-770 on one block of 46 bits with the host codec: (verdict 0 / 1 / 2 / 0xE / 0xF, the 46 bits left in the block)"""
    b = bytearray(64)
    b[0:46] = bytes(int(v) for v in blk46)[::-1]                 # cw[45 - j] = block bit j, cw[46 .. 62] = 0
    cw = (C.c_uint8 * 64).from_buffer(b)
    ep, ev = (C.c_uint8 * 4)(), (C.c_uint8 * 4)()
    e = H.sonde_ecc_decode_bch_gf2t2(bch(H), cw, ep, ev)
    if e >= 0:
        chk = any(b[46:63])
        chk = chk or b[12] != 1 ^ (sum(b[13:29]) & 1)
        chk = chk or b[29] != 1 ^ (sum(b[30:46]) & 1)
        if chk:
            e = -3
    if e >= 0:
        return e, list(b[45::-1])
    return (0xF if e == -3 else 0xE), [int(v) for v in blk46]


def encode_block(H, msg34):
    """16 + 1 + 16 + 1 message bits -> the 46 block bits (12 check bits behind them) by the host codec: block bit j = cw[45 - j]"""
    cw = (C.c_uint8 * 64)()
    for j in range(34):
        cw[45 - j] = int(msg34[j])
    assert H.sonde_ecc_encode(bch(H), cw) == 0
    return [cw[45 - j] for j in range(46)]


def biphase(sym1152):
    """bit j = 1 if half symbols 2 j and 2 j + 1 have the same hard value (s >= 0: -0.0 is a 1)"""
    hard = np.asarray(sym1152, np.float32) >= 0
    return (hard[0::2] == hard[1::2]).astype(np.uint8)


def model_frame(H, sym1152, ecc=1):
    """(600 bits behind the block loop as 75 bytes MSB first, 12 verdicts) of the 1152 half symbols behind a hit"""
    bits = HDR24 + [int(b) for b in biphase(sym1152)]
    assert len(bits) == 600
    return model_end(H, bits, ecc)


def model_end(H, bits600, ecc=1):
    bits = [int(b) for b in bits600]
    be = [0] * 12
    if ecc:
        for blk in range(12):
            at = 300 * (blk // 6) + 24 + 46 * (blk % 6)
            be[blk], bits[at:at + 46] = block_rule(H, bits[at:at + 46])
    return pack(bits), bytes(be)


def pack(bits600):
    return bytes(np.packbits(np.asarray(bits600, np.uint8)))


def unpack(bits75):
    return np.unpackbits(np.frombuffer(bytes(bits75), np.uint8))[:600]


# ---------------------------------------------------------------- records
def _g(r):
    return (lambda k: r[k]) if isinstance(r, dict) else (lambda k: getattr(r, k))


def raw_line(r, ecc=1):
    """the `-r [--ecc -v]` line of a record (a Rec, a fetch_meisei dict or a (hdr_bit, bits75, verdicts, ..) tuple)"""
    bits, be = (r[1], r[2]) if isinstance(r, tuple) else (bytes(_g(r)("bits")), bytes(_g(r)("block_err")))
    b = unpack(bits)
    val = lambda at, n: int("".join(str(int(v)) for v in b[at:at + n]), 2)       # noqa: E731
    line = ""
    for sf in range(2):
        line += "%06X " % val(300 * sf, 24)
        for j in range(6):
            line += "%04X %04X " % (val(300 * sf + 24 + 46 * j, 16), val(300 * sf + 24 + 46 * j + 17, 16))
        if ecc:
            line += "#" + "".join("%X" % e for e in be[6 * sf:6 * sf + 6]) + "#  "
    return line


def key(r):
    """(hdr_bit, the 600 bits, the 12 verdicts) of a Rec, a fetch_meisei dict or an arbiter tuple: what must agree exactly with the arbiter"""
    if isinstance(r, tuple):
        return r[:3]
    g = _g(r)
    return (g("hdr_bit"), bytes(g("bits")), bytes(g("block_err")))


def full(r):
    """everything of a Rec the emulator must reproduce under any cut, mv bit for bit"""
    return key(r) + (struct.pack("<f", r.mv),)


def mv_within_one_ulp(a, b):
    """two floats (the device's double divide and sqrt come ahead of the rounding to float: one ulp, as the M20 suite allows)"""
    ia, ib = struct.unpack("<i", struct.pack("<f", a))[0], struct.unpack("<i", struct.pack("<f", b))[0]
    return (ia < 0) == (ib < 0) and abs(ia - ib) <= 1


_arb = {}


def host_frames(H, s, softinv=False, ecc=1, cache=None):
    """the arbiter: [(hdr_bit, bits75, verdicts12, `-r` line)] of the host tier over the whole stream, a half symbol at a time (the frame is printed at its last one)"""
    if cache is not None and cache in _arb:
        return _arb[cache]
    s = np.ascontiguousarray(s, np.float32)
    h = host_dec(H, raw=1, ecc=ecc, verbose=1)
    out, buf = [], C.create_string_buffer(1024)
    base = s.ctypes.data
    sg = np.float32(-1.0 if softinv else 1.0)
    for i in range(len(s)):
        n = H.sonde_meisei_dec_push_soft(h, base + 4 * i, 1, int(softinv), 0, buf, 1024)
        assert n >= 0
        if n:
            line = buf.raw[:n].decode().rstrip("\n")
            hb = i + 1 - NSYM
            bits, be = model_frame(H, sg * s[hb:hb + NSYM], ecc)
            assert raw_line((hb, bits, be), ecc) == line, (hb, line)          # the model is the arbiter's, frame by frame
            out.append((hb, bits, be, line))
    H.sonde_meisei_dec_destroy(h)
    if cache is not None:
        _arb[cache] = out
    return out


def host_text(H, s, softinv=False, **kw):
    """what the host tier prints for the whole stream under the options kw"""
    s = np.ascontiguousarray(s, np.float32)
    h = host_dec(H, **kw)
    buf = C.create_string_buffer(1 << 20)
    n = H.sonde_meisei_dec_push_soft(h, s.ctypes.data, len(s), int(softinv), 0, buf, len(buf))
    assert n >= 0
    H.sonde_meisei_dec_destroy(h)
    return buf.raw[:n].decode()


def emu_frames(E, s, calls, softinv=False, ecc=1, cap=64):
    """the emulated consumer over the stream cut into calls (the last length repeats): Recs, frames dropped for want of room, end state"""
    s = np.ascontiguousarray(s, np.float32)
    buf = (Rec * (len(s) // NSYM + 2))()
    cl = (C.c_int * len(calls))(*calls)
    dropped, end = C.c_int(0), EmuState()
    n = E.emu_meisei_run(s.ctypes.data, len(s), cl, len(calls), int(softinv), int(ecc), cap, buf, len(buf), C.byref(dropped), C.byref(end))
    assert 0 <= n < len(buf), n
    for i in range(n):
        assert buf[i].channel == 0
    return [buf[i] for i in range(n)], dropped.value, end


def state(end):
    """the end state as far as it means anything: the pending half symbol, the bits so far and the frame position only inside a frame"""
    inside = end.mode == 1
    nb = 24 + end.done // 2
    words = [int(end.w[k]) & (0xFFFFFFFF if 32 * k + 32 <= nb else (1 << max(nb - 32 * k, 0)) - 1) for k in range(19)]
    return (end.mode, end.bits_in, [struct.pack("<f", v) for v in end.hist],
            (end.done, struct.pack("<f", end.carry) if end.done & 1 else None, words, end.hdr_bit, struct.pack("<f", end.mv)) if inside else None)


def ref_score(win):
    """corr_softhdb on 48 half symbols (demod_mod.c:1692-1735): float products, double sums in order, sum / sqrt(normx * 48.0), rounded to float"""
    win = np.asarray(win, np.float32)
    assert len(win) == HL
    sm, nx = 0.0, 0.0
    for v, b in zip(win, HDR):
        y = np.float32(1.0 if b else -1.0)
        sm += float(np.float32(y * v)); nx += float(np.float32(v * v))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(np.float64(sm) / np.sqrt(np.float64(nx) * 48.0))


def ring_at(s, hdr_bits, at, softinv=False):
    """the reference's ring when `at` half symbols have been read: the last 48 seen while searching — the stream without the frame bodies behind hdr_bits —
    oldest first, zeros where the stream has not filled it"""
    s = np.asarray(s, np.float32) * np.float32(-1.0 if softinv else 1.0)
    keep = np.ones(len(s), bool)
    for hb in hdr_bits:
        keep[hb:hb + NSYM] = False
    keep[at:] = False
    seq = np.concatenate([np.zeros(HL, np.float32), s[keep]])
    return seq[-HL:]


# ---------------------------------------------------------------- frames and streams
def fsym(k, variant="ims100", n=1):
    """the 1200 n half symbols (0 / 1) of frames k .. k + n - 1 on air, the first level low: the header is HEADER or, where a frame starts high, its inverse"""
    return synth.meisei_symbols(n, variant, k0=k)


def soft(sym, rng=None, jitter=(1.0, 1.0)):
    s = 2.0 * np.asarray(sym, np.float64) - 1.0
    if rng is not None:
        s = s * rng.uniform(jitter[0], jitter[1], len(s))
    return s.astype(np.float32)


def noise(rng, n, sigma=0.3):
    return rng.normal(0.0, sigma, n).astype(np.float32)


def sym_of_bits(bits600):
    """600 frame bits -> 1200 half symbols in biphase-S from a low level (the header comes out as HEADER)"""
    out, level = [], 0
    for b in bits600:
        level ^= 1; out.append(level)
        if not b:
            level ^= 1
        out.append(level)
    return np.array(out, np.uint8)


def frame_bits(k, variant="ims100"):
    return list(synth.meisei_frame_bits(k, variant))


def block_at(blk):
    """where block blk (0 .. 11, subframe 0 first) starts among the 600 frame bits"""
    return 300 * (blk // 6) + 24 + 46 * (blk % 6)


def bch_named(H):
    """name -> (600 frame bits, ecc, {block: verdict expected}): the named BCH cases on frame 5 (block 2 unless said otherwise); cw index p is block bit 45 - p"""
    base = frame_bits(5)
    c = {}

    def flipped(blk, cwpos):
        b = list(base)
        for p in cwpos:
            b[block_at(blk) + 45 - p] ^= 1
        return b
    c["no_error"] = (list(base), 1, {})
    for p in range(46):
        c["one_flip_%02d" % p] = (flipped(2, [p]), 1, {2: 1})
    for n_, (p, q) in enumerate([(0, 1), (3, 11), (5, 20), (12, 29), (13, 30), (28, 45), (44, 45), (0, 45)]):
        c["two_flips_%d" % n_] = (flipped(2, [p, q]), 1, {2: 2})
    # three flips: the decoder sees some other word at distance <= 2 or none: searched over triples for each outcome the rule can give
    want = {"three_pad": None, "three_parity": None, "three_accepted": None, "three_none": None}
    blk0 = base[block_at(2):block_at(2) + 46]
    for p in range(46):
        for q in range(p + 1, 46):
            for r in range(q + 1, 46):
                if all(v is not None for v in want.values()):
                    break
                t = list(blk0)
                for x in (p, q, r):
                    t[45 - x] ^= 1
                cw = (C.c_uint8 * 64)()
                for j in range(46):
                    cw[45 - j] = t[j]
                ep, ev = (C.c_uint8 * 4)(), (C.c_uint8 * 4)()
                e = H.sonde_ecc_decode_bch_gf2t2(bch(H), cw, ep, ev)
                v, _ = block_rule(H, t)
                kind = "three_none" if e < 0 else "three_pad" if any(cw[j] for j in range(46, 63)) else "three_parity" if v == 0xF else "three_accepted"
                if want[kind] is None:
                    want[kind] = ((p, q, r), v)
    for name, val in want.items():
        assert val is not None, name
        c[name] = (flipped(2, val[0]), 1, {2: val[1]})
    assert c["three_pad"][2] == {2: 0xF} and c["three_parity"][2] == {2: 0xF} and c["three_accepted"][2][2] in (1, 2) and c["three_none"][2] == {2: 0xE}
    # a valid BCH codeword with a wrong word parity bit: message bit 16 (the first word's parity) flipped and the block encoded again
    m = list(blk0[:34]); m[16] ^= 1
    b = list(base); b[block_at(2):block_at(2) + 46] = encode_block(H, m)
    c["codeword_parity1"] = (b, 1, {2: 0xF})
    m = list(blk0[:34]); m[33] ^= 1
    b = list(base); b[block_at(2):block_at(2) + 46] = encode_block(H, m)
    c["codeword_parity2"] = (b, 1, {2: 0xF})
    # S1 = 0 with S3 != 0: alpha^0 + alpha^1 + alpha^6 = 0 in GF(2^6) / 0x43 (x^6 = x + 1), alpha^0 + alpha^3 + alpha^18 = 1 + x^3 + (x^3 + x^2 + x + 1) != 0
    c["s1_zero"] = (flipped(2, [0, 1, 6]), 1, {2: 0xE})
    for blk in range(12):
        c["block_%02d" % blk] = (flipped(blk, [7, 33]), 1, {blk: 2})
    c["ecc_off"] = (flipped(2, [7]), 0, {})
    return c


def bch_messages():
    """8 messages of 16 + 1 + 16 + 1 bits with correct (odd) word parities, the all-zero and all-one words among them"""
    rng = np.random.default_rng(6351)
    words = [(0x0000, 0x0000), (0xFFFF, 0xFFFF), (0x0000, 0xFFFF), (0xA5A5, 0x0001)] + [tuple(int(v) for v in rng.integers(0, 65536, 2)) for _ in range(4)]
    out = []
    for a, b in words:
        m = []
        for w in (a, b):
            wb = [(w >> (15 - k)) & 1 for k in range(16)]
            m += wb + [1 ^ (sum(wb) & 1)]
        out.append(m)
    return out


def syndrome_blocks(H, msg34):
    """the 4096 blocks of one message: every 12-bit pattern XORed onto cw[0 .. 11] (block bits 45 .. 34) — every syndrome exactly once"""
    enc = np.array(encode_block(H, msg34), np.uint8)
    blocks = np.tile(enc, (4096, 1))
    pat = np.arange(4096)
    for p in range(12):
        blocks[:, 45 - p] ^= ((pat >> p) & 1).astype(np.uint8)
    return blocks


def sweep_frames(blocks):
    """blocks (n, 46) -> frames of 600 bits (ceil(n / 12), 600): 12 blocks a frame behind both subframe headers, the last frame filled up with its first block"""
    n = len(blocks)
    nf = (n + 11) // 12
    fr = np.zeros((nf, 600), np.uint8)
    fr[:, :24] = HDR24
    fr[:, 300:324] = [int(c) for c in "111110110110001000110000"]
    for i in range(nf * 12):
        fr[i // 12, block_at(i % 12):block_at(i % 12) + 46] = blocks[i if i < n else 12 * (i // 12)]
    return fr


# the stream cases and their options (softinv = --softinv; --ecc on).  Kept apart from the streams, which need the host library to be built: a test module must not
# load libsonde_hip.so while it is collected (tests/conftest.py: PyTorch's HIP runtime has to come first in a GPU process), so the modules parametrise over
# case_opts() and build cases() inside their tests.
STREAM_OPTS = {"clean_ims100": {}, "clean_rs11g": {}, "sigma03": {}, "back_to_back": {}, "inverted": {}, "inverted_softinv": dict(softinv=True),
               "zero_symbols": {}, "zero_symbols_neg": {}, "zero_symbols_softinv": dict(softinv=True), "zero_symbols_neg_softinv": dict(softinv=True),
               "flips_4": {}, "flips_5": {}, "edge_below": {}, "edge_above": {}, "zero_window": {}, "ring_behind_frame": {}}
BCH_STREAMS = ["no_error", "one_flip_00", "one_flip_45", "two_flips_3", "three_pad", "three_parity", "three_accepted", "three_none", "codeword_parity1", "s1_zero",
               "block_00", "block_11", "ecc_off"]


def case_opts():
    """name -> (softinv, ecc) of every case, without building a stream"""
    o = {k: (v.get("softinv", False), 1) for k, v in STREAM_OPTS.items()}
    o.update({"bch_" + k: (False, 0 if k == "ecc_off" else 1) for k in BCH_STREAMS})
    return o


FLIP4 = np.array([3, 12, 26, 37])
FLIP5 = np.array([3, 12, 26, 37, 44])


def _find_edge(H, tail):
    """amplitudes a_lo < a_hi, adjacent floats, of header half symbol 0 (a 1: +1 at unit amplitude) of a header with four flipped half symbols: the host framer
    finds the header at a_hi and not at a_lo.  The score (39 + a) / sqrt(48 (47 + a^2)) rises with a on [-1, 0] from 38 / 48 to 0.821."""
    def found(a):
        s = soft(fsym(6))
        s[FLIP4] = -s[FLIP4]
        s[0] = np.float32(a)
        h = host_dec(H, raw=1, ecc=1, verbose=1)
        buf = C.create_string_buffer(4096)
        s = np.ascontiguousarray(np.concatenate([s, tail]), np.float32)
        n = H.sonde_meisei_dec_push_soft(h, s.ctypes.data, len(s), 0, 0, buf, 4096)
        H.sonde_meisei_dec_destroy(h)
        return n > 0
    lo, hi = np.float32(-1.0), np.float32(0.0)
    assert not found(lo) and found(hi)
    while np.nextafter(lo, np.float32(2.0)) < hi:
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        if found(mid):
            hi = mid
        else:
            lo = mid
    return lo, hi


def case_streams(H):
    """name -> dict(s, softinv, ecc, n = frames the arbiter must give)"""
    c = {}
    rng = np.random.default_rng(100)
    tail = lambda n=70: noise(rng, n, 0.05)                                        # noqa: E731
    # 1. clean frames of both variants (continuous: the exact 1200 spacing, and a header in either polarity wherever a frame starts high), and sigma 0.3
    c["clean_ims100"] = dict(s=np.concatenate([tail(33), soft(fsym(0, "ims100", 3)), tail()]), n=3)
    c["clean_rs11g"] = dict(s=np.concatenate([tail(21), soft(fsym(2, "rs11g", 3)), tail()]), n=3)
    s = np.concatenate([tail(17), soft(fsym(4, "ims100", 3)), tail()])
    c["sigma03"] = dict(s=s + noise(rng, len(s), 0.3), n=3)
    # 2. back to back from the first half symbol on
    c["back_to_back"] = dict(s=np.concatenate([soft(fsym(10, "ims100", 4)), tail()]), n=4)
    # 3. polarity: the inverted stream as it is and with --softinv: mv changes sign, bits and text do not
    pol = np.concatenate([tail(33), soft(fsym(7, "rs11g", 2), rng, (0.8, 1.2)), tail(37)])
    c["inverted"] = dict(s=-pol, n=2)
    c["inverted_softinv"] = dict(s=-pol, softinv=True, n=2)
    # 4. exact zeros and -0.0 on frame half symbols (s >= 0 is true for both), under both stream polarities and with --softinv, which turns one into the other
    s = soft(fsym(9), rng, (0.8, 1.2))
    for n_, p in enumerate(range(HL + 5, FRAME, 23)):
        s[p] = np.float32(0.0) if n_ % 2 == 0 else np.float32(-0.0)
    for name, st in (("zero_symbols", s), ("zero_symbols_neg", -s)):
        full_ = np.concatenate([tail(50), st, tail()])
        c[name] = dict(s=full_, n=1)
        c[name + "_softinv"] = dict(s=full_, softinv=True, n=1)
    # 5. the threshold: 4 flipped header half symbols score 40 / 48, 5 score 38 / 48 < 0.8
    for name, idx in (("flips_4", FLIP4), ("flips_5", FLIP5)):
        s = soft(fsym(6))
        s[idx] = -s[idx]
        c[name] = dict(s=np.concatenate([tail(40), s, tail()]), n=1 if name == "flips_4" else 0)
    # ... and one half symbol's amplitude moved until the host framer changes its mind: adjacent floats on both sides of the threshold
    t = tail()
    lo, hi = _find_edge(H, t)
    for name, a in (("edge_below", lo), ("edge_above", hi)):
        s = soft(fsym(6))
        s[FLIP4] = -s[FLIP4]
        s[0] = a
        c[name] = dict(s=np.concatenate([s, t]), n=0 if name == "edge_below" else 1, amp=float(a))
    # 6. windows of exact zeros: 0 / 0 is no hit
    c["zero_window"] = dict(s=np.concatenate([np.zeros(53, np.float32), soft(fsym(14)), np.zeros(75, np.float32), soft(fsym(15)), tail()]), n=2)
    # 7. the ring behind a frame is the header it was found by: K half symbols y right behind the frame complete h1[K:] ++ y to a hit, where h1 is a header that is
    #    nearly silent wherever it disagrees with itself K half symbols on — built by search with the arbiter over K (smallest first) so that the frame's own last
    #    half symbols in the ring's place, or an emptied ring, give none.
    body16, body17 = soft(fsym(16))[HL:], soft(fsym(17))[HL:]
    for K in range(1, HL):
        h1 = soft(HDR)
        h1[[i for i in range(K, HL) if HDR[i] != HDR[i - K]]] *= np.float32(0.001)
        base = np.concatenate([tail(12), h1, body16])
        y = soft(HDR[HL - K:])
        s = np.concatenate([base, y, body17, tail()])
        fed = np.concatenate([base[-(HL - K):], y])                               # what the ring would hold had the frame's half symbols been fed into it
        emptied = np.concatenate([np.zeros(HL - K, np.float32), y])
        if abs(ref_score(fed)) > F08 or abs(ref_score(emptied)) > F08:
            continue
        got = host_frames(H, s)
        if len(got) == 2 and got[0][0] == 12 + HL and got[1][0] == len(base) + K:
            c["ring_behind_frame"] = dict(s=s, n=2, K=K, at=len(base))
            break
    for v in c.values():
        v.setdefault("softinv", False); v.setdefault("ecc", 1)
    # 8. BCH cases of the end-of-frame step as streams (what the device suite runs)
    named = bch_named(H)
    for name in BCH_STREAMS:
        bits, ecc, _ = named[name]
        c["bch_" + name] = dict(s=np.concatenate([tail(20), soft(sym_of_bits(bits), rng, (0.8, 1.2)), tail()]), n=1, softinv=False, ecc=ecc)
    assert {k: (v["softinv"], v["ecc"]) for k, v in c.items()} == case_opts()
    return c


_cases = None


def cases(H=None):
    global _cases
    if _cases is None:
        _cases = case_streams(H or load_host())
    return _cases


def stream_names():
    """the cases that are about the stream (searched, cut, replayed); the bch_ ones are single frames for the end-of-frame step"""
    return sorted(STREAM_OPTS)


def long_stream():
    """eleven frames at sigma 0.3, longer than the staging buffer"""
    rng = np.random.default_rng(1100)
    s = np.concatenate([soft(fsym(20, "ims100", 11)), np.zeros(60, np.float32)])
    return s + noise(rng, len(s), 0.3)


def cap_stream(nframes=5):
    """frames back to back for one channel"""
    return soft(fsym(30, "rs11g", nframes))


def random_cuts(n, seed, lo=1, hi=2700):
    rng = np.random.default_rng(seed)
    out, tot = [], 0
    while tot < n:
        k = int(rng.integers(lo, hi))
        out.append(k); tot += k
    return out
