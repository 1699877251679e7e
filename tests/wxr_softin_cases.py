"""Streams and arbiters shared by tests/test_softin_wxr_emu.py (the device WxR-301D soft-bit consumer under the CPU wave emulator), tests/test_gpu_softin_wxr_dev.py
(the same source as k_softin_wxr on the device) and tools/make_golden_wxr_softin.py (the reference's stdout on the same streams, tests/golden/wxr_softin_*.npz).

The streams are soft bits built from tools/synth.wxr_frames, a few thousand each, and need nothing but numpy: +1.0 for a 1 and -1.0 for a 0 (the negated stream
for the -i cases), with exact zeros and NaNs where a case is about them.  The first arbiter is the host tier on the same stream: sonde_wxr_softin_push for the
frames (bits and the number of soft bits read before the matching one) and sonde_wxr_print_frame for the text; the second is the recorded stdout of the compiled
reference.  A consumer has no `finish`: every stream ends in idle bits, so no header is open at its end (the reference would print a -t prefix for it)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

from tools import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_SRC = os.path.join(EMU_DIR, "softin_wxr_emu.cpp")
EMU_SO = os.path.join(EMU_DIR, "libsoftin_wxr_emu.so")
DEPS = [EMU_SRC, os.path.join(EMU_DIR, "wave_emu.h"), os.path.join(CSRC, "sonde_softin_wxr_dev.h"), os.path.join(CSRC, "sonde_softin_wave_dev.h"),
        os.path.join(CSRC, "sonde_rs_dev.h"), os.path.join(ROOT, "include", "sonde_hip.h")]
HL, NBITS, NBYTES = 40, 552, 69
HDR_HEX = {False: "AAAAAA2DD4", True: "AAAAAAC194"}
CUTS = [1, 39, 40, 41, 63, 64, 65, 552, 553]
VERSION = "oracle"                                           # -DVER_JSN_STR of the recorded reference build


def hdr_bits(pn9=False):
    return np.unpackbits(np.frombuffer(bytes.fromhex(HDR_HEX[bool(pn9)]), np.uint8))


class Rec(C.Structure):
    """SoftinWxrRec (csrc/sonde_softin_wxr_dev.h) = sonde_wxr_softin_rec_t (include/sonde_fsk.h)"""
    _fields_ = [("channel", C.c_int32), ("pad", C.c_int32), ("hdr_bit", C.c_uint64), ("raw", C.c_uint8 * 69), ("x", C.c_uint8 * 69), ("pad2", C.c_uint8 * 2),
                ("chkval", C.c_uint32), ("chkdat", C.c_uint32), ("chk_ok", C.c_uint8), ("frid", C.c_uint8), ("pad3", C.c_uint8 * 2), ("sn", C.c_uint32), ("cnt", C.c_uint32)]


class EmuState(C.Structure):
    """EmuWxrState (tests/emu/softin_wxr_emu.cpp)"""
    _fields_ = [("mode", C.c_int), ("pos", C.c_int), ("hist", C.c_uint64), ("valid", C.c_uint64), ("bits_in", C.c_uint64), ("hdr_bit", C.c_uint64), ("w", C.c_uint32 * 18)]


class HostFrame(C.Structure):
    """sonde_wxr_frame_t"""
    _fields_ = [("channel", C.c_int32), ("nbits", C.c_int32), ("complete", C.c_int32), ("reserved", C.c_int32), ("sample", C.c_uint64), ("bits", C.c_uint8 * NBITS)]


class HostOpts(C.Structure):
    """sonde_wxr_opts_t"""
    _fields_ = [(n, C.c_int32) for n in ("raw", "vbs", "json", "pn9", "jsn_freq_khz")] + [("version", C.c_char * 32), ("ts", C.c_int32), ("reserved", C.c_int32 * 3)]


def load_emu(src=EMU_SRC, so=EMU_SO, deps=DEPS, flags=()):
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = so + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", *flags, "-o", tmp, src])
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.emu_wxr_run.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Rec), C.c_int, C.POINTER(C.c_int),
                              C.POINTER(EmuState)]
    L.emu_wxr_end.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_uint)]
    L.emu_wxr_header40.restype = C.c_uint64
    return L


def load_host():
    from radiosonde_auto_rx_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    L = C.CDLL(engine.LIB_PATH)
    P = C.c_void_p
    L.sonde_wxr_softin_create.argtypes = [C.c_int32, C.c_int32, C.POINTER(P)]
    L.sonde_wxr_softin_destroy.argtypes = [P]
    L.sonde_wxr_softin_destroy.restype = None
    L.sonde_wxr_softin_push.argtypes = [P, P, C.c_int32, C.POINTER(HostFrame), C.c_int32]
    L.sonde_wxr_softin_finish.argtypes = [P, C.POINTER(HostFrame)]
    L.sonde_wxr_printer_create.argtypes = [C.POINTER(HostOpts), C.POINTER(P)]
    L.sonde_wxr_printer_destroy.argtypes = [P]
    L.sonde_wxr_printer_destroy.restype = None
    L.sonde_wxr_print_frame.argtypes = [P, C.POINTER(C.c_uint8), C.c_char_p, C.c_size_t]
    L.sonde_wxr_print_decoded.argtypes = [P, C.POINTER(Rec), C.c_char_p, C.c_size_t]
    return L


# ---------------------------------------------------------------- argument lists
def opts_of(argv):
    """the switches of a weathex301d argument list: pn9, inv (-i), raw (-r 1 / -R 2), vbs, json, ts"""
    a = list(argv)
    return dict(pn9="--pn9" in a, inv="-i" in a, raw=2 if "-R" in a else 1 if "-r" in a else 0, vbs="-v" in a, json="--json" in a, ts="-t" in a)


def printer(H, argv, ts=True):
    o = opts_of(argv)
    ho = HostOpts(raw=o["raw"], vbs=int(o["vbs"]), json=int(o["json"]), pn9=int(o["pn9"]), jsn_freq_khz=0, version=VERSION.encode(), ts=int(o["ts"] and ts))
    h = C.c_void_p()
    assert H.sonde_wxr_printer_create(C.byref(ho), C.byref(h)) == 0
    return h


# ---------------------------------------------------------------- the arbiter: the host tier
_arb = {}


def host_frames(H, s, pn9=False, inv=False, cache=None):
    """[(bits read before the matching one, the 552 frame bits as 69 bytes)] of sonde_wxr_softin_push over the whole stream; no header may be open at its end"""
    key = (cache, bool(pn9), bool(inv))
    if cache is not None and key in _arb:
        return _arb[key]
    s = np.ascontiguousarray(s, np.float32)
    h = C.c_void_p()
    assert H.sonde_wxr_softin_create(int(pn9), int(inv), C.byref(h)) == 0
    buf = (HostFrame * (len(s) // NBITS + 2))()
    n = H.sonde_wxr_softin_push(h, s.ctypes.data, len(s), buf, len(buf))
    assert 0 <= n < len(buf)
    out = []
    for f in buf[:n]:
        bits = np.frombuffer(bytes(f.bits), np.uint8)
        assert f.complete and f.nbits == NBITS and bits.max() <= 1
        out.append((int(f.sample), bytes(np.packbits(bits))))
    assert H.sonde_wxr_softin_finish(h, buf) == 0, "a header is open at the end of the stream"
    H.sonde_wxr_softin_destroy(h)
    if cache is not None:
        _arb[key] = out
    return out


def host_text(H, frames, argv):
    """what the host tier prints for those frames under an argument list: print_frame on the bits, the --softin loop's -t prefix in front"""
    o = opts_of(argv)
    p = printer(H, argv)
    buf = C.create_string_buffer(4096)
    text = b""
    for hb, by in frames:
        bits = np.unpackbits(np.frombuffer(by, np.uint8))
        n = H.sonde_wxr_print_frame(p, bits.ctypes.data_as(C.POINTER(C.c_uint8)), buf, len(buf))
        assert n >= 0
        if o["ts"]:
            text += b"<%8.3f> " % (hb / (5000.0 if o["pn9"] else 4800.0))
        text += buf.raw[:n]
    H.sonde_wxr_printer_destroy(p)
    return text


def rec_text(H, recs, argv):
    """what sonde_wxr_print_decoded prints for those records (Recs or fetch_wxr dicts) under an argument list"""
    p = printer(H, argv)
    buf = C.create_string_buffer(4096)
    text = b""
    for r in recs:
        n = H.sonde_wxr_print_decoded(p, C.byref(as_rec(r)), buf, len(buf))
        assert n >= 0
        text += buf.raw[:n]
    H.sonde_wxr_printer_destroy(p)
    return text


def as_rec(r):
    if isinstance(r, Rec):
        return r
    o = Rec()
    for k in ("channel", "hdr_bit", "chkval", "chkdat", "chk_ok", "frid", "sn", "cnt"):
        setattr(o, k, int(r[k]))
    o.raw = (C.c_uint8 * 69)(*bytes(r["raw"])); o.x = (C.c_uint8 * 69)(*bytes(r["x"]))
    return o


# ---------------------------------------------------------------- the serial model of the end of a frame
def verdict(by69, pn9=False):
    """(x, chkval, chkdat, chk_ok, frid, sn, cnt) of 69 frame bytes as on the air: PN9 from byte 6, xor8sum over the 53 bytes from ofs"""
    x = bytearray(by69)
    ofs = 8 if pn9 else 6
    if pn9:
        for j in range(6, NBYTES):
            x[j] ^= synth.WXR_PN9[j - 6]
    val = synth.wxr_xor8sum(x[ofs:ofs + 53])
    dat = x[ofs + 53] << 8 | x[ofs + 54]
    return bytes(x), val, dat, int(val == dat), x[ofs + 6], int.from_bytes(x[ofs:ofs + 4], "little"), x[ofs + 4] | x[ofs + 5] << 8


def _g(r):
    return (lambda k: r[k]) if isinstance(r, dict) else (lambda k: getattr(r, k))


def key(r, pn9=False):
    """everything a record holds, of a Rec, a fetch_wxr dict or an arbiter tuple (hdr_bit, bytes69) through the serial model"""
    if isinstance(r, tuple):
        return (r[0], r[1]) + verdict(r[1], pn9)
    g = _g(r)
    return (g("hdr_bit"), bytes(g("raw")), bytes(g("x")), g("chkval"), g("chkdat"), g("chk_ok"), g("frid"), g("sn"), g("cnt"))


def emu_frames(E, s, calls, pn9=False, inv=False, softinv=False, cap=64):
    """the emulated consumer over the stream cut into calls (the last length repeats): Recs, frames dropped for want of room, end state"""
    s = np.ascontiguousarray(s, np.float32)
    buf = (Rec * (len(s) // NBITS + 2))()
    cl = (C.c_int * len(calls))(*calls)
    dropped, end = C.c_int(0), EmuState()
    n = E.emu_wxr_run(s.ctypes.data, len(s), cl, len(calls), int(softinv), int(inv), int(pn9), cap, buf, len(buf), C.byref(dropped), C.byref(end))
    assert 0 <= n < len(buf), n
    for i in range(n):
        assert buf[i].channel == 0
    return [buf[i] for i in range(n)], dropped.value, end


def state(end):
    """the end state as far as it means anything: the ring while searching; the bits so far, the frame position and the header's place inside a frame"""
    if end.mode == 1:
        words = [int(end.w[k]) & (0xFFFFFFFF if 32 * k + 32 <= end.pos else (1 << max(end.pos - 32 * k, 0)) - 1) for k in range(18)]
        return (1, end.bits_in, end.pos, words, end.hdr_bit)
    return (0, end.bits_in, end.pos, end.hist, end.valid)


# ---------------------------------------------------------------- frames and streams
def fbits(frame):
    return np.unpackbits(np.frombuffer(bytes(frame), np.uint8))


def idle(n):
    return np.tile(np.array([1, 0], np.uint8), (n + 1) // 2)[:n]


def onair(frames, lead=24, gap=96, tail=70):
    """the frames' 552 bits each, behind `lead` idle bits 1010 .., with `gap` of them between two frames and `tail` behind the last"""
    parts = []
    for k, f in enumerate(frames):
        parts += [idle(gap if k else lead), fbits(f)]
    return np.concatenate(parts + [idle(tail)])


def soft(bits, rng=None, jitter=(0.6, 1.4)):
    s = 2.0 * np.asarray(bits, np.float64) - 1.0
    if rng is not None:
        s = s * rng.uniform(jitter[0], jitter[1], len(s))
    return s.astype(np.float32)


def refit(frame, pn9=False):
    """the frame with its check recomputed over what it holds now"""
    x, val = verdict(frame, pn9)[:2]
    x = bytearray(x)
    ofs = 8 if pn9 else 6
    x[ofs + 53], x[ofs + 54] = val >> 8, val & 0xFF
    if pn9:
        for j in range(6, NBYTES):
            x[j] ^= synth.WXR_PN9[j - 6]
    return bytes(x)


def _flips(bits, rng, n):
    bits = bits.copy()
    bits[rng.choice(len(bits), n, replace=False)] ^= 1
    return bits


JSON, RT, RAW2, VBS = ["--json"], ["-r", "-t"], ["-R"], ["-v"]


def build_cases():
    """name -> dict(s = float32 soft bits, pn9, inv = the consumer's -i, n = frames, ok = their verdicts, hb = bits read before each matching one (None: whatever the
    arbiter says), argv = the argument lists (behind --softin) whose reference stdout the golden holds; the first one's switches are the case's own)"""
    c = {}
    fr = lambda n, pn9, cnt0=100: synth.wxr_frames(n, pn9, cnt0=cnt0)                          # noqa: E731
    every = lambda pn: [JSON + pn, RT + pn, RAW2 + pn, VBS + pn, ["-r", "-v"] + pn]                # noqa: E731
    # 1. clean, both variants; the other variant's consumer and the other polarity find nothing in them
    for pn9, name in ((False, "clean"), (True, "clean_pn9")):
        pn = ["--pn9"] if pn9 else []
        s = soft(onair(fr(4, pn9)))
        c[name] = dict(s=s, pn9=pn9, n=4, ok=[1] * 4, hb=[24 + 39 + k * (NBITS + 96) for k in range(4)], argv=every(pn))
        c[name + "_other_variant"] = dict(s=s, pn9=not pn9, n=0, ok=[], hb=[], argv=[RT + (["--pn9"] if not pn9 else [])])
        c[name + "_i"] = dict(s=s, pn9=pn9, inv=True, n=0, ok=[], hb=[], argv=[["-i"] + JSON + pn])
        c[name + "_negated_i"] = dict(s=-s, pn9=pn9, inv=True, n=4, ok=[1] * 4, hb=c[name]["hb"], argv=[["-i"] + JSON + pn, ["-i"] + RT + pn])
    # 2. the start of the stream: a header at bit 0 matches at bit 39; a stream that starts with header[1:] and 512 bits yields nothing (39 bits cannot match)
    f = fr(3, False, 300)
    c["start_at_0"] = dict(s=soft(onair(f, lead=0)), pn9=False, n=3, ok=[1] * 3, hb=[39 + k * (NBITS + 96) for k in range(3)], argv=[RT, JSON])
    c["start_39_bits"] = dict(s=soft(np.concatenate([fbits(f[0])[1:], idle(80)])), pn9=False, n=0, ok=[], hb=[], argv=[RT])
    # 3. the ring behind a frame holds the frame's last 40 bits: a payload that ends in header[:39] (bytes 61 .. 68 are behind the check) and the next bit completes
    #    the header; the same with one bit of that tail flipped finds none; a header in mid-payload opens nothing
    for pn9, name in ((False, "ring_behind_frame"), (True, "ring_behind_frame_pn9")):
        a, b = fr(2, pn9, 400)
        ab = fbits(a)
        ab[NBITS - 39:] = hdr_bits(pn9)[:39]
        rest = np.concatenate([hdr_bits(pn9)[39:], fbits(b)[HL:], idle(90)])
        bits = np.concatenate([idle(30), ab, rest])
        pn = ["--pn9"] if pn9 else []
        ok_a = verdict(bytes(np.packbits(ab)), pn9)[3]
        c[name] = dict(s=soft(bits), pn9=pn9, n=2, ok=[ok_a, 1], hb=[30 + 39, 30 + NBITS], argv=[RT + pn, JSON + pn], end=30 + NBITS)
        flipped = bits.copy()
        flipped[30 + NBITS - 17] ^= 1
        c[name + "_tail_flipped"] = dict(s=soft(flipped), pn9=pn9, n=1, ok=[ok_a], hb=[30 + 39], argv=[RT + pn])
    a, b = fr(2, False, 500)
    a = bytearray(a)
    a[30:35] = bytes.fromhex(HDR_HEX[False])
    c["header_in_payload"] = dict(s=soft(onair([refit(a), b])), pn9=False, n=2, ok=[1, 1], hb=[24 + 39, 24 + NBITS + 96 + 39], argv=[RT, JSON])
    # 4. exact zeros of both signs and NaNs inside a payload: +-0.0 is a 1 and a NaN a 0, with and without -i (the negated stream keeps its NaNs)
    rng = np.random.default_rng(301)
    s = soft(onair(fr(2, False, 600)), rng)
    pay = 24 + HL + 16
    for k, p in enumerate(range(pay, pay + 400, 7)):
        s[p] = (np.float32(0.0), np.float32(-0.0), np.float32(np.nan))[k % 3]
    c["zeros_nan"] = dict(s=s, pn9=False, n=2, ok=None, hb=[24 + 39, 24 + NBITS + 96 + 39], argv=[["-r", "-v"], RAW2], payload=(pay, pay + 400))
    c["zeros_nan_i"] = dict(s=-s, pn9=False, inv=True, n=2, ok=None, hb=c["zeros_nan"]["hb"], argv=[["-i", "-r", "-v"], ["-i"] + RAW2], payload=(pay, pay + 400))
    # 5. damaged streams: bit flips all over six frames (a header missed, checks that fail, frame ids that are none), both variants, soft values of any size
    for pn9, name, seed in ((False, "flips", 302), (True, "flips_pn9", 303)):
        rng = np.random.default_rng(seed)
        pn = ["--pn9"] if pn9 else []
        bits = _flips(onair(synth.wxr_frames(6, pn9, cnt0=700, corrupt=(3,)), gap=40), rng, 5)
        c[name] = dict(s=soft(bits, rng, (0.05, 2.0)), pn9=pn9, n=None, ok=None, hb=None, argv=[JSON + pn, ["-r", "-v", "-t"] + pn, VBS + ["--json"] + pn])
    # 6. back to back: five frames without a gap (the record cap), and a sixth call's worth behind them
    c["back_to_back"] = dict(s=soft(onair(fr(5, False, 800), lead=0, gap=0, tail=0)), pn9=False, n=5, ok=[1] * 5, hb=[39 + NBITS * k for k in range(5)], argv=None,
                             open_end=False)
    for v in c.values():
        v.setdefault("inv", False)
    return c


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = build_cases()
    return _cases


GOLDEN_CASES = sorted(k for k, v in build_cases().items() if v["argv"])
DAMAGED = ["flips", "flips_pn9"]


def golden_path(name):
    return os.path.join(GOLDEN, "wxr_softin_%s.npz" % name)


def load_golden(name):
    """the recorded reference: soft (float32, from int8 signs where the stream is +-1 alone), argv (with --softin in front), stdout per argument list"""
    z = np.load(golden_path(name))
    raw, ends = z["stdout"].tobytes(), np.cumsum(z["lengths"])
    s = z["soft"]
    return {"soft": s.astype(np.float32), "argv": [json.loads(str(a)) for a in z["argv"]], "stdout": [raw[e - n:e] for e, n in zip(ends, z["lengths"])]}


def random_cuts(n, seed, lo=1, hi=700):
    rng = np.random.default_rng(seed)
    out, tot = [], 0
    while tot < n:
        k = int(rng.integers(lo, hi))
        out.append(k); tot += k
    return out
