"""The DEVICE LMS6 / LMS-X soft-bit consumer (radiosonde_auto_rx_amd/csrc/sonde_vit_dev.h: header search, block assembly, the K = 7 Viterbi decoder on one
wavefront — a trellis state per lane —, deconv, bits2bytes) executed on the CPU under tests/emu/wave_emu.h and driven as sonde_softin_dev_push_device drives
k_softin_lms6 (tests/emu/softin_lms6_emu.cpp).  Its block bytes go through sonde_lms6_dec_block_bytes; the text must equal what the host tier
(sonde_lms6_dec_push_soft, pinned to the compiled reference by tests/test_lms6_native.py) prints for the same stream, for --vit and --vit2 and for any cut of
the stream into calls — and the stdout of `oracle/_ref/lms6Xmod --softin ...` where that binary exists.  The same source is compiled by hipcc into
k_softin_lms6; tests/test_gpu_softin_lms6.py runs it there.

A consumer has no `finish`: the streams end after whole blocks plus a short noise tail in which no header is found, so nothing is left in progress."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lms6_vit_model as M
from tools import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc")
EMU_SRC = os.path.join(ROOT, "tests", "emu", "softin_lms6_emu.cpp")
EMU_SO = os.path.join(ROOT, "tests", "emu", "libsoftin_lms6_emu.so")
SRCS = [EMU_SRC, os.path.join(CSRC, "sonde_lms6_fields.cpp"), os.path.join(CSRC, "sonde_ecc.cpp")]
DEPS = SRCS + [os.path.join(ROOT, "tests", "emu", "wave_emu.h")] + [os.path.join(CSRC, h) for h in ("sonde_vit_dev.h", "sonde_softhdr_dev.h", "sonde_rs_dev.h")] + \
       [os.path.join(ROOT, "include", h) for h in ("sonde_lms6.h", "sonde_hip.h", "sonde_ecc.h")]
REF = os.path.join(ROOT, "oracle", "_ref", "lms6Xmod")


class Opts(C.Structure):
    _fields_ = [("raw", C.c_int32), ("ecc", C.c_int32), ("vit", C.c_int32), ("json", C.c_int32), ("typ", C.c_int32), ("gpsweek", C.c_int32),
                ("jsn_freq_khz", C.c_int32), ("version", C.c_char * 32), ("reserved", C.c_int32 * 4)]


class Rec(C.Structure):
    """EmuLms6Rec (tests/emu/softin_lms6_emu.cpp)"""
    _fields_ = [("pos", C.c_int), ("err", C.c_int), ("blen", C.c_int), ("more", C.c_int), ("type", C.c_int), ("mv", C.c_float), ("hdr_bit", C.c_uint64)]


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in DEPS):
        tmp = EMU_SO + ".%d.tmp" % os.getpid()
        # (-ffp-contract=off: the metric is the reference's expression, every product and sum rounded on its own; -Bsymbolic: the decoder inside this
        #  library is its own copy, whatever else the process has loaded)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-Wl,-Bsymbolic", "-o", tmp] + SRCS)
        os.replace(tmp, EMU_SO)
    L = C.CDLL(EMU_SO)
    L.emu_lms6_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Opts), C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.emu_lms6_run_rec.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Opts), C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                   C.POINTER(Rec), C.c_int, C.POINTER(C.c_int)]
    L.emu_lms6_decode.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return L


@pytest.fixture(scope="module")
def host():
    from radiosonde_auto_rx_amd import engine
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    L = C.CDLL(engine.LIB_PATH)
    L.sonde_lms6_dec_create.argtypes = [C.POINTER(Opts), C.POINTER(C.c_void_p)]
    L.sonde_lms6_dec_destroy.argtypes = [C.c_void_p]
    L.sonde_lms6_dec_push_soft.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]
    L.sonde_lms6_dec_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_double, C.c_char_p, C.c_size_t]
    L.sonde_lms6_dec_block_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_double, C.c_char_p, C.c_size_t]
    return L


def _soft(n_blocks, lmsx=False, sigma=0.0, seed=1, lead=37, invert=False):
    """as tests/test_lms6_native.py::_soft"""
    bits = synth.lms6_onair_bits(n_blocks, lmsx)
    s = 2.0 * bits.astype(np.float64) - 1.0
    rng = np.random.default_rng(seed)
    s = np.concatenate([rng.normal(0, 0.3, lead), s])
    s = s + rng.normal(0.0, sigma, len(s))
    if invert:
        s = -s
    return s.astype(np.float32)


def _tail(seed, n=200):
    return np.random.default_rng(1000 + seed).normal(0, 0.3, n).astype(np.float32)


# name -> (soft stream, typ, reference type option, at least this many [OK])
def _streams():
    return {
        "lms6_clean": (np.concatenate([_soft(3), _tail(1)]), 0, [], 3),
        "lms6_noisy": (np.concatenate([_soft(3, sigma=0.3, seed=2), _tail(2)]), 0, [], 3),
        "lms6_inverted": (np.concatenate([_soft(3, sigma=0.1, seed=3, invert=True), _tail(3)]), 0, [], 3),
        "lmsx_forced": (np.concatenate([_soft(2, lmsx=True, sigma=0.1, seed=4), _tail(4)]), 10, ["--lmsX"], 2),
        "lmsx_auto": (np.concatenate([_soft(3, lmsx=True, sigma=0.1, seed=5), _tail(5)]), 0, [], 1),
        "lms6_after_lmsx": (np.concatenate([_soft(3, lmsx=True, sigma=0.2, seed=7), _soft(3, sigma=0.2, seed=8, lead=0), _tail(6)]), 0, [], 2),
    }


STREAMS = _streams()
_want = {}


def _host_text(host, name, vit):
    """sonde_lms6_dec_push_soft on the whole stream (computed once per stream and decoder, shared by the cuts)"""
    if (name, vit) not in _want:
        s, typ, _, _ = STREAMS[name]
        o = Opts(ecc=1, vit=vit, typ=typ)
        d = C.c_void_p()
        assert host.sonde_lms6_dec_create(C.byref(o), C.byref(d)) == 0
        out = C.create_string_buffer(1 << 17)
        assert host.sonde_lms6_dec_push_soft(d, s.ctypes.data, len(s), 0, 0, out, len(out)) >= 0
        host.sonde_lms6_dec_destroy(d)
        ref = None
        if os.path.exists(REF):
            r = subprocess.run([REF, "--softin", "--vit" if vit == 1 else "--vit2", "--ecc"] + STREAMS[name][2], input=s.tobytes(), capture_output=True, timeout=120)
            assert r.returncode == 0
            ref = r.stdout.decode()
        _want[(name, vit)] = (out.value.decode(), ref)
    return _want[(name, vit)]


@pytest.mark.parametrize("call", [4800, 1000, 251])
@pytest.mark.parametrize("vit", [1, 2])
@pytest.mark.parametrize("name", list(STREAMS))
def test_wave_consumer_text_equals_host_tier_and_reference(emu, host, name, vit, call):
    s, typ, _, least = STREAMS[name]
    want, ref = _host_text(host, name, vit)
    assert want.count("[OK]") >= least, want
    o = Opts(ecc=1, vit=vit, typ=typ)
    out = C.create_string_buffer(1 << 17)
    nblk, nlaunch = C.c_int(0), C.c_int(0)
    n = emu.emu_lms6_run(s.ctypes.data, len(s), call, 0, C.byref(o), out, len(out), C.byref(nblk), C.byref(nlaunch))
    assert n >= 0
    got = out.value.decode()
    assert got == want, (name, vit, call, got[:400], want[:400])
    ncalls = -(-len(s) // call)
    if typ == 0:
        assert nlaunch.value > ncalls            # auto detection: a channel stops at a block with input left and is launched again
    else:
        assert nlaunch.value == ncalls           # forced type: one launch per call
    if ref is not None:
        # a consumer keeps a block in progress where the reference prints it at EOF: at most the last reference line may be missing (here none is in progress)
        gl, rl = got.splitlines(), ref.splitlines()
        assert gl == rl or gl == rl[:-1], (name, vit, call, got[:400], ref[:400])


def test_softinv_and_raw_json_text(emu, host):
    """--softinv of the negated stream, and the other output forms (-r, --json with its implied --ecc / --vit) through sonde_lms6_dec_block_bytes"""
    s = np.concatenate([_soft(3, sigma=0.2, seed=9), _tail(9)])
    for kw, inv in ((dict(ecc=1, vit=2), 1), (dict(raw=1, ecc=1, vit=1), 0), (dict(json=1, vit=2, version=b"emu"), 0), (dict(json=1), 0)):
        x = -s if inv else s
        o = Opts(**kw)
        d = C.c_void_p()
        assert host.sonde_lms6_dec_create(C.byref(o), C.byref(d)) == 0
        out = C.create_string_buffer(1 << 17)
        assert host.sonde_lms6_dec_push_soft(d, x.ctypes.data, len(x), inv, 0, out, len(out)) >= 0
        host.sonde_lms6_dec_destroy(d)
        want = out.value.decode()
        assert want.count("[OK]") >= 3
        out2 = C.create_string_buffer(1 << 17)
        assert emu.emu_lms6_run(x.ctypes.data, len(x), 1777, inv, C.byref(o), out2, len(out2), None, None) >= 0
        assert out2.value.decode() == want, kw
    # the algebraic decoder alone has no device form
    assert emu.emu_lms6_run(s.ctypes.data, len(s), 4800, 0, C.byref(Opts(ecc=1, vit=0)), out2, len(out2), None, None) < 0


def test_block_bytes_entry_arguments(host):
    o = Opts(ecc=1, vit=2)
    d = C.c_void_p()
    assert host.sonde_lms6_dec_create(C.byref(o), C.byref(d)) == 0
    out = C.create_string_buffer(4096)
    bb = (C.c_uint8 * 308)()
    nan = float("nan")
    assert host.sonde_lms6_dec_block_bytes(d, bb, 261, 4176, 0.9, nan, nan, out, len(out)) == 0 and out.value == b""       # an empty block: no frame sync, no text
    assert host.sonde_lms6_dec_block_bytes(d, bb, 301, 4176, 0.9, nan, nan, out, len(out)) < 0
    assert host.sonde_lms6_dec_block_bytes(d, bb, 261, 4801, 0.9, nan, nan, out, len(out)) < 0
    assert host.sonde_lms6_dec_block_bytes(d, None, 261, 4176, 0.9, nan, nan, out, len(out)) < 0
    assert host.sonde_lms6_dec_block_bytes(d, bb, 261, 4176, 0.9, nan, nan, None, 0) < 0
    host.sonde_lms6_dec_destroy(d)


@pytest.fixture(scope="module")
def san_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san") / "softin_lms6_replay_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(ROOT, "tests", "emu", "softin_lms6_replay.cpp")] + SRCS)
    return exe


def test_sanitized_standalone_replay_of_two_cases(host, tmp_path, san_exe):
    """the host entry (sonde_lms6_dec_block_bytes) and the emulator translation unit under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program
    with its own main (tests/emu/softin_lms6_replay.cpp), run as a process of its own, outside the interpreter, in the environment as it is (the sanitizer runtimes are linked into the program)"""
    exe = san_exe
    for name, vit, call in (("lms6_noisy", 2, 1000), ("lms6_after_lmsx", 1, 251)):
        s, typ, _, _ = STREAMS[name]
        p = tmp_path / (name + ".f32")
        s.tofile(str(p))
        r = subprocess.run([exe, str(p), str(call), str(vit), str(typ), "1", "0", "0", "0"], capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert "runtime error" not in r.stderr.decode() and "ERROR: AddressSanitizer" not in r.stderr.decode(), r.stderr.decode()[-2000:]
        assert r.stdout.decode() == _host_text(host, name, vit)[0]


# ------------------------------------------------------------------------------------------------------------------------------------------------
# The decoder where it works: against tests/lms6_vit_model.py (a numpy transcription of the reference's block decoder), and on streams whose noise the
# Viterbi decoder has to correct — printed with -r and without --ecc, so that every frame line is the decoder's output as it stands.
# ------------------------------------------------------------------------------------------------------------------------------------------------
NAN = float("nan")
_cache = {}


def _host_raw_lines(host, s, typ, vit):
    o = Opts(raw=1, ecc=0, vit=vit, typ=typ)
    d = C.c_void_p()
    assert host.sonde_lms6_dec_create(C.byref(o), C.byref(d)) == 0
    out = C.create_string_buffer(1 << 18)
    assert host.sonde_lms6_dec_push_soft(d, s.ctypes.data, len(s), 0, 0, out, len(out)) >= 0
    host.sonde_lms6_dec_destroy(d)
    return out.value.decode().splitlines()


def _ref_raw_lines(s, ropt):
    if not os.path.exists(REF):
        return None
    r = subprocess.run([REF, "--softin", "-r"] + ropt, input=s.tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0
    return r.stdout.decode().splitlines()


def _same(got, ref):
    """(a consumer keeps a block in progress where the reference prints it at EOF: at most the last reference line may be missing)"""
    return ref is None or got == ref or got == ref[:-1]


def _noisy(host, tn, kind):
    """a stream of section NOISY_*: what the host tier and the reference print for it and for its noiseless counterpart, and the model's blocks (once)"""
    if (tn, kind) not in _cache:
        s, clean, typ, vit, ropt = M.noisy_stream(tn, kind)
        want, base = _host_raw_lines(host, s, typ, vit), _host_raw_lines(host, clean, typ, vit)
        _cache[(tn, kind)] = dict(s=s, typ=typ, vit=vit, want=want, base=base, ref=_ref_raw_lines(s, ropt))
    return _cache[(tn, kind)]


def _model_blocks(s, vit, lens):
    """[(hdr_bit, mv, raw soft values, (bytes, blen, err))] of the model's framer and decoder; lens[k] = raw positions of block k (the last entry repeats)"""
    out = []
    for hb, mv, raw in M.frame_stream(s, lambda k: lens[min(k, len(lens) - 1)] - M.BLOCKSTART):
        out.append((hb, mv, raw, M.decode_block(M.block_sb(raw, mv, vit))))
    return out


@pytest.mark.parametrize("vit", [1, 2])
@pytest.mark.parametrize("kind", list(M.NOISY_KINDS))
@pytest.mark.parametrize("tn", ["lms6", "lmsx"])
def test_model_bytes_give_the_text_of_the_host_decoder_and_the_reference(host, tn, kind, vit):
    """the model is pinned before it is used: its bytes through sonde_lms6_dec_block_bytes print what sonde_lms6_dec_block prints for the same soft block
    (raw = 1, ecc = 0, forced type), block by block; all blocks together are the host tier's text of the stream and the reference's stdout"""
    s, _, typ, _, ropt = M.noisy_stream(tn, kind)
    o = Opts(raw=1, ecc=0, vit=vit, typ=typ)
    da, db = C.c_void_p(), C.c_void_p()
    assert host.sonde_lms6_dec_create(C.byref(o), C.byref(da)) == 0 and host.sonde_lms6_dec_create(C.byref(o), C.byref(db)) == 0
    blocks = _model_blocks(s, vit, [M.RAWBLKX if typ == 10 else M.RAWBLK6])
    assert len(blocks) >= 3
    a, b = C.create_string_buffer(8192), C.create_string_buffer(8192)
    text, synced = "", 0
    for hb, mv, raw, (by, blen, err) in blocks:
        assert host.sonde_lms6_dec_block(da, raw.ctypes.data, None, len(raw), float(mv), NAN, NAN, a, len(a)) >= 0
        assert host.sonde_lms6_dec_block_bytes(db, by.ctypes.data, blen, len(raw) + M.BLOCKSTART, float(mv), NAN, NAN, b, len(b)) >= 0
        assert a.value == b.value, (tn, kind, vit, hb, blen, err)
        synced += bool(a.value)
        text += b.value.decode()
    host.sonde_lms6_dec_destroy(da); host.sonde_lms6_dec_destroy(db)
    assert synced >= 1                                        # blocks that have a frame sync (hard decisions at sigma 0.9 leave few)
    lines = text.splitlines()
    assert lines == _host_raw_lines(host, s, typ, vit)
    assert _same(lines, _ref_raw_lines(s, ropt[:-1] + ["--vit" if vit == 1 else "--vit2"]))


# ---- lms6_wave_decode alone, byte for byte against the model
def _encode(u):
    """code bits (c0, c1) of the input bits u, six zero bits in front of them"""
    pa, pb = np.array([int(c) for c in M.POLY_A]), np.array([int(c) for c in M.POLY_B])
    win = np.lib.stride_tricks.sliding_window_view(np.concatenate([np.zeros(6, np.int64), np.asarray(u, np.int64)]), 7)
    return np.stack([(win @ pa) & 1, (win @ pb) & 1], axis=1).ravel()


def _code_word(rng, n, zero_start=True):
    u = rng.integers(0, 2, (n + 1) // 2)
    if zero_start:
        u[:6] = 0
    else:
        u[:6] = [1, 0, 1, 1, 0, 1]
    return (2.0 * _encode(u)[:n] - 1.0)


def _gen(kind, n, rng, p):
    """-> sb[0 .. n) as float32"""
    if kind == "noise":
        s = _code_word(rng, n) + rng.normal(0, p, n)
    elif kind == "hard":
        s = _code_word(rng, n)
        s[rng.random(n) < p] *= -1.0
    elif kind == "grid":
        s = np.round(2.0 * (_code_word(rng, n) + rng.normal(0, p, n))) / 2.0
    elif kind == "zeros":
        s = _code_word(rng, n) + rng.normal(0, 0.5, n)
        s[rng.random(n) < p] = 0.0
    elif kind == "allzero":
        s = np.zeros(n)
    elif kind == "negzero":                                    # -0.0 wherever the code bit is 0, +0.0 elsewhere, and a few of them among noisy values
        c = _code_word(rng, n)
        s = np.where(rng.random(n) < p, np.where(c < 0, -0.0, 0.0), c + rng.normal(0, 0.5, n))
    elif kind == "absorb":                                     # 1e4 swallows what 1e-3 contributes to a float32 path metric: ties through absorption
        c = _code_word(rng, n)
        s = np.where(rng.random(n) < p, 1e4 * c, 1e-3 * c * np.sign(rng.normal(0, 1, n) + 0.8))
    elif kind == "random":                                     # no code structure
        s = 2.0 * rng.integers(0, 2, n) - 1.0
    elif kind == "start":                                      # the first 12 positions encode input bits that are not zero
        s = _code_word(rng, n, zero_start=False) + rng.normal(0, p, n)
    else:
        raise KeyError(kind)
    return np.asarray(s, np.float64).astype(np.float32)


def _decode_cases():
    """name -> (kind, len, parameter); most on the short lengths (tmax 7, and 63 / 64 / 65 across the edge of the 64-step chunks of decision words, 129, odd),
    a handful on the full blocks"""
    cs = {}
    for n in (14, 126, 128, 130, 258, 1001):
        for kind, p in (("noise", 0.5), ("noise", 0.8), ("noise", 1.2), ("zeros", 0.05), ("zeros", 0.3), ("negzero", 0.3), ("absorb", 0.5), ("random", 0), ("start", 0.3)):
            cs["%s_%g_len%d" % (kind, p, n)] = (kind, n, p)
        cs["hard_0.08_len%d" % n] = ("hard", n, 0.08)
    for n in (258, 1001):
        for p in (0.02, 0.15):
            cs["hard_%g_len%d" % (p, n)] = ("hard", n, p)
        cs["grid_0.7_len%d" % n] = ("grid", n, 0.7)
    cs["grid_0.7_len128"] = ("grid", 128, 0.7)
    cs["allzero_len130"] = ("allzero", 130, 0)
    cs["random_b_len1001"] = ("random", 1001, 0)
    cs["random_c_len258"] = ("random", 258, 0)
    for kind, n, p in (("noise", 4176, 0.9), ("hard", 4176, 0.08), ("absorb", 4176, 0.5), ("random", 4176, 0), ("grid", 4800, 0.7), ("zeros", 4800, 0.15),
                       ("allzero", 4800, 0), ("start", 4800, 0.5)):
        cs["%s_%g_len%d" % (kind, p, n)] = (kind, n, p)
    return cs


DECODE_CASES = _decode_cases()


def _decode_case(name):
    """the case's block and the model's (bytes, blen, err, steps with a tie), once"""
    if ("case", name) not in _cache:
        kind, n, p = DECODE_CASES[name]
        sb = _gen(kind, n, np.random.default_rng(list(DECODE_CASES).index(name) + 5000), p)
        assert len(sb) == n and np.all(np.isfinite(sb))
        _cache[("case", name)] = (sb, M.decode_block(sb, with_ties=True))
    return _cache[("case", name)]


def test_direct_decode_cases_reach_the_error_stop_and_the_ties():
    """what the cases have to exercise, decided by the model alone: deconv's error stop (err != 0, the string cut there: blen < len / 16) in at least a quarter of
    the blocks without code structure or with a non-zero start, and 100 or more steps with tied candidates in at least half of the hard and 0.5-grid blocks"""
    cut = [n for n, (k, _, _) in DECODE_CASES.items() if k in ("random", "start")]
    hit = [n for n in cut if _decode_case(n)[1][2] != 0 and _decode_case(n)[1][1] < DECODE_CASES[n][1] / 16]
    assert 4 * len(hit) >= len(cut), (hit, cut)
    tied = [n for n, (k, _, _) in DECODE_CASES.items() if k in ("hard", "grid")]
    many = [n for n in tied if _decode_case(n)[1][3] >= 100]
    assert 2 * len(many) >= len(tied), (many, tied)
    # (and the blocks do differ from a plain hard decision: the decoder has errors to correct)
    assert sum(_decode_case(n)[1][2] == 0 and _decode_case(n)[1][1] == DECODE_CASES[n][1] // 16 for n in DECODE_CASES) >= len(DECODE_CASES) // 2


@pytest.mark.parametrize("name", list(DECODE_CASES))
def test_direct_decode_equals_model_byte_for_byte(emu, name):
    """lms6_wave_decode under the wave emulator on sb[0 .. len) — all positions the caller's — against the model: all 308 bytes, blen and err, exactly"""
    sb, (by, blen, err, _) = _decode_case(name)
    out = (C.c_uint8 * 308)()
    bl, er = C.c_int(-1), C.c_int(-1)
    assert emu.emu_lms6_decode(sb.ctypes.data, len(sb), out, C.byref(bl), C.byref(er)) == 0
    assert (bl.value, er.value) == (blen, err), name
    assert bytes(out) == by.tobytes(), (name, [i for i in range(308) if out[i] != by[i]][:8])


# ---- streams in which the decoder corrects and fails, no Reed-Solomon behind it
def _emu_raw(emu, s, typ, vit, call, cap=8):
    o = Opts(raw=1, ecc=0, vit=vit, typ=typ)
    out = C.create_string_buffer(1 << 18)
    recs = (Rec * 64)()
    nblk, nl, nd = C.c_int(0), C.c_int(0), C.c_int(0)
    assert emu.emu_lms6_run_rec(s.ctypes.data, len(s), call, 0, C.byref(o), cap, out, len(out), C.byref(nblk), C.byref(nl), recs, 64, C.byref(nd)) >= 0
    return out.value.decode().splitlines(), [recs[i] for i in range(min(nblk.value, 64))], nd.value


@pytest.mark.parametrize("kind", list(M.NOISY_KINDS))
@pytest.mark.parametrize("tn", list(M.NOISY_TYPES))
def test_noisy_streams_make_the_decoder_work(host, tn, kind):
    """the condition on the streams: the host tier (equal to the reference where that is built) prints at least three frame lines, and at least three of them are
    not lines of the noiseless stream — the decoder's output has errors in it, and nothing repairs them before the comparison"""
    c = _noisy(host, tn, kind)
    assert len(c["want"]) >= 3 and sum(l not in c["base"] for l in c["want"]) >= 3, (len(c["want"]), len(c["base"]))
    assert _same(c["want"], c["ref"])


@pytest.mark.parametrize("call", [4800, 1000, 251])
@pytest.mark.parametrize("kind", list(M.NOISY_KINDS))
@pytest.mark.parametrize("tn", list(M.NOISY_TYPES))
def test_wave_consumer_raw_text_of_noisy_streams(emu, host, tn, kind, call):
    """--softin --vit | --vit2 -r: the emulated consumer prints the host tier's and the reference's lines, and every record's blen and err are the model's"""
    c = _noisy(host, tn, kind)
    got, recs, dropped = _emu_raw(emu, c["s"], c["typ"], c["vit"], call)
    assert got == c["want"], (tn, kind, call, len(got), len(c["want"]))
    assert _same(got, c["ref"]) and dropped == 0
    if "model" not in c:
        c["model"] = _model_blocks(c["s"], c["vit"], [M.RAWBLKX if c["typ"] == 10 else M.RAWBLK6] + [M.RAWBLKX if r.type == 10 else M.RAWBLK6 for r in recs])
    assert [(r.hdr_bit, r.mv > 0, r.blen, r.err) for r in recs] == [(hb, mv > 0, blen, err) for hb, mv, _, (_, blen, err) in c["model"]]


@pytest.mark.parametrize("call", [1, 63, 64, 65])
def test_calls_shorter_than_the_header_window(emu, host, call):
    """one block in calls of 1, 63, 64 and 65 soft bits: the header window lies mostly (or all but one element) in the ring the channel keeps between calls"""
    s, _, typ, vit, _ = M.noisy_stream("lms6", "vit_s07", n_blocks=1)
    want = _host_raw_lines(host, s, typ, vit)
    assert len(want) >= 1
    got, recs, _ = _emu_raw(emu, s, typ, vit, call)
    assert got == want and len(recs) == 1 and recs[0].hdr_bit == 37 + 80


# ---- the header at the threshold
@pytest.mark.parametrize("invert", [False, True], ids=["pos", "neg"])
@pytest.mark.parametrize("name", list(M.THRESHOLD_CASES))
def test_header_at_the_threshold(emu, host, name, invert):
    """64 header bits with 9 flips (46 / 64 = 0.71875 > 0.7) and 10 (0.6875), and values that put the score within 1e-3 of 0.7 on either side: whether a block is
    found is the host tier's (and the reference's) decision; the emulated consumer agrees, with the header's bit index and the sign of its score"""
    flips, target = M.THRESHOLD_CASES[name]
    s, score, hdr_bit = M.threshold_stream(flips, target, invert)
    if target is None:
        assert score == (64 - 2 * flips) / 64.0
    else:
        assert abs(score - 0.7) < 1e-3 and (score > 0.7) == (target > 0.7)
    want = _host_raw_lines(host, s, 6, 1)
    assert _same(want, _ref_raw_lines(s, ["--lms6", "--vit"]))
    assert bool(want) == (score > 0.7), (name, score, want[:1])
    got, recs, _ = _emu_raw(emu, s, 6, 1, 1000)
    assert got == want
    assert [(r.hdr_bit, r.mv < 0) for r in recs] == ([(hdr_bit, invert)] if score > 0.7 else [])
    if recs:
        assert abs(abs(recs[0].mv) - score) < 1e-6


# ---- more blocks in a call than the record buffer holds
def _overflow_stream(n_blocks, seed=41):
    return M.soft_stream(n_blocks, sigma=0.7, seed=seed)


def _host_block_texts(host, s, vit, typ=6):
    """what the host tier prints per block (sonde_lms6_dec_block on the blocks of the model's framer)"""
    o = Opts(raw=1, ecc=0, vit=vit, typ=typ)
    d = C.c_void_p()
    assert host.sonde_lms6_dec_create(C.byref(o), C.byref(d)) == 0
    a = C.create_string_buffer(8192)
    out = []
    for hb, mv, raw in M.frame_stream(s, lambda k: M.RAWBLK6 - M.BLOCKSTART):
        assert host.sonde_lms6_dec_block(d, raw.ctypes.data, None, len(raw), float(mv), NAN, NAN, a, len(a)) >= 0
        out.append((hb, a.value.decode()))
    host.sonde_lms6_dec_destroy(d)
    return out


def test_blocks_beyond_the_record_buffer_are_dropped_and_the_rest_is_intact(emu, host):
    """ten blocks in one call, room for eight records: the ninth and tenth are decoded into the tail of the wave's LDS and dropped; the eight are what the host
    tier prints for those blocks"""
    s = _overflow_stream(10)
    per_block = _host_block_texts(host, s, 1)
    assert len(per_block) == 10 and "".join(t for _, t in per_block).splitlines() == _host_raw_lines(host, s, 6, 1)
    got, recs, dropped = _emu_raw(emu, s, 6, 1, len(s))
    assert dropped == 2 and len(recs) == 8
    assert got == "".join(t for _, t in per_block[:8]).splitlines() and len(got) >= 6
    assert [r.hdr_bit for r in recs] == [hb for hb, _ in per_block[:8]]


def test_sanitized_standalone_replay_of_the_dropped_record_path(host, tmp_path, san_exe):
    """the same under AddressSanitizer + UndefinedBehaviorSanitizer in the stand-alone program: the dropped blocks' bytes go to L->sb + 3 * LMS6_RAWBLKX"""
    s = _overflow_stream(10)
    p = tmp_path / "overflow.f32"
    s.tofile(str(p))
    r = subprocess.run([san_exe, str(p), str(len(s)), "1", "6", "0", "1", "0", "0"], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert "runtime error" not in r.stderr.decode() and "ERROR: AddressSanitizer" not in r.stderr.decode(), r.stderr.decode()[-2000:]
    assert "8 blocks, 1 launches, 2 dropped" in r.stderr.decode()
    assert r.stdout.decode().splitlines() == "".join(t for _, t in _host_block_texts(host, s, 1)[:8]).splitlines()
