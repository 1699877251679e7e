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


def test_sanitized_standalone_replay_of_two_cases(host, tmp_path):
    """the host entry (sonde_lms6_dec_block_bytes) and the emulator translation unit under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program
    with its own main (tests/emu/softin_lms6_replay.cpp), run as a process of its own, outside the interpreter, in the environment as it is (the sanitizer runtimes are linked into the program)"""
    exe = str(tmp_path / "softin_lms6_replay_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(ROOT, "tests", "emu", "softin_lms6_replay.cpp")] + SRCS)
    for name, vit, call in (("lms6_noisy", 2, 1000), ("lms6_after_lmsx", 1, 251)):
        s, typ, _, _ = STREAMS[name]
        p = tmp_path / (name + ".f32")
        s.tofile(str(p))
        r = subprocess.run([exe, str(p), str(call), str(vit), str(typ), "1", "0", "0", "0"], capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert "runtime error" not in r.stderr.decode() and "ERROR: AddressSanitizer" not in r.stderr.decode(), r.stderr.decode()[-2000:]
        assert r.stdout.decode() == _host_text(host, name, vit)[0]
