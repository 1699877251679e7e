"""The DEVICE RS92 soft-bit consumer (radiosonde_auto_rx_amd/csrc/sonde_softin_rs92_dev.h: header search at 0.8 with the ring emptied on every hit, the polarity
rule, 8N1 bytes from two soft symbols per bit on a lane per byte, RS(255,231) of the finished frame on the wave) executed on the CPU under tests/emu/wave_emu.h and
driven as sonde_softin_dev_push_device drives k_softin_rs92 (tests/emu/softin_rs92_emu.cpp).  The arbiter is the host tier sonde_rs92_dec_push_soft with `-r -v`, and
`oracle/_ref/rs92mod --softin [-i] -r -v --ecc` live where that binary exists.  The same source is compiled by hipcc into k_softin_rs92; tests/test_gpu_softin_rs92.py
runs it there on the streams of tests/rs92_softin_cases.py.

A consumer has no `finish`: every stream ends with a short tail in which no header is found, so no frame is left in progress (the reference's partial frame at end
of input has no counterpart)."""
import ctypes as C
import os
import struct
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import golden_cases
import rs92_softin_cases as M

NAMES = sorted(M.cases())


@pytest.fixture(scope="module")
def emu():
    return M.load_emu()


@pytest.fixture(scope="module")
def host():
    return M.load_host()


def _arb(host, name):
    c = M.cases()[name]
    return M.host_frames(host, c["s"], c["inv"], c["softinv"], cache=name)


_one = {}


def _one_call(emu, name):
    if name not in _one:
        c = M.cases()[name]
        got, dropped, end = M.emu_frames(emu, c["s"], [len(c["s"])], c["inv"], c["softinv"])
        _one[name] = ([M.full(r) for r in got], dropped, M.state(end))
    return _one[name]


# ---------------------------------------------------------------- 1. every case in one call against the arbiter
@pytest.mark.parametrize("name", NAMES)
def test_case_equals_host_arbiter(emu, host, name):
    c = M.cases()[name]
    want = _arb(host, name)
    assert len(want) == c["n"]                                   # what the case is about, said by the arbiter
    if "ec" in c:
        assert [w[0] for w in want] == c["ec"]
    got, dropped, st = _one_call(emu, name)
    assert dropped == 0
    assert [(e if e >= 0 else -1, hb, fr) for e, hb, fr, _ in got] == [M.key(w) for w in want]
    assert [M.raw_line(fr, e) for e, _, fr, _ in got] == [w[3] for w in want]
    assert st[0] == 0 and st[1] == len(c["s"])                   # searching again, every symbol counted


def test_scores_of_the_quoted_windows(emu):
    """the scores the cases are built on, as the consumer records them: 1 for a clean header, 50 / 60 with five flips, 40 / sqrt(40 * 60) on the empty ring"""
    mv = lambda name: [struct.unpack("<f", r[3])[0] for r in _one_call(emu, name)[0]]        # noqa: E731
    assert mv("back_to_back") == [1.0, 1.0, 1.0]
    assert mv("flips_5") == [np.float32(50.0 / 60.0)]
    assert mv("empty_ring") == [1.0, np.float32(40.0 / np.sqrt(40.0 * 60.0)), np.float32(40.0 / np.sqrt(40.0 * 60.0))]
    assert all(m < -0.8 for m in mv("inverted_inv")) and all(m > 0.8 for m in mv("inverted_softinv"))


def test_one_call_is_longer_than_the_staging_buffer():
    assert len(M.cases()["back_to_back"]["s"]) > M.STAGE_MAX and len(M.cases()["empty_ring"]["s"]) > M.STAGE_MAX


def test_dropped_hit_leaves_an_empty_ring(emu, host):
    """the stream of the other polarity cut 25 symbols behind its last header: the ring is 35 zeros and those 25 symbols"""
    c = M.cases()["inverted_neither"]
    s = c["s"][:c["last_drop"] + 25]
    assert M.host_frames(host, s) == []
    for calls in ([len(s)], [61], [4800]):
        got, dropped, end = M.emu_frames(emu, s, calls)
        assert got == [] and dropped == 0 and end.mode == 0
        assert list(end.hist) == [0.0] * 35 + [float(v) for v in s[-25:]]


@pytest.mark.parametrize("name", NAMES)
def test_text_of_the_records_equals_host_tier_under_auto_rx_options(emu, host, tmp_path_factory, name):
    """what sonde_softin_dev_fetch_rs92 does with a channel's records — sonde_rs92_dec_corrected through one decoder, frame after frame — gives the text and JSON of
    `rs92mod -vx -v --crc --ecc --vel --json --ptu -e <rinex> --softin [-i]` over the stream"""
    c = M.cases()[name]
    E = M.rinex_file(tmp_path_factory.getbasetemp())
    want = M.host_text(host, c["s"], c["inv"], c["softinv"], ephemeris=E, version=b"t")
    d = M.host_dec(host, ephemeris=E, **dict(M.AUTORX, inv=c["inv"], version=b"t"))
    buf, text = C.create_string_buffer(2048), ""
    for ec, _, fr, _ in _one_call(emu, name)[0]:
        n = host.sonde_rs92_dec_corrected(d, fr, ec, buf, 2048)
        assert n >= 0                                          # (a frame whose config CRC fails prints nothing)
        text += buf.raw[:n].decode()
    host.sonde_rs92_dec_destroy(d)
    assert text == want
    assert text.count('"lat"') == sum(e >= 0 for e, _, _, _ in _one_call(emu, name)[0])


# ---------------------------------------------------------------- 2. call cuts
def _cut_run(emu, name, calls):
    c = M.cases()[name]
    got, dropped, end = M.emu_frames(emu, c["s"], calls, c["inv"], c["softinv"])
    return [M.full(r) for r in got], dropped, M.state(end)


def _all_streams(emu, calls_of):
    for name in NAMES:
        _one_call(emu, name)
    with ThreadPoolExecutor(max_workers=8) as pool:              # (the emulator keeps its fibers per thread; ctypes releases the interpreter lock)
        res = list(pool.map(lambda name: _cut_run(emu, name, calls_of(name)), NAMES))
    for name, r in zip(NAMES, res):
        assert r == _one_call(emu, name), name                   # records (mv bit for bit: the same operations), nothing dropped, the end state


@pytest.mark.parametrize("cut", M.CUTS)
def test_fixed_cuts_equal_one_call(emu, cut):
    _all_streams(emu, lambda name: [cut])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_cuts_equal_one_call(emu, seed):
    _all_streams(emu, lambda name: M.random_cuts(len(M.cases()[name]["s"]), 100 * seed + NAMES.index(name)))


def test_state_inside_a_frame_survives_any_cut(emu):
    """stopped inside a byte of a frame: the pending symbols, the position and the header's score are the same however the stream was cut"""
    c = M.cases()["errors_12"]
    s = c["s"][:21 + 120 + 20 * 100 + 13]
    want = M.emu_frames(emu, s, [len(s)])
    assert want[2].mode == 1 and want[2].carry_n == 13 and want[2].done == 2013
    assert list(want[2].carry)[:13] == [float(v) for v in s[-13:]]
    for calls in ([1], [19], [21], [60], M.random_cuts(len(s), 5, 1, 300)):
        got = M.emu_frames(emu, s, calls)
        assert M.state(got[2]) == M.state(want[2])


# ---------------------------------------------------------------- 3. the record cap
def test_record_cap_drops_and_the_next_call_is_intact(emu, host):
    rng = np.random.default_rng(9)
    first = M.cap_stream(22)
    s = np.concatenate([first, M.soft(M.fsym(23)), M.noise(rng, 80, 0.05)])
    want = M.host_frames(host, s, cache="cap")
    assert len(want) == 23 and all(w[0] == 0 for w in want)
    got, dropped, end = M.emu_frames(emu, s, [len(first), len(s) - len(first)], cap=20)
    assert dropped == 2 and len(got) == 21
    assert [M.key(r) for r in got] == [M.key(w) for w in want[:20] + want[22:]]
    assert end.mode == 0


def test_sanitized_standalone_replay_of_the_call_cuts(host, tmp_path):
    """the emulator translation unit under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program with its own main (tests/emu/softin_rs92_replay.cpp),
    run as a process of its own, outside the interpreter, in the environment as it is (the sanitizer runtimes are linked into the program).  The damaged frame in
    calls of 21 and 61 symbols, the empty-ring stream in one call above the staging limit and in calls of 4681, the inverted stream with -i, and 22 frames against
    20 slots."""
    exe = str(tmp_path / "softin_rs92_replay_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, os.path.join(M.EMU_DIR, "softin_rs92_replay.cpp"), M.EMU_SRC])
    runs = [("errors_12", 64, ["21"]), ("errors_12", 64, ["61"]), ("empty_ring", 64, [str(M.STAGE_MAX + 1), "4800"]), ("empty_ring", 64, ["4681"]), ("inverted_inv", 64, ["60"])]
    for name, cap, calls in runs:
        c = M.cases()[name]
        p = tmp_path / (name + ".f32")
        np.ascontiguousarray(c["s"], np.float32).tofile(p)
        r = subprocess.run([exe, str(p), str(int(c["softinv"])), str(c["inv"]), str(cap)] + calls, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert b"ERROR" not in r.stderr and b"runtime error" not in r.stderr
        assert r.stdout.decode().splitlines() == [w[3] for w in _arb(host, name)] and len(_arb(host, name)) == c["n"]
    s = np.concatenate([M.cap_stream(22), M.soft(M.fsym(23)), M.noise(np.random.default_rng(9), 80, 0.05)])
    p = tmp_path / "cap.f32"
    s.tofile(p)
    r = subprocess.run([exe, str(p), "0", "0", "20", str(22 * M.ONAIR), "4880"], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"ERROR" not in r.stderr and b"runtime error" not in r.stderr and b"21 frames, 2 dropped" in r.stderr
    want = M.host_frames(host, s, cache="cap")
    assert r.stdout.decode().splitlines() == [w[3] for w in want[:20] + want[22:]]


# ---------------------------------------------------------------- 4. the end-of-frame step alone
def test_ecc_step_equals_host_decoder_on_200_frames(emu, host):
    """codeword layout, syndromes, decode and write-back on frames with 0..14 byte errors anywhere in bytes 6..239: the `-r -v` line of sonde_rs92_dec_bytes on the
    uncorrected frame, byte for byte, verdict included"""
    rng = np.random.default_rng(2024)
    h = M.host_dec(host, raw=1, verbose=1)
    buf = C.create_string_buffer(1024)
    seen = set()
    for k in range(200):
        f = bytearray(M.frames()[k % 24])
        nerr = k % 15
        for p in rng.choice(np.arange(6, 240), nerr, replace=False):
            f[int(p)] ^= int(rng.integers(1, 256))
        n = host.sonde_rs92_dec_bytes(h, bytes(f), 240, buf, 1024)
        assert n > 0
        want = buf.raw[:n].decode().rstrip("\n")
        g = C.create_string_buffer(bytes(f), 240)
        ec = emu.emu_rs92_ecc(g)
        assert M.raw_line(g.raw, ec) == want, (k, nerr, ec)
        assert ec == nerr if nerr <= 12 else True
        seen.add(ec if ec >= 0 else -1)
    host.sonde_rs92_dec_destroy(h)
    assert seen >= set(range(13)) | {-1}


# ---------------------------------------------------------------- 5. the compiled reference, live
@pytest.mark.parametrize("name", NAMES)
def test_case_equals_compiled_reference(emu, name):
    if not golden_cases.need_ref():
        return
    c = M.cases()[name]
    args = [M.REF, "--softinv" if c["softinv"] else "--softin"] + (["-i"] if c["inv"] else []) + ["-r", "-v", "--ecc"]
    r = subprocess.run(args, input=np.ascontiguousarray(c["s"], np.float32).tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0
    ref = [l.rstrip() for l in r.stdout.decode().splitlines() if l.strip()]
    got, _, _ = _one_call(emu, name)
    assert [M.raw_line(fr, e).rstrip() for e, _, fr, _ in got] == ref
