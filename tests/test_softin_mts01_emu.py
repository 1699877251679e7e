"""The DEVICE MTS01 soft-bit consumer (radiosonde_auto_rx_amd/csrc/sonde_softin_mts01_dev.h: header search at 0.8 in either polarity with the ring left as it is, a
bit per symbol on a lane per bit packed by ballot, the 131 bytes and the CRC-16 on the wave) executed on the CPU under tests/emu/wave_emu.h and driven as
sonde_softin_dev_push_device drives k_softin_mts01 (tests/emu/softin_mts01_emu.cpp).  The arbiter is the host tier sonde_mts01_dec_push_soft with `-r`, and
`oracle/_ref/mts01mod --softin -r` live where that binary exists.  The same source is compiled by hipcc into k_softin_mts01; tests/test_gpu_softin_mts01.py runs it
there on the streams of tests/mts01_softin_cases.py.

A consumer has no `finish`: every stream ends with a short tail in which no header is found, so no frame is left in progress."""
import ctypes as C
import os
import struct
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import golden_cases
import mts01_softin_cases as M

NAMES = sorted(M.case_opts())                              # (the streams are built inside the tests: nothing loads the library at collection)
F08 = M.F08


@pytest.fixture(scope="module")
def emu():
    return M.load_emu()


@pytest.fixture(scope="module")
def host():
    return M.load_host()


def _arb(host, name):
    c = M.cases()[name]
    return M.host_frames(host, c["s"], c["softinv"], cache=name)


_one = {}


def _one_call(emu, name):
    if name not in _one:
        c = M.cases()[name]
        got, dropped, end = M.emu_frames(emu, c["s"], [len(c["s"])], c["softinv"])
        _one[name] = (got, [M.full(r) for r in got], dropped, M.state(end), end)
    return _one[name]


def test_header_mask_is_the_header(emu):
    assert emu.emu_mts01_header_mask() == sum(int(ch) << i for i, ch in enumerate(M.HEADER))


# ---------------------------------------------------------------- 1. every case in one call against the arbiter
@pytest.mark.parametrize("name", NAMES)
def test_case_equals_host_arbiter(emu, host, name):
    c = M.cases()[name]
    want = _arb(host, name)
    assert len(want) == c["n"] and [w[4] for w in want] == c["ok"]      # what the case is about, said by the arbiter
    got, _, dropped, st, end = _one_call(emu, name)
    assert dropped == 0
    assert [M.key(r) for r in got] == [M.key(w) for w in want]   # hdr_bit, the 131 bytes, crcval, crcdat, the verdict
    assert [M.raw_line(r) for r in got] == [w[5] for w in want]
    hbs = [w[0] for w in want]
    for r in got:                                                # the score the reference computes over its ring at the hit, bit for bit
        assert struct.pack("<f", r.mv) == struct.pack("<f", M.ref_score(M.ring_at(c["s"], hbs, r.hdr_bit, c["softinv"])))
    assert st[0] == 0 and st[1] == len(c["s"])                   # searching again, every symbol counted
    assert [struct.pack("<f", v) for v in end.hist] == [struct.pack("<f", v) for v in M.ring_at(c["s"], hbs, len(c["s"]), c["softinv"])]


def test_scores_at_the_threshold_and_in_both_polarities(emu, host):
    """one symbol's amplitude a float apart decides within 1e-3 of 0.8; a score of exactly 0.8f is no hit; exact zeros are 0 / 0; the inverted stream is found
    with a negative score, its bits are the complement and its CRC fails; --softinv gives sign, bits and CRC back"""
    mv = lambda name: [r.mv for r in _one_call(emu, name)[0]]    # noqa: E731
    assert mv("clean") == [1.0, 1.0, 1.0]
    cs = M.cases()
    un, ex, ab = cs["edge_under"], cs["edge_exact"], cs["edge_above"]
    assert np.nextafter(np.float32(ex["amp"]), np.float32(2)) == np.float32(ab["amp"]) and un["amp"] < ex["amp"]
    a, e, b = (M.ref_score(x["s"][M.EDGE_LEAD:M.EDGE_LEAD + 32]) for x in (un, ex, ab))
    assert a < F08 and e == F08 and b > F08 and F08 - a < 1e-3 and b - F08 < 1e-3
    assert b == np.nextafter(F08, np.float32(1)) and a == np.nextafter(F08, np.float32(0))      # one float apart on both sides
    assert mv("edge_under") == [] and mv("edge_exact") == [] and mv("edge_above") == [b]
    assert np.isnan(M.ref_score(np.zeros(32, np.float32)))
    inv, sinv = _one_call(emu, "inverted")[0], _one_call(emu, "inverted_softinv")[0]
    assert len(inv) == 2 and [r.mv for r in inv] == [-r.mv for r in sinv] and all(r.mv < -F08 for r in inv)
    assert [bytes(r.bytes) for r in inv] == [bytes(v ^ 0xFF for v in r.bytes) for r in sinv]
    assert [r.crc_ok for r in inv] == [0, 0] and [r.crc_ok for r in sinv] == [1, 1]


def test_text_without_a_nul_with_an_early_one_byte_0_and_zeros(emu, host):
    by = lambda name: bytes(_one_call(emu, name)[0][0].bytes)    # noqa: E731
    assert 0 not in by("no_nul")[1:129] and by("early_nul")[10] == 0 and by("byte0_changed")[0] == 0x3C
    assert _one_call(emu, "byte0_changed")[0][0].crc_ok == 1      # byte 0 is not under the CRC
    c = M.cases()["zero_symbols"]
    hb = _arb(host, "zero_symbols")[0][0]
    sym = c["s"][hb:hb + M.NSYM]
    assert (sym == 0).sum() > 40 and any(np.signbit(v) for v in sym[sym == 0]) and any(not np.signbit(v) for v in sym[sym == 0])
    assert bytes(np.packbits(sym >= 0)) == by("zero_symbols") != bytes(np.packbits(sym > 0))       # the `>` mutation gives other bits


def test_one_call_longer_than_the_staging_buffer_and_the_two_lengths_around_it(emu, host):
    s = M.long_stream()
    assert len(s) > M.STAGE_MAX + 1
    want = M.host_frames(host, s, cache="long")
    assert len(want) == 12
    one = M.emu_frames(emu, s, [len(s)])
    assert [M.key(r) for r in one[0]] == [M.key(w) for w in want]
    for first in (M.STAGE_MAX, M.STAGE_MAX + 1):
        got = M.emu_frames(emu, s, [first, len(s) - first])
        assert [M.full(r) for r in got[0]] == [M.full(r) for r in one[0]] and M.state(got[2]) == M.state(one[2]) and got[1] == 0


# ---------------------------------------------------------------- 2. the ring
def test_ring_after_a_header_is_that_header(emu, host):
    c = M.cases()["inverted_softinv"]
    hb = _arb(host, "inverted_softinv")[0][0]
    s = c["s"][:hb + 777]
    for calls in ([len(s)], [33], [hb, 7]):
        _, _, end = M.emu_frames(emu, s, calls, True)
        assert end.mode == 1 and end.done == 777 and end.hdr_bit == hb
        assert [float(v) for v in end.hist] == [float(-v) for v in s[hb - 32:hb]]


def test_hit_right_behind_a_frame_depends_on_the_ring_the_header_left(emu, host):
    """K symbols behind the frame complete the (partly silent) header in the ring to a second hit; the frame's last symbols in its place, or zeros, give none"""
    c = M.cases()["ring_behind_frame"]
    want = _arb(host, "ring_behind_frame")
    assert [w[0] for w in want] == [44, c["at"] + c["K"]]
    got = _one_call(emu, "ring_behind_frame")[0]
    assert [r.hdr_bit for r in got] == [44, c["at"] + c["K"]]
    y = c["s"][c["at"]:c["at"] + c["K"]]
    ring = np.concatenate([c["s"][12:44][c["K"]:], y])
    assert got[1].mv == M.ref_score(ring) and abs(got[1].mv) > F08
    assert not abs(M.ref_score(np.concatenate([c["s"][c["at"] - 32 + c["K"]:c["at"]], y]))) > F08
    assert not abs(M.ref_score(np.concatenate([np.zeros(32 - c["K"], np.float32), y]))) > F08


# ---------------------------------------------------------------- 3. call cuts
def _cut_run(emu, name, calls):
    c = M.cases()[name]
    got, dropped, end = M.emu_frames(emu, c["s"], calls, c["softinv"])
    return [M.full(r) for r in got], dropped, M.state(end)


def _all_streams(emu, calls_of):
    for name in NAMES:
        _one_call(emu, name)
    with ThreadPoolExecutor(max_workers=8) as pool:              # (the emulator keeps its fibers per thread; ctypes releases the interpreter lock)
        res = list(pool.map(lambda name: _cut_run(emu, name, calls_of(name)), NAMES))
    for name, r in zip(NAMES, res):
        one = _one_call(emu, name)
        assert r == (one[1], one[2], one[3]), name               # records (mv bit for bit: the same operations), nothing dropped, the end state


@pytest.mark.parametrize("cut", M.CUTS)
def test_fixed_cuts_equal_one_call(emu, cut):
    _all_streams(emu, lambda name: [cut])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_cuts_equal_one_call(emu, seed):
    _all_streams(emu, lambda name: M.random_cuts(len(M.cases()[name]["s"]), 100 * seed + NAMES.index(name)))


def test_cuts_on_the_headers_and_the_frames_last_symbol(emu, host):
    for name in ("clean", "back_to_back", "sigma03"):
        c = M.cases()[name]
        hb = _arb(host, name)[0][0]
        one = _one_call(emu, name)
        for first in (hb - 1, hb, hb + 1, hb + M.NSYM - 1, hb + M.NSYM, hb + M.NSYM + 1, hb + 333):
            if first < 1:
                continue
            assert _cut_run(emu, name, [first, len(c["s"])]) == (one[1], one[2], one[3]), (name, first)
        assert _cut_run(emu, name, [hb + 5, 3, 1, 1, 64, 129, len(c["s"])]) == (one[1], one[2], one[3]), name


# ---------------------------------------------------------------- 4. the record cap
def _cap_stream():
    rng = np.random.default_rng(9)
    first = M.cap_stream(5)
    return first, np.concatenate([first, M.soft(M.onair([M.fbits(50)], lead=0)), M.noise(rng, 80, 0.05)])


def test_record_cap_drops_and_the_next_call_is_intact(emu, host):
    first, s = _cap_stream()
    want = M.host_frames(host, s, cache="cap")
    assert len(want) == 6 and all(w[4] for w in want)
    got, dropped, end = M.emu_frames(emu, s, [len(first), len(s) - len(first)], cap=3)
    assert dropped == 2 and len(got) == 4
    assert [M.key(r) for r in got] == [M.key(w) for w in want[:3] + want[5:]]
    assert end.mode == 0


# ---------------------------------------------------------------- 5. the CRC on the wave
def _crc(emu, by131):
    out = (C.c_int * 3)()
    assert emu.emu_mts01_crc(bytes(by131), out) == 0
    return tuple(out)


def test_crc_on_the_wave_every_single_bit_flip_of_8_random_frames(emu):
    """8 random frames: the frame as it is passes, every single-bit flip of the 128 covered bytes and of the stored word gives the serial CRC's value and a failing
    verdict, and a flip in byte 0 changes nothing"""
    rng = np.random.default_rng(128)
    for _ in range(8):
        f = bytearray(rng.integers(0, 256, 131, dtype=np.uint8).tobytes())
        re = M.crc16_re(f[1:129])
        f[129], f[130] = re & 0xFF, re >> 8
        assert _crc(emu, f) == M.verdict(f) and M.verdict(f)[2] == 1
        for bit in range(8 * 131):
            g = bytearray(f); g[bit >> 3] ^= 0x80 >> (bit & 7)
            got = _crc(emu, g)
            assert got == M.verdict(g) and got[2] == (1 if bit < 8 else 0), bit
    assert _crc(emu, bytes(131)) == M.verdict(bytes(131))          # all zero: the start value alone
    assert M.crc16_re(bytes(128)) != M.crc16_re(bytes(128), init=0)


# ---------------------------------------------------------------- 6. a stand-alone program under the sanitizers
def test_sanitized_standalone_replay_of_the_call_cuts(host, tmp_path):
    """the emulator translation unit under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program with its own main (tests/emu/softin_mts01_replay.cpp),
    run as a process of its own, outside the interpreter, in the environment as it is (the sanitizer runtimes are linked into the program)"""
    exe = str(tmp_path / "softin_mts01_replay_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, os.path.join(M.EMU_DIR, "softin_mts01_replay.cpp"), M.EMU_SRC])

    def run(s, softinv, cap, calls):
        p = tmp_path / "s.f32"
        np.ascontiguousarray(s, np.float32).tofile(p)
        r = subprocess.run([exe, str(p), str(int(softinv)), str(cap)] + calls, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert b"ERROR" not in r.stderr and b"runtime error" not in r.stderr
        return r

    for name, calls in [("sigma03", ["1"]), ("back_to_back", ["1080"]), ("back_to_back", ["1081"]), ("inverted_softinv", ["31"]), ("ring_behind_frame", ["9"]),
                        ("zero_symbols", ["65"])]:
        c = M.cases()[name]
        r = run(c["s"], c["softinv"], 64, calls)
        assert r.stdout.decode().splitlines() == [w[5] for w in _arb(host, name)] and len(_arb(host, name)) == c["n"], name
    s = M.long_stream()
    r = run(s, False, 64, [str(M.STAGE_MAX + 1), "2400"])
    assert r.stdout.decode().splitlines() == [w[5] for w in M.host_frames(host, s, cache="long")]
    first, s = _cap_stream()
    r = run(s, False, 3, [str(len(first)), "2400"])
    assert b"4 frames, 2 dropped" in r.stderr


# ---------------------------------------------------------------- 7. the compiled reference, live
@pytest.mark.parametrize("name", NAMES)
def test_case_equals_compiled_reference(emu, name):
    if not golden_cases.need_ref():
        return
    c = M.cases()[name]
    r = subprocess.run([M.REF, "--softinv" if c["softinv"] else "--softin", "-r"], input=np.ascontiguousarray(c["s"], np.float32).tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0
    ref = [l.rstrip() for l in r.stdout.decode().splitlines() if l.strip()]
    got = _one_call(emu, name)[0]
    assert [M.raw_line(r_).rstrip() for r_ in got] == ref
