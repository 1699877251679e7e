"""The DEVICE MRZ soft-bit consumer (radiosonde_auto_rx_amd/csrc/sonde_softin_mrz_dev.h: header search at 0.82 with the polarity rule and the ring left as it is,
Manchester bits on a lane per bit packed by ballot, bytes, frame type and CRC-16 on the wave, the next frame's length from the verdict) executed on the CPU under
tests/emu/wave_emu.h and driven as sonde_softin_dev_push_device drives k_softin_mrz (tests/emu/softin_mrz_emu.cpp).  The arbiter is the host tier
sonde_mrz_dec_push_soft with `-r` (`-R` where a case says so), and `oracle/_ref/mp3h1mod --softin -r` live where that binary exists.  The same source is compiled
by hipcc into k_softin_mrz; tests/test_gpu_softin_mrz.py runs it there on the streams of tests/mrz_softin_cases.py.

A consumer has no `finish`: every stream ends with a short tail in which no header is found, so no frame is left in progress."""
import ctypes as C
import os
import struct
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import golden_cases
import mrz_softin_cases as M

NAMES = sorted(M.case_opts())                              # (the streams are built inside the tests: nothing loads the library at collection)
F082 = M.F082


@pytest.fixture(scope="module")
def emu():
    return M.load_emu()


@pytest.fixture(scope="module")
def host():
    return M.load_host()


def _arb(host, name):
    c = M.cases()[name]
    return M.host_frames(host, c["s"], cache=name, **M.opts(c))


_one = {}


def _one_call(emu, name):
    if name not in _one:
        c = M.cases()[name]
        got, dropped, end = M.emu_frames(emu, c["s"], [len(c["s"])], **M.opts(c))
        _one[name] = (got, [M.full(r) for r in got], dropped, M.state(end), end)
    return _one[name]


def test_header_mask_is_the_header(emu):
    assert emu.emu_mrz_header_mask() == sum(int(ch) << i for i, ch in enumerate(M.HEADER))


# ---------------------------------------------------------------- 1. every case in one call against the arbiter
@pytest.mark.parametrize("name", NAMES)
def test_case_equals_host_arbiter(emu, host, name):
    c = M.cases()[name]
    want = _arb(host, name)
    assert len(want) == c["n"]                                   # what the case is about, said by the arbiter
    assert [w[1] for w in want] == c["nbits"] and [w[4] for w in want] == c["ok"]
    got, _, dropped, st, end = _one_call(emu, name)
    assert dropped == 0
    assert [M.key(r) for r in got] == [M.key(w) for w in want]   # hdr_bit, nbits, polarity, the bits, the verdict, crclen
    assert [M.raw_line(r, c["ofs"], c["raw2"]) for r in got] == [w[6] for w in want]
    for r in got:                                                # the score the reference computes over its ring at the hit, bit for bit
        assert struct.pack("<f", r.mv) == struct.pack("<f", M.ref_score(M.ring_at(c["s"], want, r.hdr_bit, c["softinv"])))
        if not c["raw2"]:
            fr, _ = M.frame_bytes(np.unpackbits(np.frombuffer(bytes(r.bits), np.uint8)), r.nbits, 8 if c["ofs"] is None else c["ofs"])
            assert (r.crclen, r.crcval, r.crcdat, r.crc_ok) == M.verdict(fr)
    assert st[0] == 0 and st[3] == len(c["s"])                   # searching again, every half symbol counted
    assert [struct.pack("<f", v) for v in end.hist] == [struct.pack("<f", v) for v in M.ring_at(c["s"], want, len(c["s"]), c["softinv"])]
    assert end.bitfrm_len == ([408] + [(w[5] + 6) * 8 for w in want if w[4]])[-1]


def test_scores_at_the_threshold(emu, host):
    """36 / 44 is not found; one half symbol's amplitude a float apart decides within 1e-3 of 0.82; a score of exactly 0.82f is no hit; exact zeros are 0 / 0"""
    mv = lambda name: [r.mv for r in _one_call(emu, name)[0]]    # noqa: E731
    assert [abs(m) for m in mv("clean_ecef")] == [1.0, 1.0, 1.0]
    cs = M.cases()
    un, ex, ab = cs["edge_under"], cs["edge_exact"], cs["edge_above"]
    assert np.nextafter(np.float32(ex["amp"]), np.float32(2)) == np.float32(ab["amp"]) and un["amp"] < ex["amp"]
    a, e, b = (M.ref_score(x["s"][M.EDGE_LEAD:M.EDGE_LEAD + 44]) for x in (un, ex, ab))
    assert a < F082 and e == F082 and b > F082 and F082 - a < 1e-3 and b - F082 < 1e-3
    assert b == np.nextafter(F082, np.float32(1)) and a == np.nextafter(F082, np.float32(0))      # one float apart on both sides
    assert mv("edge_under") == [] and mv("edge_exact") == [] and mv("edge_above") == [b]
    assert np.isnan(M.ref_score(np.zeros(44, np.float32)))


def test_polarity_rule(emu, host):
    """the inverted stream: nothing without -i or --auto; with -i and with --softinv the same bits, the scores of opposite sign; --auto flips once, at the first
    hit, and stays flipped in the calls behind it"""
    inv, sinv, aut = (_one_call(emu, n)[0] for n in ("inverted_i", "inverted_softinv", "inverted_auto"))
    assert _one_call(emu, "inverted_plain")[0] == [] and len(inv) == 2
    assert [r.mv for r in inv] == [-r.mv for r in sinv] == [r.mv for r in aut] and all(r.mv < -F082 for r in inv)
    assert [M.key(r)[3:] for r in inv] == [M.key(r)[3:] for r in sinv] == [M.key(r)[3:] for r in aut]
    assert [r.inv for r in inv] == [1, 1] and [r.inv for r in sinv] == [0, 0] and [r.inv for r in aut] == [1, 1]
    c = M.cases()["inverted_auto"]
    hb = [w[0] for w in _arb(host, "inverted_auto")]
    assert _one_call(emu, "inverted_plain")[4].inv == 0 and _one_call(emu, "inverted_auto")[4].inv == 1
    got, _, end = M.emu_frames(emu, c["s"], [hb[0] + 100, hb[1] - hb[0], len(c["s"])], **M.opts(c))
    assert [M.full(r) for r in got] == _one_call(emu, "inverted_auto")[1] and end.inv == 1
    _, _, end = M.emu_frames(emu, c["s"][:hb[0] - 1], [hb[0] - 1], **M.opts(c))
    assert end.inv == 0                                           # not before the hit


def test_dropped_hit_leaves_the_ring_running(emu, host):
    c = M.cases()["dropped_then_true"]
    at, true_at = c["at"], c["true_at"]
    assert M.ref_score(c["s"][at - 44:at]) < -F082                # the hit that is dropped
    assert [q for q in range(44, true_at) if abs(M.ref_score(c["s"][q - 44:q])) > F082] == [at]       # and no other window in front of the true header
    assert true_at - 44 < at and (at - 1) // 64 == (true_at - 1) // 64       # the true header begins inside its window; both positions in one round of 64
    want = _arb(host, "dropped_then_true")
    assert [w[0] for w in want] == [true_at] and want[0][4] == 1
    got = _one_call(emu, "dropped_then_true")[0]
    assert [r.hdr_bit for r in got] == [true_at] and got[0].mv == M.ref_score(c["s"][true_at - 44:true_at]) > F082
    # with the ring emptied or stopped at the dropped hit the true header is not found
    assert not M.ref_score(np.concatenate([np.zeros(at - (true_at - 44), np.float32), c["s"][at:true_at]])) > F082


def test_equal_halves_decide_bits(emu, host):
    """the case is about something: with s = +-0 read as negative (the `>` mutation), or the halves swapped, other bits come out"""
    for name, inv in (("equal_halves", 0), ("equal_halves_inv", 1)):
        c = M.cases()[name]
        w = _arb(host, name)[0]
        sym = c["s"][w[0]:w[0] + 772]
        d = (sym[1::2] - sym[0::2]).astype(np.float32)
        assert (d == 0).sum() >= 30 and any(np.signbit(v) for v in d[d == 0]) and any(not np.signbit(v) for v in d[d == 0])
        bits = M.manchester(sym, inv)
        assert list(bits) != list(((d > 0).astype(np.uint8)) ^ (0 if inv else 1))
        assert list(bits) != list(M.manchester(sym[np.arange(772) ^ 1], inv))
        assert w[2] == inv


def test_one_call_longer_than_the_staging_buffer_and_the_two_lengths_around_it(emu, host):
    s = M.long_stream()
    assert len(s) > M.STAGE_MAX + 1
    want = M.host_frames(host, s, cache="long")
    assert len(want) == 16 and [w[1] for w in want] == [408] * 5 + [384] * 11
    one = M.emu_frames(emu, s, [len(s)])
    assert [M.key(r) for r in one[0]] == [M.key(w) for w in want]
    for first in (M.STAGE_MAX, M.STAGE_MAX + 1):
        got = M.emu_frames(emu, s, [first, len(s) - first])
        assert [M.full(r) for r in got[0]] == [M.full(r) for r in one[0]] and M.state(got[2]) == M.state(one[2]) and got[1] == 0


# ---------------------------------------------------------------- 2. the ring
def test_ring_after_an_accepted_header_is_that_header(emu, host):
    c = M.cases()["inverted_softinv"]
    hb = _arb(host, "inverted_softinv")[0][0]
    s = c["s"][:hb + 555]
    for calls in ([len(s)], [45], [hb, 7]):
        _, _, end = M.emu_frames(emu, s, calls, **M.opts(c))
        assert end.mode == 1 and end.done == 555 and end.hdr_bit == hb
        assert [float(v) for v in end.hist] == [float(-v) for v in s[hb - 44:hb]]
        assert float(end.carry) == float(-s[-1])                 # the pending odd half symbol


def test_hit_right_behind_a_frame_depends_on_the_ring_the_header_left(emu, host):
    """K half symbols behind the frame complete the (partly silent) header in the ring to a second hit; the frame's last half symbols in its place, or zeros, give none"""
    c = M.cases()["ring_behind_frame"]
    want = _arb(host, "ring_behind_frame")
    assert [w[0] for w in want] == [56, c["at"] + c["K"]]
    got = _one_call(emu, "ring_behind_frame")[0]
    assert [r.hdr_bit for r in got] == [56, c["at"] + c["K"]]
    y = c["s"][c["at"]:c["at"] + c["K"]]
    ring = np.concatenate([c["s"][12:56][c["K"]:], y])
    assert got[1].mv == M.ref_score(ring) and abs(got[1].mv) > F082
    assert not abs(M.ref_score(np.concatenate([c["s"][c["at"] - 44 + c["K"]:c["at"]], y]))) > F082
    assert not abs(M.ref_score(np.concatenate([np.zeros(44 - c["K"], np.float32), y]))) > F082


# ---------------------------------------------------------------- 3. call cuts
def _cut_run(emu, name, calls):
    c = M.cases()[name]
    got, dropped, end = M.emu_frames(emu, c["s"], calls, **M.opts(c))
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


def test_length_switch_across_calls_and_cuts_on_headers_frame_ends_and_odd_half_symbols(emu, host):
    """calls that end with a header's last half symbol, with a frame's last (the verdict of one call sets the length the next call reads with), one half symbol to
    either side of both, and on an odd half symbol of a frame"""
    for name in ("switch", "switch_back", "clean_latlon", "sigma03"):
        c = M.cases()[name]
        want = _arb(host, name)
        one = _one_call(emu, name)
        for w in want[:3]:
            hb, end_ = w[0], w[0] + 2 * (w[1] - 22)
            for first in (hb - 1, hb, hb + 1, end_ - 1, end_, end_ + 1, hb + 333):
                assert _cut_run(emu, name, [first, len(c["s"])]) == (one[1], one[2], one[3]), (name, first)
        ends = [w[0] + 2 * (w[1] - 22) for w in want]
        calls = [ends[0]] + [b - a for a, b in zip(ends, ends[1:])] + [len(c["s"])]
        assert _cut_run(emu, name, calls) == (one[1], one[2], one[3]), name       # a frame a call: every switch happens between calls
        assert _cut_run(emu, name, [want[0][0] + 5, 3, 1, 1, 64, 129, len(c["s"])]) == (one[1], one[2], one[3]), name


def test_state_inside_a_bit_survives_any_cut(emu, host):
    c = M.cases()["sigma03"]
    hb = _arb(host, "sigma03")[0][0]
    s = c["s"][:hb + 2 * 200 + 1]
    want = M.emu_frames(emu, s, [len(s)])
    assert want[2].mode == 1 and want[2].done == 401 and float(want[2].carry) == float(s[-1])
    for calls in ([1], [2], [3], [43], [64], [65], M.random_cuts(len(s), 5, 1, 300)):
        got = M.emu_frames(emu, s, calls)
        assert M.state(got[2]) == M.state(want[2]), calls


# ---------------------------------------------------------------- 4. the record cap
def test_capacity_2_with_5_frames_and_the_switch_behind_a_dropped_frame(emu, host):
    first, second = M.cap_streams()
    s = np.concatenate([first, second])
    want = M.host_frames(host, s, cache="cap")
    assert len(want) == 6 and [w[1] for w in want] == [408, 408, 408, 384, 384, 384] and all(w[4] for w in want)
    got, dropped, end = M.emu_frames(emu, s, [len(first), len(second)], cap=2)
    assert dropped == 3 and len(got) == 3
    assert [M.key(r) for r in got] == [M.key(w) for w in want[:2] + want[5:]]
    assert got[2].nbits == 384 and got[2].crc_ok == 1 and end.mode == 0 and end.bitfrm_len == 384


# ---------------------------------------------------------------- 5. the CRC on the wave
def _crc(emu, fr51):
    out = (C.c_int * 4)()
    assert emu.emu_mrz_crc(bytes(fr51), out) == 0
    return tuple(out)


def test_crc_on_the_wave_every_single_bit_flip_of_8_random_frames_of_each_length(emu):
    """8 random frames of each type (42 and 45 bytes under the CRC): the frame as it is passes, and every single-bit flip of the covered bytes and of the stored
    word gives the serial CRC's value and verdict"""
    rng = np.random.default_rng(4245)
    for crclen in (42, 45):
        for _ in range(8):
            f = bytearray(rng.integers(0, 256, 51, dtype=np.uint8).tobytes())
            f[30:32] = b"\xff\xff" if crclen == 42 else b"\x12\xff"
            f[3 + crclen:5 + crclen] = M.crc16rev(f[3:3 + crclen]).to_bytes(2, "little")
            assert _crc(emu, f) == M.verdict(f) and M.verdict(f)[0] == crclen and M.verdict(f)[3] == 1
            for bit in range(8 * 3, 8 * (crclen + 5)):
                g = bytearray(f); g[bit >> 3] ^= 0x80 >> (bit & 7)
                got = _crc(emu, g)
                assert got == M.verdict(g), (crclen, bit)
                assert got[3] == 0 or got[0] != crclen            # (a flip in bytes 30 / 31 changes the frame type; everything else fails)
    assert _crc(emu, bytes(51)) == M.verdict(bytes(51))            # all zero: the start value alone


# ---------------------------------------------------------------- 6. a stand-alone program under the sanitizers
def test_sanitized_standalone_replay_of_the_call_cuts(host, tmp_path):
    """the emulator translation unit under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program with its own main (tests/emu/softin_mrz_replay.cpp),
    run as a process of its own, outside the interpreter, in the environment as it is (the sanitizer runtimes are linked into the program)"""
    exe = str(tmp_path / "softin_mrz_replay_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, os.path.join(M.EMU_DIR, "softin_mrz_replay.cpp"), M.EMU_SRC])

    def run(s, c, cap, calls):
        p = tmp_path / "s.f32"
        np.ascontiguousarray(s, np.float32).tofile(p)
        args = [int(c["softinv"]), int(c["inv"]), int(c["aut"]), int(c["raw2"]), 8 if c["ofs"] is None else c["ofs"], cap]
        r = subprocess.run([exe, str(p)] + [str(a) for a in args] + calls, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert b"ERROR" not in r.stderr and b"runtime error" not in r.stderr
        return r

    for name, calls in [("switch_back", ["1"]), ("sigma03", ["43"]), ("inverted_auto", ["65"]), ("ofs_64", ["251"]), ("raw2_never_switches", ["1000"])]:
        c = M.cases()[name]
        r = run(c["s"], c, 64, calls)
        assert r.stdout.decode().splitlines() == [w[6] for w in _arb(host, name)] and len(_arb(host, name)) == c["n"], name
    s = M.long_stream()
    r = run(s, M.case_opts()["clean_ecef"], 64, [str(M.STAGE_MAX + 1), "2400"])
    assert r.stdout.decode().splitlines() == [w[6] for w in M.host_frames(host, s, cache="long")]
    first, second = M.cap_streams()
    r = run(np.concatenate([first, second]), M.case_opts()["clean_ecef"], 2, [str(len(first)), "2400"])
    assert b"3 frames, 3 dropped" in r.stderr


# ---------------------------------------------------------------- 7. the compiled reference, live
@pytest.mark.parametrize("name", NAMES)
def test_case_equals_compiled_reference(emu, name):
    if not golden_cases.need_ref():
        return
    c = M.cases()[name]
    args = [M.REF, "--softinv" if c["softinv"] else "--softin", "-R" if c["raw2"] else "-r"] + (["-i"] if c["inv"] else []) + (["--auto"] if c["aut"] else [])
    if c["ofs"] is not None:
        args += ["--ofs", str(c["ofs"])]
    r = subprocess.run(args, input=np.ascontiguousarray(c["s"], np.float32).tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0
    ref = [l.rstrip() for l in r.stdout.decode().splitlines() if l.strip()]
    got = _one_call(emu, name)[0]
    assert [M.raw_line(r_, c["ofs"], c["raw2"]).rstrip() for r_ in got][:c.get("ref_n")] == ref      # (ref_n: the reference program ends at a switch back to 408)
