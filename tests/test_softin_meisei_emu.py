"""The DEVICE Meisei soft-bit consumer (radiosonde_auto_rx_amd/csrc/sonde_softin_meisei_dev.h: header search at 0.8 in either polarity with the ring left as it is,
biphase-S bits on a lane per bit packed by ballot, the 12 BCH(63,51) blocks with the padding and word-parity rules one at a time on the wave) executed on the CPU
under tests/emu/wave_emu.h and driven as sonde_softin_dev_push_device drives k_softin_meisei (tests/emu/softin_meisei_emu.cpp).  The arbiter is the host tier
sonde_meisei_dec_push_soft with `-r --ecc -v` (`-r -v` where a case has --ecc off), and `oracle/_ref/meisei100mod --softin -r --ecc -v` live where that binary
exists.  The same source is compiled by hipcc into k_softin_meisei; tests/test_gpu_softin_meisei.py runs it there on the streams of tests/meisei_softin_cases.py.

A consumer has no `finish`: every stream ends with a short tail in which no header is found, so no frame is left in progress."""
import ctypes as C
import os
import struct
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import golden_cases
import meisei_softin_cases as M

NAMES = sorted(M.case_opts())                              # (the streams are built inside the tests: nothing loads the library at collection)
STREAMS = M.stream_names()
F08 = M.F08


@pytest.fixture(scope="module")
def emu():
    return M.load_emu()


@pytest.fixture(scope="module")
def host():
    return M.load_host()


def _opts(c):
    return dict(softinv=c["softinv"], ecc=c["ecc"])


def _arb(host, name):
    c = M.cases()[name]
    return M.host_frames(host, c["s"], cache=name, **_opts(c))


_one = {}


def _one_call(emu, name):
    if name not in _one:
        c = M.cases()[name]
        got, dropped, end = M.emu_frames(emu, c["s"], [len(c["s"])], **_opts(c))
        _one[name] = (got, [M.full(r) for r in got], dropped, M.state(end), end)
    return _one[name]


def test_header_mask_is_the_header(emu):
    assert emu.emu_meisei_header_mask() == sum(int(ch) << i for i, ch in enumerate(M.HEADER))


# ---------------------------------------------------------------- 1. every case in one call against the arbiter
@pytest.mark.parametrize("name", NAMES)
def test_case_equals_host_arbiter(emu, host, name):
    c = M.cases()[name]
    want = _arb(host, name)
    assert len(want) == c["n"]                                   # what the case is about, said by the arbiter
    got, _, dropped, st, end = _one_call(emu, name)
    assert dropped == 0
    assert [M.key(r) for r in got] == [M.key(w) for w in want]   # hdr_bit, the 600 bits, the 12 verdicts
    assert [M.raw_line(r, c["ecc"]) for r in got] == [w[3] for w in want]
    hbs = [w[0] for w in want]
    for r in got:                                                # the score the reference computes over its ring at the hit, bit for bit
        assert struct.pack("<f", r.mv) == struct.pack("<f", M.ref_score(M.ring_at(c["s"], hbs, r.hdr_bit, c["softinv"])))
    assert st[0] == 0 and st[1] == len(c["s"])                   # searching again, every half symbol counted
    assert [struct.pack("<f", v) for v in end.hist] == [struct.pack("<f", v) for v in M.ring_at(c["s"], hbs, len(c["s"]), c["softinv"])]


def test_scores_at_the_threshold_and_in_both_polarities(emu, host):
    """40 / 48 is found, 38 / 48 is not; one half symbol's amplitude a float apart decides on both sides within 1e-3 of 0.8; exact zeros are 0 / 0; the inverted
    stream's scores have the other sign, --softinv gives the sign back, and bits and lines are the same all three ways"""
    mv = lambda name: [r.mv for r in _one_call(emu, name)[0]]    # noqa: E731
    assert [abs(m) for m in mv("clean_ims100")] == [1.0, 1.0, 1.0]
    assert mv("flips_4") == [np.float32(40.0 / 48.0)] and mv("flips_5") == []
    assert M.ref_score(M.cases()["flips_5"]["s"][40:88]) == np.float32(38.0 / 48.0)
    lo, hi = M.cases()["edge_below"], M.cases()["edge_above"]
    assert np.nextafter(np.float32(lo["amp"]), np.float32(2)) == np.float32(hi["amp"])
    a, b = M.ref_score(lo["s"][:48]), M.ref_score(hi["s"][:48])
    assert a <= F08 < b and F08 - a < 1e-3 and b - F08 < 1e-3
    assert mv("edge_below") == [] and mv("edge_above") == [b]
    assert np.isnan(M.ref_score(np.zeros(48, np.float32)))
    inv, sinv = _one_call(emu, "inverted")[0], _one_call(emu, "inverted_softinv")[0]
    assert len(inv) == 2 and [r.mv for r in inv] == [-r.mv for r in sinv] and all(abs(r.mv) > F08 for r in inv)
    assert [M.key(r) for r in inv] == [M.key(r) for r in sinv]
    signs = [np.sign(r.mv) for r in _one_call(emu, "clean_ims100")[0] + _one_call(emu, "clean_rs11g")[0] + _one_call(emu, "back_to_back")[0]]
    assert 1.0 in signs and -1.0 in signs                        # continuous frames start on either level: hits of both polarities
    # an exact zero is a 1 whatever its sign and whatever --softinv makes of it, while every other half symbol changes sides: --softinv on a stream is the
    # negated stream, and both differ from the stream as it is — at the zeros alone does the polarity matter for bits
    for a_, b_ in (("zero_symbols", "zero_symbols_neg_softinv"), ("zero_symbols_neg", "zero_symbols_softinv")):
        assert [M.key(r) for r in _one_call(emu, a_)[0]] == [M.key(r) for r in _one_call(emu, b_)[0]]
    assert [M.key(r) for r in _one_call(emu, "zero_symbols")[0]] != [M.key(r) for r in _one_call(emu, "zero_symbols_neg")[0]]


def test_zeros_decide_bits(emu, host):
    """the zero case is about something: with the zeros read as negative (the `>` mutation) other bits come out"""
    c = M.cases()["zero_symbols"]
    hb = _arb(host, "zero_symbols")[0][0]
    sym = c["s"][hb:hb + M.NSYM]
    other = np.where(sym == 0, np.float32(-1.0), sym)
    assert (sym == 0).sum() > 40 and list(M.biphase(sym)) != list(M.biphase(other))
    assert any(np.signbit(v) for v in sym[sym == 0]) and any(not np.signbit(v) for v in sym[sym == 0])


def test_one_call_longer_than_the_staging_buffer_and_the_two_lengths_around_it(emu, host):
    s = M.long_stream()
    assert len(s) > M.STAGE_MAX + 1
    want = M.host_frames(host, s, cache="long")
    assert len(want) == 11
    one = M.emu_frames(emu, s, [len(s)])
    assert [M.key(r) for r in one[0]] == [M.key(w) for w in want]
    for first in (M.STAGE_MAX, M.STAGE_MAX + 1):
        got = M.emu_frames(emu, s, [first, len(s) - first])
        assert [M.full(r) for r in got[0]] == [M.full(r) for r in one[0]] and M.state(got[2]) == M.state(one[2]) and got[1] == 0


# ---------------------------------------------------------------- 2. the ring
def test_ring_after_an_accepted_header_is_that_header(emu, host):
    c = M.cases()["inverted_softinv"]
    hb = _arb(host, "inverted_softinv")[0][0]
    s = c["s"][:hb + 777]
    for calls in ([len(s)], [49], [hb, 7]):
        _, _, end = M.emu_frames(emu, s, calls, **_opts(c))
        assert end.mode == 1 and end.done == 777 and end.hdr_bit == hb
        assert [float(v) for v in end.hist] == [float(-v) for v in s[hb - 48:hb]]
        assert float(end.carry) == float(-s[-1])                 # the pending odd half symbol


def test_hit_right_behind_a_frame_depends_on_the_ring_the_header_left(emu, host):
    """K half symbols behind the frame complete the (partly silent) header in the ring to a second hit; the frame's last half symbols in its place, or zeros, give none"""
    c = M.cases()["ring_behind_frame"]
    want = _arb(host, "ring_behind_frame")
    assert [w[0] for w in want] == [60, c["at"] + c["K"]]
    got = _one_call(emu, "ring_behind_frame")[0]
    assert [r.hdr_bit for r in got] == [60, c["at"] + c["K"]]
    y = c["s"][c["at"]:c["at"] + c["K"]]
    ring = np.concatenate([c["s"][12:60][c["K"]:], y])
    assert got[1].mv == M.ref_score(ring) and abs(got[1].mv) > F08
    assert not abs(M.ref_score(np.concatenate([c["s"][c["at"] - 48 + c["K"]:c["at"]], y]))) > F08
    assert not abs(M.ref_score(np.concatenate([np.zeros(48 - c["K"], np.float32), y]))) > F08


# ---------------------------------------------------------------- 3. call cuts
def _cut_run(emu, name, calls):
    c = M.cases()[name]
    got, dropped, end = M.emu_frames(emu, c["s"], calls, **_opts(c))
    return [M.full(r) for r in got], dropped, M.state(end)


def _all_streams(emu, calls_of):
    for name in STREAMS:
        _one_call(emu, name)
    with ThreadPoolExecutor(max_workers=8) as pool:              # (the emulator keeps its fibers per thread; ctypes releases the interpreter lock)
        res = list(pool.map(lambda name: _cut_run(emu, name, calls_of(name)), STREAMS))
    for name, r in zip(STREAMS, res):
        one = _one_call(emu, name)
        assert r == (one[1], one[2], one[3]), name               # records (mv bit for bit: the same operations), nothing dropped, the end state


@pytest.mark.parametrize("cut", M.CUTS)
def test_fixed_cuts_equal_one_call(emu, cut):
    _all_streams(emu, lambda name: [cut])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_cuts_equal_one_call(emu, seed):
    _all_streams(emu, lambda name: M.random_cuts(len(M.cases()[name]["s"]), 100 * seed + STREAMS.index(name)))


def test_cuts_on_the_headers_and_the_frames_last_symbol_and_an_odd_half_symbol(emu, host):
    """a call that ends with the header's last half symbol, one that ends with the frame's last, one half symbol to either side of both, and calls that end on an
    odd half symbol of the frame"""
    for name in ("clean_ims100", "back_to_back", "sigma03"):
        c = M.cases()[name]
        hb = _arb(host, name)[0][0]
        one = _one_call(emu, name)
        for first in (hb - 1, hb, hb + 1, hb + M.NSYM - 1, hb + M.NSYM, hb + M.NSYM + 1, hb + 1, hb + 333, hb + 641):
            if first < 1:
                continue
            assert _cut_run(emu, name, [first, len(c["s"])]) == (one[1], one[2], one[3]), (name, first)
        assert _cut_run(emu, name, [hb + 5, 3, 1, 1, 64, 129, len(c["s"])]) == (one[1], one[2], one[3]), name


def test_state_inside_a_bit_survives_any_cut(emu, host):
    c = M.cases()["sigma03"]
    hb = _arb(host, "sigma03")[0][0]
    s = c["s"][:hb + 2 * 200 + 1]
    want = M.emu_frames(emu, s, [len(s)])
    assert want[2].mode == 1 and want[2].done == 401 and float(want[2].carry) == float(s[-1])
    for calls in ([1], [2], [3], [47], [64], [65], M.random_cuts(len(s), 5, 1, 300)):
        got = M.emu_frames(emu, s, calls)
        assert M.state(got[2]) == M.state(want[2]), calls


# ---------------------------------------------------------------- 4. the record cap
def _cap_stream():
    rng = np.random.default_rng(9)
    first = M.cap_stream(5)
    return first, np.concatenate([first, M.soft(M.fsym(40)), M.noise(rng, 80, 0.05)])


def test_record_cap_drops_and_the_next_call_is_intact(emu, host):
    first, s = _cap_stream()
    want = M.host_frames(host, s, cache="cap")
    assert len(want) == 6 and all(w[2] == bytes(12) for w in want)
    got, dropped, end = M.emu_frames(emu, s, [len(first), len(s) - len(first)], cap=3)
    assert dropped == 2 and len(got) == 4
    assert [M.key(r) for r in got] == [M.key(w) for w in want[:3] + want[5:]]
    assert end.mode == 0


def test_sanitized_standalone_replay_of_the_call_cuts(host, tmp_path):
    """the emulator translation unit under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program with its own main (tests/emu/softin_meisei_replay.cpp),
    run as a process of its own, outside the interpreter, in the environment as it is (the sanitizer runtimes are linked into the program).  The noisy stream in
    calls of 1 (odd half symbols), 47 and 65, the back-to-back stream in calls of 1200 and 1201, the inverted stream with --softinv, the ring case in calls of 9,
    the BCH streams (--ecc off among them), the long stream in one call above the staging limit, and five frames against three slots."""
    exe = str(tmp_path / "softin_meisei_replay_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, os.path.join(M.EMU_DIR, "softin_meisei_replay.cpp"), M.EMU_SRC])

    def run(s, c, cap, calls):
        p = tmp_path / "s.f32"
        np.ascontiguousarray(s, np.float32).tofile(p)
        r = subprocess.run([exe, str(p), str(int(c["softinv"])), str(c["ecc"]), str(cap)] + calls, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert b"ERROR" not in r.stderr and b"runtime error" not in r.stderr
        return r

    runs = [("sigma03", ["1"]), ("sigma03", ["47"]), ("sigma03", ["65"]), ("back_to_back", ["1200"]), ("back_to_back", ["1201"]), ("inverted_softinv", ["48"]),
            ("ring_behind_frame", ["9"]), ("zero_symbols_neg", ["63"])] + [("bch_" + k, ["64"]) for k in M.BCH_STREAMS]
    for name, calls in runs:
        c = M.cases()[name]
        r = run(c["s"], c, 64, calls)
        assert r.stdout.decode().splitlines() == [w[3] for w in _arb(host, name)] and len(_arb(host, name)) == c["n"], name
    plain = dict(softinv=False, ecc=1)
    s = M.long_stream()
    r = run(s, plain, 64, [str(M.STAGE_MAX + 1), "2400"])
    assert r.stdout.decode().splitlines() == [w[3] for w in M.host_frames(host, s, cache="long")]
    first, s = _cap_stream()
    r = run(s, plain, 3, [str(len(first)), "2400"])
    assert b"4 frames, 2 dropped" in r.stderr
    want = M.host_frames(host, s, cache="cap")
    assert r.stdout.decode().splitlines() == [w[3] for w in want[:3] + want[5:]]


# ---------------------------------------------------------------- 5. the end-of-frame step alone
def _end(emu, bits600, ecc=1):
    r = M.Rec()
    assert emu.emu_meisei_end(M.pack(bits600), ecc, C.byref(r)) == 0
    return r


def test_bch_every_syndrome_of_8_messages(emu, host):
    """the decoder's result depends on the syndrome alone, and the 12 check bits reach all 4096: 8 messages x 4096 patterns on cw[0 .. 11] = 32 768 blocks, twelve a
    frame; verdict class and the 46 bits left in the block equal sonde_ecc_decode_bch_gf2t2 plus the padding and word-parity rule, block for block"""
    classes = {}
    for m in M.bch_messages():
        blocks = M.syndrome_blocks(host, m)
        frames = M.sweep_frames(blocks)
        n = 0
        for fr in frames:
            r = _end(emu, fr)
            out = M.unpack(r.bits)
            for k in range(12):
                i = n if n < len(blocks) else 12 * (n // 12)
                v, left = M.block_rule(host, blocks[i])
                at = M.block_at(k)
                assert r.block_err[k] == v and list(out[at:at + 46]) == left, (n, k)
                classes[v] = classes.get(v, 0) + 1
                n += 1
            assert list(out[:24]) == list(fr[:24]) and list(out[300:324]) == list(fr[300:324])
    assert set(classes) == {0, 1, 2, 0xE, 0xF}, classes
    assert classes[0] == 8                                        # the codewords themselves (the fill of each last frame repeats a damaged block)


def test_bch_named_cases(emu, host):
    named = M.bch_named(host)
    base = M.frame_bits(5)
    for name, (bits, ecc, want) in named.items():
        r = _end(emu, bits, ecc)
        mb, mbe = M.model_end(host, bits, ecc)
        assert (bytes(r.bits), bytes(r.block_err)) == (mb, mbe), name
        assert {k: v for k, v in enumerate(r.block_err) if v} == want, name
        if ecc and all(v <= 2 for v in want.values()) and not name.startswith("three"):
            assert list(M.unpack(r.bits)) == base, name           # corrected back to the frame
        if any(v >= 0xE for v in want.values()) or not ecc:
            assert list(M.unpack(r.bits)) == [int(b) for b in bits], name      # bits as received: no write-back on a negative verdict, none without --ecc
    # the accepted miscorrection leaves a different, valid block
    r = _end(emu, named["three_accepted"][0])
    assert list(M.unpack(r.bits)) != base


# ---------------------------------------------------------------- 6. the compiled reference, live
@pytest.mark.parametrize("name", NAMES)
def test_case_equals_compiled_reference(emu, name):
    if not golden_cases.need_ref():
        return
    c = M.cases()[name]
    args = [M.REF, "--softinv" if c["softinv"] else "--softin", "-r", "-v"] + (["--ecc"] if c["ecc"] else [])
    r = subprocess.run(args, input=np.ascontiguousarray(c["s"], np.float32).tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0
    ref = [l.rstrip() for l in r.stdout.decode().splitlines() if l.strip()]
    got = _one_call(emu, name)[0]
    assert [M.raw_line(r_, c["ecc"]).rstrip() for r_ in got] == ref
