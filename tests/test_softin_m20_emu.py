"""The DEVICE M20 soft-bit consumer (radiosonde_auto_rx_amd/csrc/sonde_softin_mxx_dev.h: header search at 0.8 in either polarity, two soft symbols per bit, the
differential code, bits2bytes on a lane per byte, print_frame's verdicts) executed on the CPU under tests/emu/wave_emu.h and driven as sonde_softin_dev_push_device
drives k_softin_m20 (tests/emu/softin_m20_emu.cpp).  The arbiter is the host framer (sonde_softin_create(SONDE_M20) / set_m10_skip / push / fetch_m20, pinned to the
compiled reference by tests/test_m20_fields.py), and `oracle/_ref/m20mod --softin` live where that binary exists.  Records agree exactly — nbits, len, cs_ok, cs_calc,
blk_ok, fw, mv_pos, the 172 frame bytes — and mv bit for bit (the same operations, -ffp-contract=off).  The same source is compiled by hipcc into k_softin_m20;
tests/test_gpu_softin_m20.py runs it there on the streams of tests/m20_softin_cases.py.

A consumer has no `finish`: every stream ends with a short tail in which no header is found, so no frame is left in progress.

A frame's first bit is decided against '0' (0x30) and so never decodes as '1': through a symbol stream byte 0 stays below 0x80, and the clamp of the length byte at
0x45 + 64 = 0x85 cannot be reached that way.  The length bytes from 0x80 up go through m20_wave_verdicts alone (emu_m20_verdicts) against sonde_m20_frame_finish."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import m20_softin_cases as M
from radiosonde_auto_rx_amd.engine import SondeM20Frame

ROOT = M.ROOT
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    return M.load_emu()


@pytest.fixture(scope="module")
def host():
    return M.load_host()


def _state(st):
    """the end state as far as it means anything: the pending symbol only while one is pending, frame position and previous bit only inside a frame, the skip count
    only while skipping"""
    return (st["mode"], st["bits_in"], st["mhalf"] if st["mode"] == 1 else 0, st["ms1"] if st["mode"] == 1 and st["mhalf"] else 0.0,
            (st["mpos"], st["mbit0"], st["hdr_bit"], st["mv"]) if st["mode"] == 1 else None, st["mskip"] if st["mode"] == 2 else 0)


def _ref_lines(s, skip, softinv=False):
    r = subprocess.run([M.REF, "--softinv" if softinv else "--softin", "-r", "-v" if skip else "-vvv"], input=np.ascontiguousarray(s, np.float32).tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0
    return [l.rstrip() for l in r.stdout.decode().splitlines() if l.strip()]


# ---------------------------------------------------------------- 1. the golden streams
_gold = {}


def _golden(host, name, skip):
    if (name, skip) not in _gold:
        s = np.concatenate([make_golden.m20_field_symbols(make_golden.M20_FIELD_SCENARIOS[name]).astype(np.float32), M.noise(np.random.default_rng(99), 60)])
        _gold[(name, skip)] = (s,) + M.host_frames(host, s, skip)
    return _gold[(name, skip)]


@pytest.mark.parametrize("calls", [[9600], [1000], [251]], ids=["9600", "1000", "251"])
@pytest.mark.parametrize("skip", [1, 0], ids=["skip", "noskip"])
@pytest.mark.parametrize("name", sorted(make_golden.M20_FIELD_SCENARIOS))
def test_golden_streams_equal_host_framer_and_golden_lines(emu, host, name, skip, calls):
    s, want, want_lines = _golden(host, name, skip)
    n = make_golden.M20_FIELD_SCENARIOS[name]["n"]
    assert len(want) == n if skip else len(want) >= n
    got, dropped, _, lines = M.emu_frames(emu, s, calls, skip, H=host)
    assert dropped == 0 and got == want
    if skip:
        gold = np.load(os.path.join(ROOT, "tests", "golden", "m20_fields.npz"))["%s|6" % name].tobytes().decode()
        assert lines == [l.rstrip() for l in gold.splitlines() if l.strip()]
    assert lines == want_lines


# ---------------------------------------------------------------- 2. call cuts
def _cut_stream(n_frames=2):
    """noise, then frames a skip apart (each with its preamble; the gap of 2760 symbols covers the 2720 the skip drops), a tail"""
    rng = np.random.default_rng(21)
    parts = [M.noise(rng, 77)]
    for k in range(n_frames):
        parts += [M.soft(M.frame_symbols(M.m20_bytes(20 + k)), rng, (0.7, 1.3), 0.1), M.noise(rng, 2760 + 13 * k)]
    return np.concatenate(parts)


_cut = {}


def _single(emu, host, s, skip, key):
    if (key, skip) not in _cut:
        got, dropped, st = M.emu_frames(emu, s, [len(s)], skip)
        want, _ = M.host_frames(host, s, skip)
        assert dropped == 0 and got == want and len(got) >= (1 if key == "cut1" else 2)
        _cut[(key, skip)] = (got, st)
    return _cut[(key, skip)]


@pytest.mark.parametrize("cut", ["1", "63", "64", "65", "pair", "header_end", "frame_end", "in_skip"])
@pytest.mark.parametrize("skip", [1, 0], ids=["skip", "noskip"])
def test_any_cut_of_the_stream_gives_the_single_call_result(emu, host, skip, cut):
    s = _cut_stream(1 if cut == "1" else 2)               # (a launch per symbol: one frame and its skip are enough)
    one, st_one = _single(emu, host, s, skip, "cut1" if cut == "1" else "cut")
    hdr = one[0][6]                                       # mv_pos: symbols read when the first header matched = a call of that length ends on its last symbol
    calls = {"1": [1], "63": [63], "64": [64], "65": [65], "pair": [hdr + 7, 9600], "header_end": [hdr, 9600], "frame_end": [hdr + M.NSYM, 9600],
             "in_skip": [hdr + M.NSYM + 1000, 9600]}[cut]
    got, dropped, st = M.emu_frames(emu, s, calls, skip)
    assert dropped == 0 and got == one and _state(st) == _state(st_one)
    if cut in ("pair", "header_end", "frame_end", "in_skip"):
        # the state at the cut itself is the one the case is named after
        _, _, at = M.emu_frames(emu, s[:calls[0]], [calls[0]], skip)
        want = {"pair": (1, 1, 3), "header_end": (1, 0, 0), "frame_end": (2 if skip else 0, 0, M.NSYM // 2), "in_skip": (2 if skip else 0, None, None)}[cut]
        assert at["mode"] == want[0]
        if want[1] is not None and at["mode"] == 1:
            assert (at["mhalf"], at["mpos"]) == want[1:]
        if cut == "in_skip" and skip:
            assert at["mskip"] == M.NSYM // 2 + 1000


@pytest.mark.parametrize("first", [M.STAGE_MAX, M.STAGE_MAX + 1], ids=["staged", "not_staged"])
@pytest.mark.parametrize("skip", [1, 0], ids=["skip", "noskip"])
def test_one_call_at_and_above_the_staging_limit(emu, host, skip, first):
    """a call of M10_STAGE_MAX symbols is staged in (emulated) LDS, one of a symbol more reads the stream where it lies: the same frames"""
    s = _cut_stream(3)
    assert len(s) > first + 2000
    one, st_one = _single(emu, host, s, skip, "stage")
    got, dropped, st = M.emu_frames(emu, s, [first, 9600], skip)
    assert dropped == 0 and got == one and _state(st) == _state(st_one) and len(got) == 3


def test_sanitized_standalone_replay_of_the_call_cuts(emu, host, tmp_path):
    """the emulator translation unit and the host entry point behind its records (sonde_m20_rawline) under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone
    program with its own main (tests/emu/softin_m20_replay.cpp), run as a process of its own, outside the interpreter, in the environment as it is (the sanitizer
    runtimes are linked into the program).  Case 2 once: calls of 65 symbols, skip and no-skip, and one call above the staging limit with a record buffer of one."""
    exe = str(tmp_path / "softin_m20_replay_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, os.path.join(M.EMU_DIR, "softin_m20_replay.cpp"), M.EMU_SRC,
                           os.path.join(M.CSRC, "sonde_frame.cpp")])
    s = _cut_stream(3)
    p = tmp_path / "cut.f32"
    s.tofile(p)
    for skip, cap, calls, least in ((1, 8, ["65"], 3), (0, 8, ["65"], 3), (0, 1, [str(M.STAGE_MAX + 1), "9600"], 2)):
        r = subprocess.run([exe, str(p), str(skip), "0", str(cap)] + calls, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert b"ERROR" not in r.stderr and b"runtime error" not in r.stderr
        _, want = M.host_frames(host, s, skip)
        got = r.stdout.decode().splitlines()
        if cap == 1:
            # two frames complete in the first call, one record fits: the second is dropped, the call after it is intact
            assert got == [want[0], want[2]] and b"3 frames" not in r.stderr and b"1 dropped" in r.stderr
        else:
            assert got == want and len(got) >= least


def test_pairs_of_equal_symbols_decode_as_one(emu, host):
    s = M.equal_pair_stream()
    plain = s.copy()
    for k in (100, 101, 377, 900):
        plain[44 + 32 + 50 + 2 * k] -= np.float32(0.01)           # the first symbol a little lower: s2 - s1 > 0, the same bit whatever the comparison
    want, _ = M.host_frames(host, s, 1)
    got, _, _ = M.emu_frames(emu, s, [700], 1)
    assert len(want) == 1 and got == want
    assert M.rec_no_mv(want[0])[7] == M.rec_no_mv(M.host_frames(host, plain, 1)[0][0])[7]
    low = s.copy()
    low[44 + 32 + 50 + 2 * 100] += np.float32(0.01)               # (and s2 - s1 < 0 is another frame)
    assert M.host_frames(host, low, 1)[0][0][8] != want[0][8]


@pytest.mark.parametrize("gap", [2721, 2720, 2719, 2717])
def test_the_skip_ends_after_exactly_2720_symbols(emu, host, gap):
    """The ring is not fed during the skip.  A header that starts right behind the 2720 dropped symbols is seen whole (score 1); with a shorter gap its first symbols are
    dropped and the window begins with what the ring still holds of the FIRST header — whose tail happens to repeat the header's beginning, so it is still found, with
    another score (the first frame's amplitudes) or, three symbols short, with two mismatches.  The score tells where the skip ended."""
    s = M.skip_end_stream(gap)
    want, _ = M.host_frames(host, s, 1)
    assert len(want) == 2 and want[1][6] == want[0][6] + M.NSYM + gap + 32
    mv = M.mv_of(want[1])
    assert (mv == 1.0) if gap >= 2720 else (0.99 < mv < 1.0) if gap == 2719 else (0.86 < mv < 0.89)
    for calls in ([9600], [333]):
        got, dropped, _ = M.emu_frames(emu, s, calls, 1)
        assert got == want and dropped == 0
    assert M.emu_frames(emu, s, [9600], 0)[0] == M.host_frames(host, s, 0)[0]


# ---------------------------------------------------------------- 3. the threshold
@pytest.mark.parametrize("calls", [[9600], [37]], ids=["9600", "37"])
@pytest.mark.parametrize("softinv", [0, 1])
@pytest.mark.parametrize("flips,found", [(3, True), (4, False)])
def test_header_with_three_flips_is_found_with_four_not(emu, host, flips, found, softinv, calls):
    s = M.threshold_stream(flips)
    if softinv:
        s = -s
    want, _ = M.host_frames(host, s, 1, softinv=softinv)
    got, dropped, st = M.emu_frames(emu, s, calls, 1, softinv=softinv)
    assert len(want) == int(found) and got == want and dropped == 0
    if found:
        assert M.mv_of(got[0]) == np.float32(26.0 / 32.0) and got[0][6] == 40 + 32
    else:
        assert st["mode"] == 0


def test_scores_within_1e_3_of_the_threshold_decide_as_the_host_framer(emu, host):
    amps, lo, hi = M.edge_amplitudes(host)
    sides = set()
    for a in amps:
        s = M.threshold_stream(3, amp=a)
        want, _ = M.host_frames(host, s, 1)
        for calls in ([9600], [41]):
            got, _, _ = M.emu_frames(emu, s, calls, 1)
            assert got == want, (float(a), len(got), len(want))
        sides.add(len(want))
        # the score itself, from the stream: within 1e-3 of the threshold for every amplitude used
        w = s[40:72].astype(np.float64)
        y = np.array([1.0 if c == "1" else -1.0 for c in M.HEADER])
        mv = float((w * y).sum() / np.sqrt((w * w).sum() * 32.0))
        assert abs(mv - 0.8) < 1e-3, (float(a), mv)
        if want:
            assert abs(M.mv_of(want[0]) - mv) < 1e-6
    assert sides == {0, 1} and lo < hi


@pytest.mark.parametrize("calls", [[9600], [7], [32]], ids=["9600", "7", "32"])
def test_windows_of_exact_zeros_give_no_hit(emu, host, calls):
    """all-zero windows are the reference's 0 / 0: NaN, no header — at the very start of a stream (the ring is zero as well) and in the middle of it"""
    rng = np.random.default_rng(8)
    fr = M.soft(M.frame_symbols(M.m20_bytes(2), preamble=False), rng, (0.9, 1.1))
    s = np.concatenate([np.zeros(40, np.float32), M.noise(rng, 50), np.zeros(32, np.float32), fr, M.noise(rng, 50)])
    want, _ = M.host_frames(host, s, 1)
    got, dropped, st = M.emu_frames(emu, s, calls, 1)
    assert len(want) == 1 and want[0][6] == 40 + 50 + 32 + 32 and got == want and dropped == 0
    assert np.isfinite(M.mv_of(got[0])) and np.isfinite(st["mv"])
    z = np.zeros(200, np.float32)
    got, dropped, st = M.emu_frames(emu, z, calls, 1)
    assert got == [] and st["mode"] == 0 and st["bits_in"] == 200


@pytest.mark.parametrize("skip", [1, 0], ids=["skip", "noskip"])
@pytest.mark.parametrize("softinv", [0, 1])
def test_inverted_stream_with_and_without_softinv(emu, host, softinv, skip):
    s = -_cut_stream()
    want, _ = M.host_frames(host, s, skip, softinv=softinv)
    plain, _ = M.host_frames(host, -s, skip)
    got, _, _ = M.emu_frames(emu, s, [1000], skip, softinv=softinv)
    assert got == want and len(got) >= 2
    # the differential code does not care: the same frames either way, the score with the sign of the stream as the decoder sees it
    assert [M.rec_no_mv(r) for r in got] == [M.rec_no_mv(r) for r in plain]
    assert all((M.mv_of(r) > 0) == bool(softinv) for r in got)
    if os.path.exists(M.REF):
        assert _ref_lines(s, skip, softinv) == M.host_frames(host, s, skip, softinv=softinv)[1]


# ---------------------------------------------------------------- 4. length and check variants
VARIANTS = M.variant_frames()


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_length_and_check_variants(emu, host, name):
    data, expect = VARIANTS[name]
    s = M.variant_stream(data)
    for skip in (1, 0):
        want, want_lines = M.host_frames(host, s, skip)
        got, dropped, _, lines = M.emu_frames(emu, s, [1000], skip, H=host)
        assert got == want and lines == want_lines and dropped == 0 and len(got) >= 1
    r = got[0]
    assert r[8][:165] == data and r[0] == 1320
    f = dict(zip(("nbits", "len", "cs_ok", "cs_calc", "blk_ok", "fw"), r[:6]))
    for k, v in expect.items():
        assert f[k] == v, (name, k, f[k], v)
    if os.path.exists(M.REF) and data[0] != 0:                     # (length byte 0: the reference reads in front of its frame buffer; the host rule stands in)
        assert _ref_lines(s, 1)[:1] == [want_lines[0]]


def test_header_pattern_inside_the_payload_is_not_searched(emu, host):
    data = M.m20_bytes(12)
    s = M.variant_stream(data, header_in_payload=True)
    clean = M.variant_stream(data)
    for skip in (1, 0):
        want, _ = M.host_frames(host, s, skip)
        got, _, st = M.emu_frames(emu, s, [500], skip)
        ref, _ = M.host_frames(host, clean, skip)
        assert got == want and len(got) == 1 and got[0][6] == ref[0][6] == 77 + 44 + 32 and st["mode"] == (2 if skip else 0)
    # the pattern is one: alone in front of a frame's worth of symbols it is found
    at = 77 + 44 + 32 + 1000
    _, _, st = M.emu_frames(emu, s[at:at + 40], [40], 0)
    assert st["mode"] == 1 and st["hdr_bit"] == 32 and st["mpos"] == 4


@pytest.mark.parametrize("b0", [0x45 + 64, 0x45 + 65, 0xC0, 0xFF])
def test_length_bytes_a_stream_cannot_carry_are_clamped_as_frame_finish_does(emu, host, b0):
    rng = np.random.default_rng(b0)
    for good in (True, False):
        fr = bytearray(rng.integers(0, 256, 165, dtype=np.uint8).tobytes())
        fr[0] = b0
        pc = 0x45 + 64 - 1
        cs = make_golden.synth.m10_checksum(bytes(fr[:pc])) ^ (0 if good else 0x4000)
        fr[pc] = cs >> 8; fr[pc + 1] = cs & 0xFF
        got = SondeM20Frame()
        assert emu.emu_m20_verdicts(bytes(fr), C.byref(got)) == 0
        want = SondeM20Frame()
        C.memmove(want.frame, bytes(fr), 165)
        assert host.sonde_m20_frame_finish(C.byref(want)) == 0
        assert M.rec(got) == M.rec(want)
        assert got.len == 0x45 + 64 + 1 and got.cs_ok == int(good)


def test_verdicts_for_every_length_byte_equal_frame_finish(emu, host):
    rng = np.random.default_rng(4)
    fr = bytearray(rng.integers(0, 256, 165, dtype=np.uint8).tobytes())
    for b0 in range(256):
        fr[0] = b0
        got, want = SondeM20Frame(), SondeM20Frame()
        assert emu.emu_m20_verdicts(bytes(fr), C.byref(got)) == 0
        C.memmove(want.frame, bytes(fr), 165)
        assert host.sonde_m20_frame_finish(C.byref(want)) == 0
        assert M.rec(got) == M.rec(want), b0


# ---------------------------------------------------------------- 5. no-skip density
def test_four_frames_in_one_call_without_the_skip(emu, host):
    s = M.dense_stream(8)
    want, want_lines = M.host_frames(host, s, 0)
    assert len(want) == 8 and [r[6] for r in want] == [32 + 2672 * k for k in range(8)]
    assert [r[6] for r in M.host_frames(host, s, 1)[0]] == [32 + 2672 * k for k in (0, 3, 6)]      # (with the skip, 2720 symbols dropped behind each frame, two of three are lost)
    got, dropped, st = M.emu_frames(emu, s, [9600], 0)
    assert got == want and dropped == 0
    if os.path.exists(M.REF):
        assert _ref_lines(s, 0) == want_lines
    # a record buffer of three: the call of four frames (9600 symbols: headers at 32, 2704, 5376 and 8048 of 10688 ...) loses its last, the calls after it are intact
    first = [r for r in want if r[6] + M.NSYM <= 9600]
    assert len(first) == 3
    got, dropped, st = M.emu_frames(emu, s, [2672 * 4, 9600], 0, cap=3)
    assert dropped == 1 and got == want[:3] + want[4:]


def test_more_frames_in_one_call_than_the_record_buffer_of_one_channel(emu, host):
    """the device's buffer for one channel holds 4 * 1 + 16 records: a call of 22 frames (not staged) delivers 20 and counts two; the next call is intact"""
    s = np.concatenate([M.dense_stream(22, seed=12), M.dense_stream(2, seed=13)])
    want, _ = M.host_frames(host, s, 0)
    assert len(want) == 24
    got, dropped, st = M.emu_frames(emu, s, [22 * 2672 + 10, 9600], 0, cap=20)
    assert dropped == 2 and got == want[:20] + want[22:]
