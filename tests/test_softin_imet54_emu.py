"""The DEVICE iMet-54 soft-bit consumer (radiosonde_auto_rx_amd/csrc/sonde_softin_imet54_dev.h: header search at 0.8 with the ring left as it is, the polarity rule
with --auto, 8N1 characters on a lane per character, de-interleave + Hamming(8,4) on a lane per codeword, the ecc sums and both check sums on the wave) executed on
the CPU under tests/emu/wave_emu.h and driven as sonde_softin_dev_push_device drives k_softin_imet54 (tests/emu/softin_imet54_emu.cpp).  The arbiter is the host tier
sonde_imet54_dec_push_soft with `-r --ecc` (`-r` where a case has --ecc off), and `oracle/_ref/imet54mod --softin [-i] [--auto] -r --ecc` live where that binary
exists.  The same source is compiled by hipcc into k_softin_imet54; tests/test_gpu_softin_imet54.py runs it there on the streams of tests/imet54_softin_cases.py.

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
import imet54_softin_cases as M
from tools import synth

NAMES = sorted(M.case_opts())                              # (the streams are built inside the tests: nothing loads the library at collection)
STREAMS = M.stream_names()
F08 = np.float32(0.8)


@pytest.fixture(scope="module")
def emu():
    return M.load_emu()


@pytest.fixture(scope="module")
def host():
    return M.load_host()


def _opts(c):
    return dict(inv=c["inv"], softinv=c["softinv"], aut=c["aut"], ecc=c["ecc"])


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
    assert emu.emu_imet54_header_mask() == sum(int(ch) << i for i, ch in enumerate(M.HEADER))


# ---------------------------------------------------------------- 1. every case in one call against the arbiter
@pytest.mark.parametrize("name", NAMES)
def test_case_equals_host_arbiter(emu, host, name):
    c = M.cases()[name]
    want = _arb(host, name)
    assert len(want) == c["n"]                                   # what the case is about, said by the arbiter
    got, _, dropped, st, end = _one_call(emu, name)
    assert dropped == 0
    assert [M.key(r, c["ecc"]) for r in got] == [M.key(w, c["ecc"]) for w in want]
    assert [M.raw_line(r, c["ecc"]) for r in got] == [w[6] for w in want]
    hbs = [w[0] for w in want]
    for r in got:                                                # the score the reference computes over its ring at the hit, bit for bit
        assert struct.pack("<f", r.mv) == struct.pack("<f", M.ref_score(M.ring_at(c["s"], hbs, r.hdr_bit, c["softinv"])))
    assert st[0] == 0 and st[2] == len(c["s"])                   # searching again, every symbol counted
    assert end.inv == c.get("end_inv", c["inv"])
    assert [struct.pack("<f", v) for v in end.hist] == [struct.pack("<f", v) for v in M.ring_at(c["s"], hbs, len(c["s"]), c["softinv"])]


def test_scores_at_the_threshold(emu, host):
    """34 / 40 is found, 32 / 40 = 0.8f is not; one symbol's amplitude a float apart decides on both sides within 1e-3 of 0.8; exact zeros are 0 / 0"""
    mv = lambda name: [r.mv for r in _one_call(emu, name)[0]]    # noqa: E731
    assert mv("clean") == [1.0, 1.0, 1.0]
    assert mv("flips_3") == [np.float32(34.0 / 40.0)]
    assert mv("flips_4") == []
    s4 = M.cases()["flips_4"]["s"]
    assert M.ref_score(s4[40:80]) == F08                          # exactly the threshold: no hit
    lo, hi = M.cases()["edge_below"], M.cases()["edge_above"]
    assert np.nextafter(np.float32(lo["amp"]), np.float32(2)) == np.float32(hi["amp"])
    a, b = M.ref_score(lo["s"][:40]), M.ref_score(hi["s"][:40])
    assert a <= F08 < b and F08 - a < 1e-3 and b - F08 < 1e-3
    assert mv("edge_below") == [] and mv("edge_above") == [b]
    assert np.isnan(M.ref_score(np.zeros(40, np.float32)))
    assert all(m < -0.8 for m in mv("inverted_inv") + mv("inverted_auto")) and all(m > 0.8 for m in mv("inverted_softinv"))
    assert [r.inv for r in _one_call(emu, "inverted_auto")[0]] == [1, 1]         # --auto: flipped at the first header and kept for the next
    assert [r.inv for r in _one_call(emu, "auto_flips_back")[0]] == [1, 0]


def test_one_call_longer_than_the_staging_buffer_and_the_two_lengths_around_it(emu, host):
    s = M.long_stream()
    assert len(s) > M.STAGE_MAX + 1
    want = M.host_frames(host, s, cache="long")
    assert len(want) == 6
    one = M.emu_frames(emu, s, [len(s)])
    assert [M.key(r) for r in one[0]] == [M.key(w) for w in want]
    for first in (M.STAGE_MAX, M.STAGE_MAX + 1):
        got = M.emu_frames(emu, s, [first, len(s) - first])
        assert [M.full(r) for r in got[0]] == [M.full(r) for r in one[0]] and M.state(got[2]) == M.state(one[2]) and got[1] == 0


# ---------------------------------------------------------------- 2. the ring
def test_ring_after_an_accepted_header_is_that_header(emu, host):
    c = M.cases()["inverted_softinv"]
    hb = _arb(host, "inverted_softinv")[0][0]
    s = c["s"][:hb + 1234]
    for calls in ([len(s)], [41], [hb, 7]):
        _, _, end = M.emu_frames(emu, s, calls, **_opts(c))
        assert end.mode == 1 and end.done == 1234 and end.carry_n == 4 and end.hdr_bit == hb
        assert [float(v) for v in end.hist] == [float(-v) for v in s[hb - 40:hb]]
        assert [float(v) for v in end.carry[:4]] == [float(-v) for v in s[-4:]]


def test_hit_right_behind_a_frame_depends_on_the_ring_the_header_left(emu, host):
    """two symbols behind character 220 complete the (partly silent) header in the ring to a second hit; the frame's last symbols in its place, or zeros, give none"""
    c = M.cases()["ring_behind_frame"]
    want = _arb(host, "ring_behind_frame")
    assert [w[0] for w in want] == [72, c["at"] + c["K"]]
    got = _one_call(emu, "ring_behind_frame")[0]
    assert [r.hdr_bit for r in got] == [72, c["at"] + c["K"]]
    y = c["s"][c["at"]:c["at"] + c["K"]]
    ring = np.concatenate([c["s"][32:72][c["K"]:], y])
    assert got[1].mv == M.ref_score(ring) and got[1].mv > F08
    assert not abs(M.ref_score(np.concatenate([c["s"][c["at"] - 40 + c["K"]:c["at"]], y]))) > F08
    assert not abs(M.ref_score(np.concatenate([np.zeros(40 - c["K"], np.float32), y]))) > F08


def test_header_20_symbols_behind_a_dropped_hit_is_found_with_the_arbiters_score(emu, host):
    c = M.cases()["dropped_then_20"]
    want = _arb(host, "dropped_then_20")
    assert [w[0] for w in want] == [c["hdr_bit"]]
    assert M.ref_score(c["s"][30:70]) < -F08                     # the hit of the other polarity, dropped
    got = _one_call(emu, "dropped_then_20")[0]
    assert [r.hdr_bit for r in got] == [c["hdr_bit"]]
    assert got[0].mv == M.ref_score(c["s"][50:90]) and F08 < got[0].mv < 0.81
    assert not abs(M.ref_score(np.concatenate([np.zeros(20, np.float32), c["s"][70:90]]))) > F08       # an emptied ring would not find it


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


def test_cuts_on_the_headers_and_the_frames_last_symbol(emu, host):
    """a call that ends with the header's last symbol, one that ends with the frame's last symbol, one symbol to either side of both"""
    for name in ("clean", "back_to_back"):
        c = M.cases()[name]
        hb = _arb(host, name)[0][0]
        one = _one_call(emu, name)
        for first in (hb - 1, hb, hb + 1, hb + M.NSYM - 1, hb + M.NSYM, hb + M.NSYM + 1):
            assert _cut_run(emu, name, [first, len(c["s"])]) == (one[1], one[2], one[3]), (name, first)


def test_state_inside_a_character_survives_any_cut(emu):
    c = M.cases()["sigma03"]
    s = c["s"][:17 + M.PRE + 40 + 10 * 100 + 7]
    want = M.emu_frames(emu, s, [len(s)])
    assert want[2].mode == 1 and want[2].carry_n == 7 and want[2].done == 1007
    assert list(want[2].carry)[:7] == [float(v) for v in s[-7:]]
    for calls in ([1], [9], [11], [40], M.random_cuts(len(s), 5, 1, 300)):
        got = M.emu_frames(emu, s, calls)
        assert M.state(got[2]) == M.state(want[2])


# ---------------------------------------------------------------- 4. the record cap
def _cap_stream():
    rng = np.random.default_rng(9)
    first = M.cap_stream(5)
    return first, np.concatenate([first, M.soft(M.onair(M.fbits(M.frame(40)), pre=0, idle=0)), M.noise(rng, 80, 0.05)])


def test_record_cap_drops_and_the_next_call_is_intact(emu, host):
    first, s = _cap_stream()
    want = M.host_frames(host, s, cache="cap")
    assert len(want) == 6 and all(w[5] == "[OK]" for w in want)
    got, dropped, end = M.emu_frames(emu, s, [len(first), len(s) - len(first)], cap=3)
    assert dropped == 2 and len(got) == 4
    assert [M.key(r) for r in got] == [M.key(w) for w in want[:3] + want[5:]]
    assert end.mode == 0


def test_sanitized_standalone_replay_of_the_call_cuts(host, tmp_path):
    """the emulator translation unit under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program with its own main (tests/emu/softin_imet54_replay.cpp),
    run as a process of its own, outside the interpreter, in the environment as it is (the sanitizer runtimes are linked into the program).  The noisy stream in
    calls of 11 and 41 symbols, the long stream in one call above the staging limit, the back-to-back stream in calls of 2241, the inverted stream with --auto in
    calls of 40, a frame with --ecc off, and five frames against three slots."""
    exe = str(tmp_path / "softin_imet54_replay_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, os.path.join(M.EMU_DIR, "softin_imet54_replay.cpp"), M.EMU_SRC])

    def run(s, c, cap, calls):
        p = tmp_path / "s.f32"
        np.ascontiguousarray(s, np.float32).tofile(p)
        r = subprocess.run([exe, str(p), str(int(c["softinv"])), str(c["inv"]), str(c["aut"]), str(c["ecc"]), str(cap)] + calls, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert b"ERROR" not in r.stderr and b"runtime error" not in r.stderr
        return r

    for name, calls in (("sigma03", ["11"]), ("sigma03", ["41"]), ("back_to_back", ["2241"]), ("inverted_auto", ["40"]), ("eof_ecc_off_damaged", ["64"]), ("ring_behind_frame", ["9"])):
        c = M.cases()[name]
        r = run(c["s"], c, 64, calls)
        assert r.stdout.decode().splitlines() == [w[6] for w in _arb(host, name)] and len(_arb(host, name)) == c["n"]
    plain = dict(softinv=False, inv=0, aut=0, ecc=1)
    s = M.long_stream()
    r = run(s, plain, 64, [str(M.STAGE_MAX + 1), "4800"])
    assert r.stdout.decode().splitlines() == [w[6] for w in M.host_frames(host, s, cache="long")]
    first, s = _cap_stream()
    r = run(s, plain, 3, [str(len(first)), "4800"])
    assert b"4 frames, 2 dropped" in r.stderr
    want = M.host_frames(host, s, cache="cap")
    assert r.stdout.decode().splitlines() == [w[6] for w in want[:3] + want[5:]]


# ---------------------------------------------------------------- 5. the end-of-frame step alone
def _py_crc(f):
    """both verdicts from the generator's own forward forms (tools/synth.py, pinned by the reference printing [OK] / [ok] for its frames)"""
    c0, c1 = synth._imet54_check_words(bytearray(f))
    c0 ^= ((f[100] << 8) | f[101]) ^ 0x5000; c1 ^= ((f[106] << 8) | f[107]) ^ 0x1DAD
    m4 = bytearray(0x34)
    for i in range(0x34 // 4):
        for j in range(4):
            m4[4 * i + j] = f[4 * i + 3 - j]
    rem = 0
    for byte in m4:
        rem ^= byte << 24
        for _ in range(8):
            rem = ((rem << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if rem & 0x80000000 else (rem << 1) & 0xFFFFFFFF
    return int(c1 == 0 and (c0 & 0xF000) == 0), int((rem ^ 0x63D60875) == int.from_bytes(f[0x34:0x38], "big"))


def _end(emu, bits, ecc):
    r = M.Rec()
    assert emu.emu_imet54_end(M.chars_of(bits), ecc, C.byref(r)) == 0
    return r


def _host_line(host, decs, bits, ecc):
    if ecc not in decs:
        decs[ecc] = M.host_dec(host, raw=1, ecc=ecc)
    sb = np.ascontiguousarray(2.0 * np.asarray(bits, np.float32) - 1.0, np.float32)
    buf = C.create_string_buffer(1024)
    n = host.sonde_imet54_dec_frame(decs[ecc], sb.ctypes.data, 2200, buf, 1024)
    assert n > 0
    return buf.raw[:n].decode().rstrip("\n")


def test_end_of_frame_equals_host_decoder_on_200_frames(emu, host):
    """gather, Hamming, nibbles, ecc sums and tag on frames with 0 .. 2 flips per codeword, random frames and a random 220th character: the `-r [--ecc]` line of
    sonde_imet54_dec_frame byte for byte; both check-sum verdicts against the generator's forward forms"""
    rng = np.random.default_rng(2054)
    decs, tags = {}, set()
    for k in range(200):
        kind = k % 5
        if kind == 4:
            fr = bytes(rng.integers(0, 256, 108, dtype=np.uint8))
        else:
            fr = M.frame(k, check=("std", "cont", "none")[k % 3], imet50=bool(k % 7 == 0))
        bits = M.fbits(fr).copy()
        if kind in (1, 2):                                       # sparse single flips / up to two per codeword
            for j in range(216):
                nf = int(rng.integers(0, 3)) if kind == 2 else int(rng.random() < 0.03)
                for i in rng.choice(8, nf, replace=False):
                    bits[M.cwbit(j, int(i))] ^= 1
        if kind == 3:
            j = int(rng.integers(0, 216)); i = rng.choice(8, 2, replace=False)
            bits[M.cwbit(j, int(i[0]))] ^= 1; bits[M.cwbit(j, int(i[1]))] ^= 1
        bits[2190:2200] = rng.integers(0, 2, 10)
        for p in rng.choice(220, 25, replace=False):             # start and stop bits are not looked at
            bits[10 * int(p)] ^= 1; bits[10 * int(p) + 9] ^= int(rng.integers(0, 2))
        ecc = int(k % 4 != 3)
        r = _end(emu, bits, ecc)
        want = _host_line(host, decs, bits, ecc)
        assert M.raw_line(r, ecc) == want, (k, kind, ecc)
        assert (r.crc_std, r.crc_cont) == _py_crc(bytes(r.frame)), k
        assert r.ecc_std == r.ecc_frm
        tags.add(M.tag_of(r))
    for d in decs.values():
        host.sonde_imet54_dec_destroy(d)
    assert tags == {"[OK]", "[ok]", "[oo]", "[NO]", "[no]"}


def test_hamming_cases(emu, host):
    decs = {}
    H = M.hamming_bits()
    base = M.frame(3)
    for name, (bits, ecc) in H.items():
        assert M.raw_line(_end(emu, bits, ecc), ecc) == _host_line(host, decs, bits, ecc), name
    rec = {name: _end(emu, bits, ecc) for name, (bits, ecc) in H.items()}
    sums = lambda r: (r.ecc_frm, r.ecc_tlm, r.ecc_std)           # noqa: E731
    assert sums(rec["no_error"]) == (0, 0, 0) and bytes(rec["no_error"].frame) == base and rec["no_error"].crc_std == 1
    assert sums(rec["one_flip_each"]) == (8, 8, 8) and bytes(rec["one_flip_each"].frame) == base
    for i in range(8):
        assert sums(rec["flip_cw5_bit%d" % i]) == (1, 1, 1) and bytes(rec["flip_cw5_bit%d" % i].frame) == base
    # two flips: 0xF0 and a nibble of 16, which leaves its half of the byte 0
    r = rec["two_flips"]
    assert sums(r) == (-1, -1, -1) and r.frame[10] == base[10] & 0x0F and bytes(r.frame[:10]) + bytes(r.frame[11:]) == base[:10] + base[11:]
    # the bounds of ecc_tlm (88) and ecc_std (104); codeword 40 is repaired ahead of them
    assert sums(rec["f0_at_0"]) == (-1, -1, -1)
    assert sums(rec["f0_at_87"]) == (-1, -1, -1)
    assert sums(rec["f0_at_88"]) == (-1, 1, -1)
    assert sums(rec["f0_at_103"]) == (-1, 1, -1)
    assert sums(rec["f0_at_104"]) == (1, 1, 1) and rec["f0_at_104"].frame[52] == base[52] & 0x0F
    assert [sums(rec["fix_at_%d" % j]) for j in (87, 88, 103, 104)] == [(1, 1, 1), (1, 0, 1), (1, 0, 1), (0, 0, 0)]
    assert bytes(rec["char220_set"].frame) == base == bytes(rec["char220_mixed"].frame) and sums(rec["char220_set"]) == (0, 0, 0)
    # --ecc off: nothing repaired, the damaged codeword misses the table
    r = rec["ecc_off_damaged"]
    assert sums(r) == (-1, -1, -1) and r.frame[15] == base[15] & 0x0F and sums(rec["ecc_off_clean"]) == (0, 0, 0)
    for d in decs.values():
        host.sonde_imet54_dec_destroy(d)


def test_check_sum_cases(emu, host):
    decs = {}
    S = M.checksum_bits()
    rec = {}
    for name, (bits, ecc) in S.items():
        r = rec[name] = _end(emu, bits, ecc)
        assert M.raw_line(r, ecc) == _host_line(host, decs, bits, ecc), name
        assert (r.crc_std, r.crc_cont) == _py_crc(bytes(r.frame)), name
    v = lambda name: (rec[name].crc_std, rec[name].crc_cont, M.tag_of(rec[name]))        # noqa: E731
    assert v("check_std") == (1, 0, "[OK]") and v("check_cont") == (0, 1, "[ok]") and v("check_none") == (0, 0, "[oo]")
    for p in (0, 51, 52, 99, 100, 105, 107):
        # the standard check covers every byte but the low 12 bits of the word at 100; the continuous one bytes 0 .. 55
        assert v("check_std_flip%d" % p)[0] == 0, p
        assert v("check_cont_flip%d" % p)[1] == (0 if p <= 52 else 1), p
        assert v("check_none_flip%d" % p) == (0, 0, "[oo]")
    f = bytearray(M.frame(4)); f[101] ^= 0x5A; f[100] ^= 0x0A
    assert _end(emu, M.fbits(bytes(f)), 1).crc_std == 1           # (those twelve bits are not checked)
    assert v("none_not_f8") == (0, 0, "[oo]") and v("none_f8_repaired") == (0, 0, "[NO]") and v("none_not_f8_repaired") == (0, 0, "[no]")
    assert v("none_ecc_off") == (0, 0, "[NO]") and v("std_ecc_off") == (1, 0, "[OK]")
    for d in decs.values():
        host.sonde_imet54_dec_destroy(d)


# ---------------------------------------------------------------- 6. the compiled reference, live
@pytest.mark.parametrize("name", NAMES)
def test_case_equals_compiled_reference(emu, name):
    if not golden_cases.need_ref():
        return
    c = M.cases()[name]
    args = [M.REF, "--softinv" if c["softinv"] else "--softin"] + (["-i"] if c["inv"] else []) + (["--auto"] if c["aut"] else []) + ["-r"] + (["--ecc"] if c["ecc"] else [])
    r = subprocess.run(args, input=np.ascontiguousarray(c["s"], np.float32).tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0
    ref = [l.rstrip() for l in r.stdout.decode().splitlines() if l.strip()]
    got = _one_call(emu, name)[0]
    assert [M.raw_line(r_, c["ecc"]) for r_ in got] == ref
