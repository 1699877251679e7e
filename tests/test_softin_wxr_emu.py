"""The DEVICE WxR-301D soft-bit consumer (radiosonde_auto_rx_amd/csrc/sonde_softin_wxr_dev.h: signs by ballot into the 40-bit ring, 512 bits behind a ring that equals
the header, then the 69 bytes, PN9 and the xor8 / sum8 check on the wave) executed on the CPU under tests/emu/wave_emu.h and driven as
sonde_softin_dev_push_device drives k_softin_wxr (tests/emu/softin_wxr_emu.cpp).  The arbiter is the host tier on the same stream — sonde_wxr_softin_push for the
frames, sonde_wxr_print_frame for the text — and the recorded stdout of the compiled reference (tests/golden/wxr_softin_*.npz, tools/make_golden_wxr_softin.py) is
the second.  The same source is compiled by hipcc into k_softin_wxr; tests/test_gpu_softin_wxr_dev.py runs it there.

A consumer has no `finish`: every stream ends in idle bits, so no header is open at its end."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import wxr_softin_cases as W
from tools import synth

NAMES = sorted(W.build_cases())
ARGS = (["--json"], ["-r", "-t"], ["-R"], ["-v"], ["-r", "-v"], ["-v", "--json", "-t"])


@pytest.fixture(scope="module")
def emu():
    return W.load_emu()


@pytest.fixture(scope="module")
def host():
    return W.load_host()


def _arb(host, name):
    c = W.cases()[name]
    return W.host_frames(host, c["s"], c["pn9"], c["inv"], cache=name)


_one = {}


def _one_call(emu, name):
    if name not in _one:
        c = W.cases()[name]
        got, dropped, end = W.emu_frames(emu, c["s"], [len(c["s"])], c["pn9"], c["inv"])
        _one[name] = (got, [W.key(r) for r in got], dropped, W.state(end))
    return _one[name]


def test_header_record_and_lds_sizes(emu):
    for pn9 in (0, 1):
        assert emu.emu_wxr_header40(pn9) == int(W.HDR_HEX[bool(pn9)], 16)
    assert emu.emu_wxr_rec_bytes() == 176 == C.sizeof(W.Rec) and emu.emu_wxr_lds_bytes() == 216


# ---------------------------------------------------------------- 1. every case in one call against both arbiters
@pytest.mark.parametrize("name", NAMES)
def test_case_equals_host_arbiter(emu, host, name):
    c = W.cases()[name]
    want = _arb(host, name)
    if c["n"] is not None:
        assert len(want) == c["n"]                                # what the case is about, said by the arbiter
    if c["hb"] is not None:
        assert [w[0] for w in want] == c["hb"]
    if c["ok"] is not None:
        assert [W.verdict(w[1], c["pn9"])[3] for w in want] == c["ok"]
    got, keys, dropped, st = _one_call(emu, name)
    assert dropped == 0
    assert keys == [W.key(w, c["pn9"]) for w in want]             # hdr_bit, the bytes before and behind PN9, chkval, chkdat, the verdict, frame id, serial, counter
    assert st[0] == 0 and st[1] == len(c["s"])                    # searching again, every bit counted
    with np.errstate(invalid="ignore"):                           # the ring: the stream's last 40 bits, all of them held
        bits = ((c["s"] <= 0) if c["inv"] else (c["s"] >= 0)).astype(np.uint8)
    assert st[3] == int("".join(map(str, bits[-40:])), 2) and st[4] == (1 << 40) - 1


@pytest.mark.parametrize("name", W.GOLDEN_CASES)
def test_case_equals_recorded_reference(emu, host, name):
    g, c = W.load_golden(name), W.cases()[name]
    assert g["soft"].tobytes() == np.ascontiguousarray(c["s"], np.float32).tobytes() and g["argv"] == [["--softin"] + a for a in c["argv"]]
    for argv, ref in zip(g["argv"], g["stdout"]):
        o = W.opts_of(argv)
        assert (o["pn9"], o["inv"]) == (c["pn9"], c["inv"])
        got = _one_call(emu, name)[0]
        assert W.rec_text(host, got, argv) + b"\n" == ref, (name, argv)
        assert W.host_text(host, _arb(host, name), argv) + b"\n" == ref


def test_stream_start_wrong_variant_and_polarity(emu, host):
    g = lambda name: _one_call(emu, name)[0]                      # noqa: E731
    assert g("start_at_0")[0].hdr_bit == 39 and g("start_39_bits") == []
    assert g("clean_other_variant") == [] and g("clean_pn9_other_variant") == [] and g("clean_i") == [] and g("clean_pn9_i") == []
    assert len(g("clean")) == 4 and len(g("clean_pn9")) == 4
    # the first 39 bits of a stream cannot match whatever they are: the same stream behind one more bit does
    c = W.cases()["start_39_bits"]
    s = np.concatenate([np.float32([1.0]), c["s"]])
    assert [r.hdr_bit for r in W.emu_frames(emu, s, [len(s)])[0]] == [39]


def test_ring_behind_a_frame(emu, host):
    for name in ("ring_behind_frame", "ring_behind_frame_pn9"):
        c = W.cases()[name]
        got = _one_call(emu, name)[0]
        assert [r.hdr_bit for r in got] == [30 + 39, c["end"] + 0]                # the header ends in the first bit behind the frame
        assert bytes(got[1].raw)[:5] == bytes.fromhex(W.HDR_HEX[c["pn9"]]) and got[1].chk_ok == 1
        assert [r.hdr_bit for r in _one_call(emu, name + "_tail_flipped")[0]] == [30 + 39]
    got = _one_call(emu, "header_in_payload")[0]
    assert len(got) == 2 and bytes(got[0].raw)[30:35] == bytes.fromhex(W.HDR_HEX[False]) and got[0].chk_ok == 1


def test_zeros_and_nan(emu, host):
    for name in ("zeros_nan", "zeros_nan_i"):
        c = W.cases()[name]
        lo, hi = c["payload"]
        sym = c["s"][lo:hi]
        z = sym[sym == 0]
        assert len(z) > 30 and any(np.signbit(v) for v in z) and any(not np.signbit(v) for v in z) and np.isnan(sym).sum() > 15
        got = _one_call(emu, name)[0]
        bits = np.unpackbits(np.frombuffer(bytes(got[0].raw), np.uint8))[lo - 24:hi - 24]
        with np.errstate(invalid="ignore"):
            ge, gt = ((sym <= 0), (sym < 0)) if c["inv"] else ((sym >= 0), (sym > 0))
        assert (bits == ge).all() and not (bits == gt).all()      # the `>` / `<` mutation gives other bits
        assert (bits[sym == 0] == 1).all() and (bits[np.isnan(sym)] == 0).all()
    assert [W.key(r)[1:] for r in _one_call(emu, "zeros_nan")[0]] == [W.key(r)[1:] for r in _one_call(emu, "zeros_nan_i")[0]]


@pytest.mark.parametrize("softinv,inv", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_invert_stream_xor_invert(emu, host, softinv, inv):
    c = W.cases()["clean"]
    one = _one_call(emu, "clean")[1]
    s = c["s"] if softinv == inv else -c["s"]
    assert [W.key(r) for r in W.emu_frames(emu, s, [len(s)], False, inv, softinv)[0]] == one
    assert W.emu_frames(emu, -s, [len(s)], False, inv, softinv)[0] == []


# ---------------------------------------------------------------- 2. call cuts
def _cut_run(emu, name, calls):
    c = W.cases()[name]
    got, dropped, end = W.emu_frames(emu, c["s"], calls, c["pn9"], c["inv"])
    return [W.key(r) for r in got], dropped, W.state(end)


def _all_streams(emu, calls_of, names=NAMES):
    for name in names:
        _one_call(emu, name)
    with ThreadPoolExecutor(max_workers=8) as pool:              # (the emulator keeps its fibers per thread; ctypes releases the interpreter lock)
        res = list(pool.map(lambda name: _cut_run(emu, name, calls_of(name)), names))
    for name, r in zip(names, res):
        assert r == _one_call(emu, name)[1:], name                # records, nothing dropped, the end state


# a bit a call is a launch a bit: the streams of up to 1300 bits (every kind of case is among them) and one clean and one damaged stream of each variant
BIT_BY_BIT = [n for n in NAMES if len(W.build_cases()[n]["s"]) <= 1300] + ["clean", "clean_pn9", "flips", "flips_pn9"]


@pytest.mark.parametrize("cut", W.CUTS)
def test_fixed_cuts_equal_one_call(emu, cut):
    _all_streams(emu, lambda name: [cut], BIT_BY_BIT if cut == 1 else NAMES)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_cuts_equal_one_call(emu, seed):
    _all_streams(emu, lambda name: W.random_cuts(len(W.cases()[name]["s"]), 100 * seed + NAMES.index(name)))


def test_cuts_around_the_header_and_the_frames_last_bit(emu, host):
    for name in ("clean", "clean_pn9", "ring_behind_frame", "back_to_back", "flips"):
        c = W.cases()[name]
        n = len(c["s"])
        hb = _arb(host, name)[1][0]                               # the second frame: a frame lies in front of it
        one = _one_call(emu, name)[1:]
        last = hb + 512                                           # the frame's last bit
        for first in list(range(hb - 40, hb + 2)) + [last - 1, last, last + 1]:
            assert _cut_run(emu, name, [first, n]) == one, (name, first)
            # the end state inside the first call alone is the one-call state of that much of the stream
            a = W.emu_frames(emu, c["s"][:first], [first], c["pn9"], c["inv"])
            b = W.emu_frames(emu, c["s"][:first], [hb - 45, 3, 64, 1, n], c["pn9"], c["inv"])
            assert ([W.key(r) for r in a[0]], W.state(a[2])) == ([W.key(r) for r in b[0]], W.state(b[2])), (name, first)


# ---------------------------------------------------------------- 3. the record cap
def _cap_stream():
    first = W.cases()["back_to_back"]["s"]
    return first, np.concatenate([first, W.cases()["header_in_payload"]["s"]])


def test_record_cap_drops_and_the_next_call_is_intact(emu, host):
    first, s = _cap_stream()
    want = W.host_frames(host, s, cache="cap")
    assert len(want) == 7
    got, dropped, end = W.emu_frames(emu, s, [len(first), len(s) - len(first)], cap=3)
    assert dropped == 2 and len(got) == 5                        # five frames in the first call, three of them kept; the second call's two are all there
    assert [W.key(r) for r in got] == [W.key(w) for w in want[:3] + want[5:]]
    assert end.mode == 0 and end.bits_in == len(s)


# ---------------------------------------------------------------- 4. the check on the wave
def _end(emu, by69, pn9):
    out = (C.c_uint * 75)()
    assert emu.emu_wxr_end(bytes(by69), int(pn9), out) == 0
    return (bytes(out[6:75]),) + tuple(out[:6])


@pytest.mark.parametrize("pn9", [False, True])
def test_check_on_the_wave_every_single_bit_flip_of_8_random_frames(emu, pn9):
    """8 random frames with a fitting check: the frame passes; every single-bit flip of the 69 bytes gives the serial xor8sum's chkval / chkdat, and the verdict
    fails exactly when the flip lies in the 55 bytes from ofs"""
    rng = np.random.default_rng(69 + pn9)
    ofs = 8 if pn9 else 6
    for _ in range(8):
        f = W.refit(rng.integers(0, 256, 69, dtype=np.uint8).tobytes(), pn9)
        assert _end(emu, f, pn9) == W.verdict(f, pn9) and W.verdict(f, pn9)[3] == 1
        for bit in range(8 * 69):
            g = bytearray(f); g[bit >> 3] ^= 0x80 >> (bit & 7)
            got = _end(emu, g, pn9)
            assert got == W.verdict(g, pn9), bit
            assert got[3] == (0 if ofs <= bit >> 3 < ofs + 55 else 1), bit
    for f in (bytes(69), bytes([0xFF] * 69)):
        assert _end(emu, f, pn9) == W.verdict(f, pn9)
    x = W.verdict(bytes(69), True)[0]
    assert x[:6] == bytes(6) and x[6:] == synth.WXR_PN9[:63]      # PN9 starts at byte 6 with the sequence's first byte


# ---------------------------------------------------------------- 5. the printer from the record
@pytest.mark.parametrize("name", NAMES)
def test_print_decoded_equals_print_frame(emu, host, name):
    c = W.cases()[name]
    got, want = _one_call(emu, name)[0], _arb(host, name)
    pn, i = (["--pn9"] if c["pn9"] else []), (["-i"] if c["inv"] else [])
    for a in ARGS:
        argv = a + pn + i
        assert W.rec_text(host, got, argv) == W.host_text(host, want, argv), (name, argv)


def test_text_comes_from_the_record(emu, host):
    got = _one_call(emu, "clean")[0]
    text = W.rec_text(host, got, ["--json", "-v"])
    assert text.count(b"[OK]") == 4 and text.count(b'"type"') == 2 and b"[NO]" not in text
    bad = []
    for r in got:
        q = W.Rec.from_buffer_copy(bytes(r)); q.chk_ok = 0
        bad.append(q)
    text = W.rec_text(host, bad, ["--json", "-v"])
    assert text.count(b"[NO]") == 4 and b"[OK]" not in text and b'"type"' not in text
    q = W.Rec.from_buffer_copy(bytes(got[1])); q.sn = 7; q.cnt = 9; q.chkval = 0x1234; q.chkdat = 0xABCD
    assert W.rec_text(host, [q], ["-v"]).startswith(b" (7)  [    9] ") and b"[ABCD:1234]" in W.rec_text(host, [q], ["-v"])
    q = W.Rec.from_buffer_copy(bytes(got[1])); q.raw[0] = 0x0F
    assert W.rec_text(host, [q], ["-R"]).startswith(b"00001111") and W.rec_text(host, [got[1]], ["-R"]).startswith(b"10101010")


# ---------------------------------------------------------------- 6. a stand-alone program under the sanitizers
def test_sanitized_standalone_replay_of_the_call_cuts(host, tmp_path):
    """the emulator translation unit under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program with its own main (tests/emu/softin_wxr_replay.cpp),
    run as a process of its own, outside the interpreter, in the environment as it is (the sanitizer runtimes are linked into the program)"""
    exe = str(tmp_path / "softin_wxr_replay_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, os.path.join(W.EMU_DIR, "softin_wxr_replay.cpp"), W.EMU_SRC])

    def run(s, softinv, inv, pn9, cap, calls):
        p = tmp_path / "s.f32"
        np.ascontiguousarray(s, np.float32).tofile(p)
        r = subprocess.run([exe, str(p), str(int(softinv)), str(int(inv)), str(int(pn9)), str(cap)] + calls, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert b"ERROR" not in r.stderr and b"runtime error" not in r.stderr
        return r

    for name, calls in [("clean_pn9", ["1"]), ("ring_behind_frame", ["41"]), ("zeros_nan_i", ["63"]), ("flips", ["65", "553"])]:
        c = W.cases()[name]
        r = run(c["s"], False, c["inv"], c["pn9"], 64, calls)
        argv = ["-r", "-v"] + (["--pn9"] if c["pn9"] else [])
        assert r.stdout == W.host_text(host, _arb(host, name), argv) and len(_arb(host, name)) > 0, name
    first, s = _cap_stream()
    r = run(s, False, False, False, 3, [str(len(first)), "4000"])
    assert b"5 frames, 2 dropped" in r.stderr
