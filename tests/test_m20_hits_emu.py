"""The per-hit DEVICE decoder of M20 hits in base-rate and mixed engines (radiosonde_auto_rx_amd/csrc/sonde_m20_hits_dev.h: differential decoding into the channel's
persistent bit characters, bits2bytes, frame and block checksum, one wavefront per hit record) executed on the CPU under tests/emu/wave_emu.h and launched as
k_m20_hits is (tests/emu/m20_hits_emu.cpp).  The arbiter is a numpy restatement of mxx_bytes followed by the library's own sonde_m20_frame_finish
(tests/m20_hits_cases.py): every constructed record must come out equal in all 208 bytes, and the channels' characters with it.  The same source is compiled by hipcc
into k_m20_hits; tests/test_gpu_m20_hits.py runs it there on the same records.  Argument checks of the C entry points that need no GPU are at the end."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import m20_hits_cases as M
from radiosonde_auto_rx_amd.engine import SondeM20Frame


@pytest.fixture(scope="module")
def emu():
    return M.load_emu()


_ref = {}


def _arbiter():
    if "a" not in _ref:
        recs, nch = M.records()
        _ref["a"] = M.arbiter(recs, nch)
    return _ref["a"]


def _named(frames):
    return {r[0]: f for r, f in zip(M.records()[0], frames)}


# ---------------------------------------------------------------- 1. every record against the arbiter
def test_every_record_and_the_characters_equal_the_arbiter(emu):
    recs, nch = M.records()
    want, want_chars = _arbiter()
    got, chars, done = M.emu_run(emu, recs, nch, grid=nch)
    assert len(got) == len(recs) == len(want) and done == (len(recs), 0)
    for (name, *_), g, w in zip(recs, got, want):
        assert C.sizeof(g) == 208 and M.key(g) == M.key(w), name
    assert np.array_equal(chars, want_chars)


def test_the_cases_cover_both_checksum_verdicts_every_block_verdict_and_the_clamped_length(emu):
    recs, nch = M.records()
    rec = _named(M.emu_run(emu, recs, nch, grid=3)[0])
    assert {f.cs_ok for f in rec.values()} == {0, 1} and {f.blk_ok for f in rec.values()} == {-1, 0, 1}
    assert (rec["good"].cs_ok, rec["good"].blk_ok, rec["good"].fw, rec["good"].len) == (1, 1, 6, 0x46)
    assert rec["bad_checksum"].cs_ok == 0 and rec["blk_zero"].blk_ok == -1 and rec["blk_bad"].blk_ok == 0 and rec["fw8"].fw == 8 and rec["fw8"].cs_ok == 1
    other_level = M.arbiter([("", M.hard_bits(M.frame165(6, fw=6), 0), 1320, 0, 0.0)], 1)[0][0]
    assert bytes(rec["fw6_first_bit_1"].frame) == bytes(other_level.frame) and rec["fw6_first_bit_1"].cs_ok == 1      # the level of the first bit says nothing
    # the length byte behind the differential code: its top bit is the frame's first character, which is never '1'
    for L in M.LENGTHS:
        f = rec["len_%02x" % L]
        assert f.frame[0] == L & 0x7F and f.len == (L & 0x7F) + 1, hex(L)
    assert [rec["len_%02x" % L].cs_ok for L in M.LENGTHS] == [1, 0, 1, 1, 1, 1, 1, 1]      # 0x00: nothing summed; 0x01: the checksum would lie on the length byte
    assert rec["len_00"].fw == 0 and rec["len_00"].cs_calc == 0 and rec["len_01"].fw == 0 and rec["len_45_bad"].cs_ok == 0
    assert rec["len_ff"].len == 0x80                                                       # aux bytes 58: the longest frame the bits can announce
    # the verdict function alone, on frame bytes as they stand: here 0x85, 0x86 and 0xFF are what they say, and the clamp at 64 aux bytes is reached
    lens = {}
    for name, fr in M.verdict_frames().items():
        got = SondeM20Frame()
        C.memset(C.byref(got), 0, C.sizeof(got))
        assert emu.emu_m20_verdicts(fr, C.byref(got)) == 0
        want = M.finish(fr)
        assert (got.len, got.fw, got.cs_calc, got.cs_ok, got.blk_ok) == (want.len, want.fw, want.cs_calc, want.cs_ok, want.blk_ok), name
        # (0x00: nothing is summed, which counts as good; 0x01: the checksum would lie on the length byte itself)
        assert got.cs_ok == (1 if name.startswith("len_00") else 0 if name.startswith("len_01") else int(name.endswith("good"))), name
        lens[name] = got.len
    assert [lens["len_%02x_good" % L] for L in M.LENGTHS] == [0x01, 0x02, 0x45, 0x46, 0x47, 0x86, 0x86, 0x86]


def test_short_records_and_what_stays_behind_the_terminator(emu):
    recs, nch = M.records()
    rec = _named(M.emu_run(emu, recs, nch, grid=nch + 5)[0])                               # (more workgroups than channels)
    for nb in M.SHORT:
        f = rec["nbits_%d" % nb]
        assert f.nbits == nb and not any(f.frame[(nb + 7) // 8:])                          # a fresh channel: zeros behind the bits that exist
    assert (rec["nbits_1319"].frame[164] & 1) == 0 and any(rec["nbits_1319"].frame[:165])
    first, short, last, fresh = rec["chain_full_1"], rec["chain_short"], rec["chain_full_2"], rec["short_fresh"]
    assert first.nbits == last.nbits == 1320 and short.nbits == fresh.nbits == 700
    # 700 bits: bytes 0 .. 86 are the short frame's; byte 87 holds four of its bits (0xF0), the terminator (0x08) and three characters the channel held before
    # (0x07); bytes 88 .. 164 are what the channel held before
    assert bytes(short.frame[:87]) == bytes(fresh.frame[:87]) and (short.frame[87] & 0xF0) == (fresh.frame[87] & 0xF0) and (short.frame[87] & 0x08) == 0
    assert bytes(short.frame[88:165]) == bytes(first.frame[88:165]) and any(first.frame[88:165])
    assert (short.frame[87] & 0x07) == (first.frame[87] & 0x07)
    assert not any(fresh.frame[88:]) and (fresh.frame[87] & 0x0F) == 0
    assert bytes(last.frame) == bytes(M.arbiter([("", M.hard_bits(M.frame165(43, good=False)), 1320, 0, 0.0)], 1)[0][0].frame)      # a full frame leaves nothing of the earlier ones
    assert (short.mv, fresh.channel != short.channel, first.channel == short.channel == last.channel) == (np.float32(-0.82), True, True)


# ---------------------------------------------------------------- 2. the launch: grid sizes, the ring
def test_records_do_not_depend_on_the_grid(emu):
    recs, nch = M.records()
    want, want_chars = _arbiter()
    for grid in (1, 3, nch + 7):
        got, chars, done = M.emu_run(emu, recs, nch, grid=grid)
        assert [M.key(g) for g in got] == [M.key(w) for w in want] and np.array_equal(chars, want_chars) and done == (len(recs), 0), grid


def test_a_ring_that_wraps_with_done_moved_in_two_launches(emu):
    recs, _ = M.records()
    six = [r for r in recs if r[0].startswith("chain") or r[0].startswith("between")] + [recs[0]]
    renumber = {c: i for i, c in enumerate(dict.fromkeys(r[3] for r in six))}                # their four channels as 0 .. 3
    six = [(n, b, nb, renumber[ch], mv) for n, b, nb, ch, mv in six]
    assert len(six) == 6
    want, want_chars = M.arbiter(six, 4)
    for grid in (1, 3):
        # max_frames 4: records 0 .. 2 in slots 0 .. 2, then records 3 .. 5 in slots 3, 0, 1; the characters go from launch to launch
        a, chars, done = M.emu_run(emu, six[:3], 4, grid=grid, max_frames=4, start=0)
        assert done == (3, 0)
        b, chars, done = M.emu_run(emu, six[3:], 4, grid=grid, max_frames=4, start=3, chars=chars)
        assert done == (6, 0)
        assert [M.key(f) for f in a + b] == [M.key(w) for w in want] and np.array_equal(chars, want_chars), grid
    # six records queued into a ring of four since the last launch: only the last four are there; they are decoded once each, on characters that have not seen
    # the two that were lost
    got, chars, done = M.emu_run(emu, six, 4, grid=3, max_frames=4, start=0)
    want4, want4_chars = M.arbiter(six[2:], 4)
    assert [M.key(f) for f in got] == [M.key(w) for w in want4] and np.array_equal(chars, want4_chars) and done == (6, 0)


def test_a_launch_with_nothing_queued_writes_nothing(emu):
    out = (SondeM20Frame * 2)()
    C.memset(out, 0xEE, C.sizeof(out))
    d = (C.c_uint * 2)(5, 0)
    bits, nb, ch = np.zeros((2, 165), np.uint8), np.zeros(2, np.int32), np.zeros(2, np.int32)
    chars = np.full((1, M.CHARS), 0x5A, np.uint8)
    assert emu.emu_m20_hits_run(bits.ctypes.data, nb.ctypes.data, ch.ctypes.data, None, 1, 2, 5, 3, chars.ctypes.data, out, d) == 0
    assert bytes(out) == b"\xEE" * C.sizeof(out) and (d[0], d[1]) == (5, 0) and (chars == 0x5A).all()


# ---------------------------------------------------------------- 3. a stand-alone program under the sanitizers
def test_sanitized_standalone_replay_of_the_records(emu, tmp_path):
    """the emulator translation unit under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program with its own main (tests/emu/m20_hits_replay.cpp),
    run as a process of its own, outside the interpreter, in the environment as it is (the sanitizer runtimes are linked into the program): the same records, the
    same lines.  The bit and character buffers are exactly as long as the kernel may index, so a read or write beyond them is an error there."""
    exe = str(tmp_path / "m20_hits_replay_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, M.REPLAY_SRC, M.EMU_SRC])
    recs, nch = M.records()
    want, want_chars = _arbiter()
    p = tmp_path / "hits.bin"
    np.stack([r[1] for r in recs]).tofile(p)
    args = [exe, str(p), "3", str(nch)]
    for _, _, nb, ch, mv in recs:
        args += [str(nb), str(ch), repr(float(mv))]
    r = subprocess.run(args, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"ERROR" not in r.stderr and b"runtime error" not in r.stderr

    def line(f):
        return "%d %d %d %d %d %d %d %d %s %s" % (f.channel, f.nbits, f.len, f.cs_ok, f.cs_calc, f.blk_ok, f.fw, f.mv_pos, np.float32(f.mv).tobytes()[::-1].hex(),
                                                  bytes(f.frame).hex())
    lines = r.stdout.decode().splitlines()
    assert lines[:len(recs)] == [line(w) for w in want]
    assert lines[len(recs):] == [bytes(c).hex() for c in want_chars]
    assert b"%d records, done %d ticket 0" % (len(recs), len(recs)) in r.stderr


# ---------------------------------------------------------------- 4. the C entry points, as far as they go without a GPU
def test_entry_points_check_their_arguments_before_the_device_is_touched():
    import torch
    from radiosonde_auto_rx_amd.engine import decode_m20_hits_device, lib, m20_entry, SondeError
    L = lib()
    fn = m20_entry("sonde_m20_decode_device")
    E_ARG, E_NOGPU = -1, -2
    bits, nb, ch = np.zeros((2, 165), np.uint8), np.array([1320, 700], np.int32), np.array([0, 1], np.int32)
    out = (SondeM20Frame * 2)()
    B, N, CH = bits.ctypes.data, nb.ctypes.data, ch.ctypes.data
    assert fn(None, N, CH, None, 2, 2, out, None) == E_ARG and fn(B, None, CH, None, 2, 2, out, None) == E_ARG and fn(B, N, None, None, 2, 2, out, None) == E_ARG
    assert fn(B, N, CH, None, 2, 2, None, None) == E_ARG and fn(B, N, CH, None, -1, 2, out, None) == E_ARG and fn(B, N, CH, None, 2, 0, out, None) == E_ARG
    assert fn(B, N, CH, None, 2, 1, out, None) == E_ARG                              # channel 1 of one channel
    for bad in (np.array([1321, 0], np.int32), np.array([0, -1], np.int32)):
        assert fn(B, bad.ctypes.data, CH, None, 2, 2, out, None) == E_ARG
    assert fn(B, N, np.array([0, -1], np.int32).ctypes.data, None, 2, 2, out, None) == E_ARG
    assert fn(B, N, CH, None, 0, 2, out, None) == 0                                  # nothing to do
    assert m20_entry("sonde_engine_fetch_m20_lagged")(None, out, 2, 1) == E_ARG and L.sonde_engine_fetch_m20(None, out, 2, 0) == E_ARG
    if not torch.cuda.is_available():
        assert fn(B, N, CH, None, 2, 2, out, None) == E_NOGPU
        with pytest.raises(SondeError):
            decode_m20_hits_device(bits, nb, ch, 2)
