"""The per-hit DEVICE decoders of generic engines (radiosonde_auto_rx_amd/csrc/sonde_family_hits_dev.h: Meisei BCH(63,51), iMet-54 Hamming(8,4) and check sums,
MTS01 CRC-16, RS92 RS(255,231), one wavefront per hit record) executed on the CPU under tests/emu/wave_emu.h and launched as k_family_hits is
(tests/emu/family_hits_emu.cpp).  The arbiter is the host tier sonde_<kind>_dec_frame on the same soft bits (tests/test_*_native.py pin it to the compiled
reference): every constructed hit gives a record, sonde_<kind>_dec_decoded / sonde_rs92_dec_corrected give text from it, and that text is compared byte for byte
under `-r -v` and under the receivers' JSON options.  The same source is compiled by hipcc into k_family_hits; tests/test_gpu_family_hits.py runs it there on the
same hits.  Argument checks of the C entry points that need no GPU are at the end."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import family_hits_cases as F
from radiosonde_auto_rx_amd.family import DEVICE_KINDS, FamilyHit

KINDS = F.KINDS


@pytest.fixture(scope="module")
def emu():
    return F.load_emu()


_recs = {}


def _records(emu, kind):
    """the kind's hits through one emulated launch per --ecc value (a workgroup per record): {ecc: (hits, records)}"""
    if kind not in _recs:
        _recs[kind] = {e: (hs, F.emu_run(emu, kind, e, [h[1] for h in hs], [h[2] for h in hs], grid=len(hs))[0]) for e, hs in F.by_ecc(kind)}
    return _recs[kind]


def _named(emu, kind):
    return {h[0]: r for hs, rs in _records(emu, kind).values() for h, r in zip(hs, rs)}


# ---------------------------------------------------------------- 1. record -> text against the arbiter
@pytest.mark.parametrize("kind", KINDS)
def test_text_from_the_record_equals_the_host_tier_on_the_soft_bits(emu, kind):
    for ecc, (hs, recs) in _records(emu, kind).items():
        assert len(recs) == len(hs)
        for (name, s, mv, _), r in zip(hs, recs):
            assert r["kind"] == DEVICE_KINDS[kind] and r["nbits"] == len(s) and r["decoded"] == int(len(s) == F.NB[kind]), name
            assert r["mv_pos"] == 0 and np.float32(r["mv"]) == np.float32(mv)
        for opts in [F.raw_opts(kind, ecc)] + ([F.JSON[kind]] if ecc else []):
            want = F.text_by_frame(kind, hs, opts)
            got = F.text_by_record(kind, hs, recs, opts)
            for (name, *_), w, g in zip(hs, want, got):
                assert g == w, (name, opts)
            assert sum(1 for w in want if w.strip()) >= len(hs) // 2             # (the comparison is not one of empty strings)
    if kind in ("IMET5", "RS92"):                                                # (a JSON object per good frame; Meisei pairs frames, MTS01's builder has no position)
        hs, recs = _records(emu, kind)[1]
        assert any(l.startswith("{") for t in F.text_by_record(kind, hs, recs, F.JSON[kind]) for l in t.splitlines())


# ---------------------------------------------------------------- 2. what the cases are about, said by the records
def test_meisei_cases_flips_padding_parity_every_block_ecc_off_zeros(emu):
    import meisei_softin_cases as ME
    H = ME.load_host()
    rec = _named(emu, "MEISEI")
    for name, (bits, ecc, exp) in ME.bch_named(H).items():
        r = rec[name]
        want_bits, want_be = ME.model_end(H, bits, ecc)
        assert r["data"][:75] == want_bits and r["aux"] == want_be and not any(r["data"][75:]), name
        assert {k: v for k, v in enumerate(r["aux"]) if v} == exp, name
        assert r["v"][:2] == [sum(v >= 0xE for v in want_be), sum(v != 0 for v in want_be)] and r["v"][2:] == [0, 0, 0, 0], name
    assert rec["ecc_off"]["aux"] == bytes(12) and rec["ecc_off"]["data"][:75] == ME.pack(ME.bch_named(H)["ecc_off"][0])
    assert {rec["three_pad"]["aux"][2], rec["three_none"]["aux"][2], rec["s1_zero"]["aux"][2]} == {0xF, 0xE}
    # exact zeros and -0.0: both are a 1 (s >= 0); with `>` the bits differ
    hit = next(h for h in F.hits("MEISEI") if h[0] == "zeros")
    s = hit[1]
    assert (s == 0).sum() == 200 and np.signbit(s[s == 0]).sum() == 100
    assert rec["zeros"]["data"][:75] == ME.model_frame(H, s, 1)[0]
    hard_gt = s > 0
    assert ME.pack(ME.HDR24 + [int(b) for b in (hard_gt[0::2] == hard_gt[1::2])]) != ME.model_frame(H, s, 0)[0]


def test_imet54_cases_repairs_and_failures_around_88_and_104_check_sums_ecc_off(emu):
    rec = _named(emu, "IMET5")
    v = lambda name: rec[name]["v"][:5]                                          # noqa: E731  ecc_frm, ecc_tlm, ecc_std, crc_std, crc_cont
    assert v("no_error") == [0, 0, 0, 1, 0]                                      # (synth frames carry the standard check sum unless asked otherwise)
    assert v("fix_at_87")[:3] == [1, 1, 1] and v("fix_at_88")[:3] == [1, 0, 1] and v("fix_at_103")[:3] == [1, 0, 1] and v("fix_at_104")[:3] == [0, 0, 0]
    assert v("f0_at_87")[:3] == [-1, -1, -1] and v("f0_at_88")[:3] == [-1, 1, -1] and v("f0_at_103")[:3] == [-1, 1, -1] and v("f0_at_104")[:3] == [1, 1, 1]
    assert v("check_std")[3:] == [1, 0] and v("check_cont")[3:] == [0, 1] and v("check_none")[3:] == [0, 0]      # each check sum good alone, and neither
    # without --ecc nothing is repaired: the damaged codeword 30 has no table entry, which counts as uncorrectable in front of 88
    assert v("ecc_off_damaged")[:3] == [-1, -1, -1] and v("ecc_off_clean")[:3] == [0, 0, 0]
    assert rec["ecc_off_damaged"]["data"][:108] != rec["ecc_off_clean"]["data"][:108]
    for name in ("no_error", "two_flips", "check_cont"):
        assert not any(rec[name]["data"][108:]) and rec[name]["aux"] == bytes(12) and rec[name]["v"][5] == 0


def test_mts01_cases_crc_good_and_bad_and_the_unflip_of_a_negative_score(emu):
    import mts01_softin_cases as MT
    rec = _named(emu, "MTS01")
    hs = {h[0]: h for h in F.hits("MTS01")}
    for name, r in rec.items():
        if name == "short":
            continue
        s = hs[name][1] if hs[name][2] >= 0 else -hs[name][1]
        by, val, dat, ok, _ = MT.model_frame(s)
        assert r["data"][:131] == by and r["v"][:3] == [val, dat, ok] and r["v"][3:] == [0, 0, 0] and not any(r["data"][131:]), name
    assert [rec[n]["v"][2] for n in ("good", "data_flip", "crc_flip", "negative_mv", "positive_mv_inverted_bits", "good_after")] == [1, 0, 0, 1, 0, 1]
    assert rec["negative_mv"]["mv"] < 0 and rec["negative_mv_zeros"]["data"] == rec["zeros"]["data"]      # -(+-0.0) is still a 1


def test_rs92_cases_up_to_the_codes_limit_and_in_the_parity_bytes(emu):
    import rs92_softin_cases as RS
    rec = _named(emu, "RS92")
    ec = lambda name: rec[name]["v"][0]                                          # noqa: E731
    assert [ec(n) for n in ("clean", "one_byte", "twelve_bytes", "parity_bytes", "parity_and_message", "start_stop_bits", "clean_after")] == [0, 1, 12, 3, 12, 0, 0]
    assert ec("thirteen_bytes") < 0
    fr = RS.frames()
    for name, k in (("clean", 0), ("one_byte", 1), ("twelve_bytes", 2), ("parity_bytes", 4), ("parity_and_message", 5), ("start_stop_bits", 3), ("clean_after", 6)):
        assert rec[name]["data"] == bytes(fr[k]), name                           # repaired back to the frame that was sent, the header bytes in front
    assert rec["thirteen_bytes"]["data"] != bytes(fr[3]) and rec["thirteen_bytes"]["data"][:6] == bytes(fr[3][:6])


@pytest.mark.parametrize("kind", KINDS)
def test_a_hit_one_bit_short_is_marked_and_noise_is_decoded_to_whatever_it_is(emu, kind):
    rec = _named(emu, kind)
    r = rec["short"]
    assert r["decoded"] == 0 and r["nbits"] == F.NB[kind] - 1 and r["v"] == [0] * 6 and r["aux"] == bytes(12) and r["data"] == bytes(240)
    assert rec["noise"]["decoded"] == 1 and rec["noise"]["nbits"] == F.NB[kind]


# ---------------------------------------------------------------- 3. the launch: grid sizes, the ring
@pytest.mark.parametrize("kind", KINDS)
def test_records_do_not_depend_on_the_grid_and_the_ring_wraps(emu, kind):
    ecc, hs = F.by_ecc(kind)[0]
    hs = hs[:10] if len(hs) >= 10 else (hs * 10)[:10]
    softs, mvs = [h[1] for h in hs], [h[2] for h in hs]
    one, done = F.emu_run(emu, kind, ecc, softs, mvs, grid=1)
    assert done == (10, 0) and [r["channel"] for r in one] == list(range(10))
    for grid in (3, 10, 17):                                                     # (17: more workgroups than records)
        got, done = F.emu_run(emu, kind, ecc, softs, mvs, grid=grid)
        assert [F.rec_key(r) for r in got] == [F.rec_key(r) for r in one] and done == (10, 0), grid
    body = lambda r: F.rec_key(r)[1:]                                            # noqa: E731  (everything but the channel, which is the ring slot here)
    # max_frames = 4, the counter at 6: records 6 .. 9 land in slots 2, 3, 0, 1
    for grid in (1, 3, 7):
        got, done = F.emu_run(emu, kind, ecc, softs[6:], mvs[6:], grid=grid, max_frames=4, start=6)
        assert [r["channel"] for r in got] == [2, 3, 0, 1] and [body(r) for r in got] == [body(r) for r in one[6:]] and done == (10, 0), grid
    # ten hits queued into a ring of four since the last launch (done = 0): only the last four are there, and they are decoded once each
    got, done = F.emu_run(emu, kind, ecc, softs, mvs, grid=3, max_frames=4, start=0)
    assert [body(r) for r in got] == [body(r) for r in one[6:]] and done == (10, 0)


def test_a_launch_with_nothing_queued_writes_nothing(emu):
    out = (FamilyHit * 2)()                                                      # counter == done: no record is the launch's
    C.memset(out, 0xEE, C.sizeof(out))
    d = (C.c_uint * 2)(5, 0)
    soft = np.zeros((2, F.NB["MTS01"]), np.float32); nb = np.zeros(2, np.int32)
    assert emu.emu_family_run(71, 1, soft.ctypes.data, F.NB["MTS01"], nb.ctypes.data, None, 2, 5, 5, 3, out, d) == 0
    assert bytes(out) == b"\xEE" * C.sizeof(out) and (d[0], d[1]) == (5, 0)


# ---------------------------------------------------------------- 4. a stand-alone program under the sanitizers
def test_sanitized_standalone_replay_of_the_hits(emu, tmp_path):
    """the emulator translation unit under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program with its own main (tests/emu/family_hits_replay.cpp),
    run as a process of its own, outside the interpreter, in the environment as it is (the sanitizer runtimes are linked into the program): the same hits, the same
    lines.  The soft-bit buffer is exactly max_frames x nbits long, so a read beyond a hit is an error there."""
    exe = str(tmp_path / "family_hits_replay_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, F.REPLAY_SRC, F.EMU_SRC])

    def line(r):
        return "%d %d %d %d " % (r["channel"], r["kind"], r["nbits"], r["decoded"]) + " ".join(str(v) for v in r["v"]) + " " + r["aux"].hex() + " " + r["data"].hex()

    for kind in KINDS:
        for ecc, (hs, recs) in _records(emu, kind).items():
            soft = np.zeros((len(hs), F.NB[kind]), np.float32)
            for i, h in enumerate(hs):
                soft[i, :len(h[1])] = h[1]
            p = tmp_path / "hits.f32"
            soft.tofile(p)
            args = [exe, str(p), str(DEVICE_KINDS[kind]), str(ecc), str(F.NB[kind]), "3", str(len(hs)), "0"]
            for h in hs:
                args += [str(len(h[1])), repr(float(h[2]))]
            r = subprocess.run(args, capture_output=True, timeout=300)
            assert r.returncode == 0, r.stderr.decode()[-2000:]
            assert b"ERROR" not in r.stderr and b"runtime error" not in r.stderr
            assert r.stdout.decode().splitlines() == [line(x) for x in recs], (kind, ecc)
            assert b"%d records, done %d ticket 0" % (len(hs), len(hs)) in r.stderr


# ---------------------------------------------------------------- 5. the C entry points, as far as they go without a GPU
def test_direct_entry_arguments_are_checked_before_the_device_is_touched():
    import torch
    from radiosonde_auto_rx_amd.engine import lib
    L = lib()
    fn = L.sonde_family_decode_device
    fn.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
    E_ARG, E_NOGPU = -1, -2
    nb = F.NB["MEISEI"]
    soft = np.zeros((2, 2400), np.float32); n = np.array([nb, nb - 1], np.int32); out = (FamilyHit * 2)()
    ok = lambda kind, ecc, s, stride, nn, cnt, o: fn(kind, ecc, s, stride, nn, cnt, o)      # noqa: E731
    S, N, O = soft.ctypes.data, n.ctypes.data, C.addressof(out)
    for bad_kind in (0, 41, 9, 6, 31, 99, -11):                                 # (LMS6 and MRZ are not kinds of this decoder)
        assert ok(bad_kind, 1, S, 2400, N, 2, O) == E_ARG
    assert ok(11, 1, S, 2400, N, -1, O) == E_ARG
    assert ok(11, 1, None, 2400, N, 2, O) == E_ARG and ok(11, 1, S, 2400, None, 2, O) == E_ARG and ok(11, 1, S, 2400, N, 2, None) == E_ARG
    assert ok(92, 0, S, 2400, N, 2, O) == E_ARG                                  # RS92 always corrects
    assert ok(11, 1, S, nb - 1, N, 2, O) == E_ARG and ok(92, 1, S, 2339, N, 2, O) == E_ARG      # a stride shorter than the kind's frame
    neg = np.array([nb, -1], np.int32); over = np.array([nb, 2401], np.int32)
    assert ok(11, 1, S, 2400, neg.ctypes.data, 2, O) == E_ARG and ok(11, 1, S, 2400, over.ctypes.data, 2, O) == E_ARG
    assert ok(11, 1, S, 2400, N, 0, O) == 0                                      # nothing to do
    if not torch.cuda.is_available():
        for kind in (11, 54, 71, 92):
            assert ok(kind, 1, S, 2400, N, 2, O) == E_NOGPU
        assert L.sonde_engine_set_family(None, 11, 1) == E_ARG and L.sonde_engine_fetch_family(None, O, 2, 0) == E_ARG
