"""The per-hit DEVICE decoder of generic engines carrying MRZ (radiosonde_auto_rx_amd/csrc/sonde_mrz_hits_dev.h: bits, bytes and the CRC-16 under both frame lengths,
one wavefront per hit record) executed on the CPU under tests/emu/wave_emu.h and launched as k_mrz_hits is (tests/emu/mrz_hits_emu.cpp).  The arbiter is the host
tier sonde_mrz_dec_frame on the same soft bits through a decoder that has seen the same history (tests/test_mrz_native.py pins it to the compiled reference):
sequences of hits go through one decoder with .hit and through another with .decoded on the emulator's records, and after every hit the text — under `-r -v` and
under the receivers' JSON options — and sonde_mrz_dec_frame_bits are equal.  The same source is compiled by hipcc into k_mrz_hits; tests/test_gpu_mrz_hits.py runs
it there on the same hits.  Argument checks of the C entry points that need no GPU are at the end."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import mrz_hits_cases as Z
from radiosonde_auto_rx_amd.engine import SondeError
from radiosonde_auto_rx_amd.family import DEVICE_KINDS, DEVICE_KINDS_ALL, FamilyDecoder, FamilyHit


@pytest.fixture(scope="module")
def emu():
    return Z.load_emu()


_recs = {}


def _records(emu):
    """every sequence through one emulated launch (a workgroup per record): {name: (ofs, hits, records)}"""
    if not _recs:
        for name, ofs, hs in Z.sequences():
            recs, done = Z.emu_run(emu, ofs, [h[1] for h in hs], [h[2] for h in hs], grid=len(hs))
            assert done == (len(hs), 0)
            _recs[name] = (ofs, hs, recs)
    return _recs


def _named(emu, seq="main"):
    _, hs, recs = _records(emu)[seq]
    return {h[0]: r for h, r in zip(hs, recs)}


# ---------------------------------------------------------------- 1. record -> text against the arbiter, hit by hit
@pytest.mark.parametrize("seq", ["main", "ofs0", "ofs16"])
def test_text_and_frame_length_after_every_hit_equal_the_host_tier(emu, seq):
    ofs, hs, recs = _records(emu)[seq]
    assert len(recs) == len(hs)
    for i, ((name, s, mv), r) in enumerate(zip(hs, recs)):
        assert r["kind"] == Z.KIND and r["nbits"] == len(s) and r["decoded"] == int(len(s) == Z.NB) and r["channel"] == i, name
        assert r["mv_pos"] == 0 and np.float32(r["mv"]) == np.float32(mv)
    for opts in (Z.RAW, Z.JSON):
        want = Z.text_by_frame(hs, opts, ofs)
        got = Z.text_by_record(hs, recs, opts, ofs)
        for (name, *_), w, g in zip(hs, want, got):
            assert g[0] == w[0] and g[1] == w[1], (name, opts, w, g)
    want = Z.text_by_frame(hs, Z.RAW, ofs)
    assert all(w[0].strip() for w in want) and any("[OK]" in w[0] for w in want)            # (the comparison is not one of empty strings)
    assert {g[2] for g in got} == {408, 384}                                               # (and the decoder stood at both lengths)


# ---------------------------------------------------------------- 2. what the cases are about, said by the records and the arbiter's text
def test_every_complete_record_is_the_model_of_its_soft_bits(emu):
    for seq, (ofs, hs, recs) in _records(emu).items():
        for (name, s, _), r in zip(hs, recs):
            if len(s) < Z.NB:
                continue
            data, v = Z.model(s, ofs)
            assert r["data"][:52] == data and not any(r["data"][51:]) and r["aux"] == bytes(12), (seq, name)
            assert [x & 0xFFFFFFFF for x in r["v"]] == v, (seq, name, r["v"], v)


def test_main_sequence_walks_408_384_408_and_each_case_is_what_its_name_says(emu):
    ofs, hs, recs = _records(emu)["main"]
    rec = _named(emu)
    want = {h[0]: w for h, w in zip(hs, Z.text_by_frame(hs, Z.RAW, ofs))}
    got = {h[0]: g for h, g in zip(hs, Z.text_by_record(hs, recs, Z.RAW, ofs))}
    ok = lambda n: "[OK]" in want[n][0]                                          # noqa: E731
    v = lambda n: rec[n]["v"]                                                    # noqa: E731
    # a clean ECEF hit at 408 bits
    assert got["ecef_clean"][2] == 408 and v("ecef_clean")[:3] == [1, 0, 45] and ok("ecef_clean") and want["ecef_clean"][1] == 386
    # one flipped payload bit: [NO] under both lengths
    assert v("ecef_payload_flip")[:2] == [0, 0] and not ok("ecef_payload_flip")
    # -0.0 and +0.0 on a 1 bit are both a 0: the frame changes and fails; with the sign bit as the rule -0.0 would have passed
    for n in ("ecef_neg_zero", "ecef_pos_zero"):
        s = next(h[1] for h in hs if h[0] == n)
        z = np.flatnonzero(s == 0)
        assert len(z) == 1 and np.signbit(s[z[0]]) == (n == "ecef_neg_zero")
        assert not (rec[n]["data"][(22 + z[0]) >> 3] >> (7 - ((22 + z[0]) & 7))) & 1 and v(n)[:2] == [0, 0] and not ok(n)
    assert rec["ecef_neg_zero"]["data"] == rec["ecef_pos_zero"]["data"]
    assert v("ecef_zero_on_a_zero")[:2] == [1, 0] and ok("ecef_zero_on_a_zero")
    # bytes 30 / 31 one bit away from FF FF, and on it: crclen changes
    assert v("ecef_ff_fe")[:3] == [1, 0, 45] and ok("ecef_ff_fe") and v("ecef_into_ffff")[:3] == [0, 0, 42] and not ok("ecef_into_ffff")
    # a clean lat / lon hit while at 408 bits, 24 random values behind it: [OK], the decoder moves to 384
    assert got["latlon_at_408"][2] == 408 and v("latlon_at_408")[:3] == [1, 1, 42] and ok("latlon_at_408") and want["latlon_at_408"][1] == 362
    # the second one is read at 362 bits: v[1]
    assert got["latlon_at_384"][2] == 384 and v("latlon_at_384")[:3] == [1, 1, 42] and ok("latlon_at_384")
    # an ECEF hit while the decoder is at 384 bits: good at 408, not at 384, and the text is the host tier's [NO]
    assert got["ecef_at_384"][2] == 384 and v("ecef_at_384")[:3] == [1, 0, 45] and not ok("ecef_at_384") and got["ecef_at_384"][0] == want["ecef_at_384"][0]
    assert want["ecef_at_384"][1] == 362
    assert v("latlon_payload_flip")[:3] == [0, 0, 42] and v("latlon_out_of_ffff")[:3] == [0, 0, 45]
    # the hits of the end of input: not decoded, everything behind the head zero; the host tier reads up to 362 of their bits
    for n in Z.SHORT:
        r = rec["short_%d" % n]
        assert r["decoded"] == 0 and r["nbits"] == n and r["v"] == [0] * 6 and r["aux"] == bytes(12) and r["data"] == bytes(240)
    assert ok("short_362") and ok("short_385") and not ok("short_361")
    # a frame that passes as ECEF at 384 bits takes the decoder back to 408
    assert got["crafted_back_to_408"][2] == 384 and v("crafted_back_to_408")[:3] == [1, 1, 45] and want["crafted_back_to_408"][1] == 386
    assert got["ecef_at_408_again"][2] == 408 and ok("ecef_at_408_again")
    # the 24 values behind a lat / lon frame do not enter the verdict at 384 bits, and do enter the record's bits
    a = next(h[1] for h in hs if h[0] == "latlon_at_384")
    b = a.copy(); b[362:] = -b[362:]
    ra, rb = Z.emu_run(emu, 8, [a, b])[0]
    assert ra["v"][1] == rb["v"][1] == 1 and Z.split16(ra["v"][3])[1] == Z.split16(rb["v"][3])[1] and ra["data"][:48] == rb["data"][:48] and ra["data"][48:51] != rb["data"][48:51]


def test_other_offsets_pass_where_the_frame_was_placed_for_them(emu):
    r0, r16 = _named(emu, "ofs0"), _named(emu, "ofs16")
    assert [r0[n]["v"][:3] for n in ("ecef", "latlon", "latlon_at_384", "ecef_at_384")] == [[1, 0, 45], [1, 1, 42], [1, 1, 42], [1, 0, 45]]
    assert r0["natural_ecef"]["v"][:2] == [0, 0] and r0["flip"]["v"][:2] == [0, 0]
    assert r16["latlon"]["v"][:3] == [1, 0, 42] and r16["ecef"]["v"][:2] == [0, 0] and r16["short"]["decoded"] == 0
    assert all(r["v"][5] == 0 for r in r0.values() if r["decoded"]) and all(r["v"][5] == 16 for r in r16.values() if r["decoded"])


def test_a_record_made_under_another_offset_is_refused(emu):
    rec = _named(emu)["ecef_clean"]
    for kw in (dict(bits_ofs=0, bits_ofs_given=1), dict(bits_ofs=16, bits_ofs_given=1)):
        d = FamilyDecoder("MRZ", **Z.RAW, **kw)
        with pytest.raises(SondeError):
            d.decoded(rec)
        d.close()
    d = FamilyDecoder("MRZ", **Z.RAW, bits_ofs=16)                              # (not given: the default 8 holds, as in sonde_mrz_dec_create)
    assert "[OK]" in d.decoded(rec)
    d.close()
    assert "MRZ" not in DEVICE_KINDS and DEVICE_KINDS_ALL == dict(DEVICE_KINDS, MRZ=31)


# ---------------------------------------------------------------- 3. the launch: grid sizes, the ring
def test_records_do_not_depend_on_the_grid_and_the_ring_wraps(emu):
    hs = Z.all_hits()[4:14]                                                      # ten hits, among them lat / lon ones, noise and NaNs
    softs, mvs = [h[1] for h in hs], [h[2] for h in hs]
    one, done = Z.emu_run(emu, 8, softs, mvs, grid=1)
    assert done == (10, 0) and [r["channel"] for r in one] == list(range(10))
    for grid in (3, 10, 17):                                                     # (17: more workgroups than records)
        got, done = Z.emu_run(emu, 8, softs, mvs, grid=grid)
        assert [Z.rec_key(r) for r in got] == [Z.rec_key(r) for r in one] and done == (10, 0), grid
    body = lambda r: Z.rec_key(r)[1:]                                            # noqa: E731  (everything but the channel, which is the ring slot here)
    # max_frames = 4, the counter at 6: records 6 .. 9 land in slots 2, 3, 0, 1
    for grid in (1, 3, 7):
        got, done = Z.emu_run(emu, 8, softs[6:], mvs[6:], grid=grid, max_frames=4, start=6)
        assert [r["channel"] for r in got] == [2, 3, 0, 1] and [body(r) for r in got] == [body(r) for r in one[6:]] and done == (10, 0), grid
    # ten hits queued into a ring of four since the last launch (done = 0): only the last four are there, and they are decoded once each
    got, done = Z.emu_run(emu, 8, softs, mvs, grid=3, max_frames=4, start=0)
    assert [body(r) for r in got] == [body(r) for r in one[6:]] and done == (10, 0)
    # a start counter close to the wrap of 32 bits
    got, done = Z.emu_run(emu, 8, softs, mvs, grid=3, max_frames=16, start=0xFFFFFFFB)
    assert [body(r) for r in got] == [body(r) for r in one] and done == (5, 0)


def test_every_byte_of_every_record_is_written(emu):
    for _, hs, recs in _records(emu).values():                                   # the output was 0xEE beforehand (emu_run)
        for h, r in zip(hs, recs):
            if r["decoded"]:
                assert r["data"][51:] == bytes(189) and r["aux"] == bytes(12), h[0]
            else:
                assert Z.rec_key(r)[6:] == ((0,) * 6, bytes(12), bytes(240)), h[0]
            assert r["channel"] >= 0 and r["kind"] == Z.KIND and r["decoded"] in (0, 1) and r["mv_pos"] == 0


def test_a_launch_with_nothing_queued_writes_nothing(emu):
    out = (FamilyHit * 2)()                                                      # counter == done: no record is the launch's
    C.memset(out, 0xEE, C.sizeof(out))
    d = (C.c_uint * 2)(5, 0)
    soft = np.zeros((2, Z.NB), np.float32); nb = np.zeros(2, np.int32)
    assert emu.emu_mrz_hits_run(8, soft.ctypes.data, Z.NB, nb.ctypes.data, None, 2, 5, 5, 3, out, d) == 0
    assert bytes(out) == b"\xEE" * C.sizeof(out) and (d[0], d[1]) == (5, 0)
    assert emu.emu_mrz_hits_run(65, soft.ctypes.data, Z.NB, nb.ctypes.data, None, 2, 5, 5, 3, out, d) == -1
    assert emu.emu_mrz_hits_bits() == Z.NB


# ---------------------------------------------------------------- 4. a stand-alone program under the sanitizers
def test_sanitized_standalone_replay_of_the_hits(emu, tmp_path):
    """the emulator translation unit under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program with its own main (tests/emu/mrz_hits_replay.cpp),
    run as a process of its own, outside the interpreter, in the environment as it is (the sanitizer runtimes are linked into the program): the same hits, the same
    lines.  The soft-bit buffer is exactly max_frames x 386 long, so a read beyond a hit is an error there."""
    exe = str(tmp_path / "mrz_hits_replay_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, Z.REPLAY_SRC, Z.EMU_SRC])

    def line(r):
        return "%d %d %d %d " % (r["channel"], r["kind"], r["nbits"], r["decoded"]) + " ".join(str(v) for v in r["v"]) + " " + r["aux"].hex() + " " + r["data"].hex()

    for name, (ofs, hs, recs) in _records(emu).items():
        soft = np.zeros((len(hs), Z.NB), np.float32)
        for i, h in enumerate(hs):
            soft[i, :len(h[1])] = h[1]
        p = tmp_path / "hits.f32"
        soft.tofile(p)
        args = [exe, str(p), str(ofs), str(Z.NB), "3", str(len(hs)), "0"]
        for h in hs:
            args += [str(len(h[1])), repr(float(h[2]))]
        r = subprocess.run(args, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert b"ERROR" not in r.stderr and b"runtime error" not in r.stderr
        assert r.stdout.decode().splitlines() == [line(x) for x in recs], name
        assert b"%d records, done %d ticket 0" % (len(hs), len(hs)) in r.stderr


# ---------------------------------------------------------------- 5. the C entry points, as far as they go without a GPU
def test_direct_entry_arguments_are_checked_before_the_device_is_touched():
    import torch
    from radiosonde_auto_rx_amd.engine import lib
    L = lib()
    fn = L.sonde_mrz_decode_device
    fn.argtypes = [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
    E_ARG, E_NOGPU = -1, -2
    soft = np.zeros((2, 400), np.float32); n = np.array([386, 385], np.int32); out = (FamilyHit * 2)()
    S, N, O = soft.ctypes.data, n.ctypes.data, C.addressof(out)
    assert fn(-1, S, 400, N, 2, O) == E_ARG and fn(65, S, 400, N, 2, O) == E_ARG
    assert fn(8, S, 400, N, -1, O) == E_ARG
    assert fn(8, None, 400, N, 2, O) == E_ARG and fn(8, S, 400, None, 2, O) == E_ARG and fn(8, S, 400, N, 2, None) == E_ARG
    assert fn(8, S, 385, N, 2, O) == E_ARG                                       # a stride shorter than a hit
    neg = np.array([386, -1], np.int32); over = np.array([386, 401], np.int32)
    assert fn(8, S, 400, neg.ctypes.data, 2, O) == E_ARG and fn(8, S, 400, over.ctypes.data, 2, O) == E_ARG
    assert fn(8, S, 400, N, 0, O) == 0 and fn(0, S, 400, N, 0, O) == 0 and fn(64, S, 400, N, 0, O) == 0      # nothing to do
    L.sonde_engine_set_family_mrz.argtypes = [C.c_void_p, C.c_int32]
    assert L.sonde_engine_set_family_mrz(None, 8) == E_ARG and L.sonde_engine_set_family(None, 31, 1) == E_ARG
    if not torch.cuda.is_available():
        assert fn(8, S, 400, N, 2, O) == E_NOGPU
