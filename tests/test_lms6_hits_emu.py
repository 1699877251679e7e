"""The per-hit DEVICE decoder of generic engines carrying LMS6 / LMS-X (radiosonde_auto_rx_amd/csrc/sonde_lms6_hits_dev.h: the raw-bit sign alternation, then the
soft-bit consumer's wave Viterbi, deconv and bits2bytes, one wavefront per hit record) executed on the CPU under tests/emu/wave_emu.h and launched as k_lms6_hits is
(tests/emu/lms6_hits_emu.cpp).  Two arbiters, both pinned to the compiled reference elsewhere (tests/test_softin_lms6_emu.py, tests/test_lms6_native.py): the numpy
model tests/lms6_vit_model.py for the records, and the host tier sonde_lms6_dec_block on the same soft bits for the text — sequences of hits go through one
decoder with .hit and through another with .decoded on the emulator's records, and after every block the characters and the decoder's type are equal.  The same
source is compiled by hipcc into k_lms6_hits; tests/test_gpu_lms6_hits.py runs it there on the same hits.  Argument checks of the C entry points that need no GPU
are at the end.  Every comparison is for equality.

The issue behind this decoder expected a block of noise to make deconv stop early (err != 0, a short blen).  A hit cannot do that: its first 80 positions are the
sync values +-1 themselves, the first eight trellis steps of the zero path cost nothing there, and what follows step 12 depends on the state at step 12 alone — so
the survivor's first six input bits are zero whatever the 4096 values behind the header are, and deconv's register starts as the encoder's did.  The noise block is
in the list and equals the model, with err = 0; lms6_wave_decode's early stop is covered where a caller's own first positions reach it
(tests/test_softin_lms6_emu.py)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import lms6_hits_cases as Z
from radiosonde_auto_rx_amd.engine import SondeError
from radiosonde_auto_rx_amd.family import DEVICE_KINDS, DEVICE_KINDS_ALL, DEVICE_KINDS_LMS, FamilyDecoder, Lms6Hit


@pytest.fixture(scope="module")
def emu():
    return Z.load_emu()


# ---------------------------------------------------------------- 1. records against the model
@pytest.mark.parametrize("lmsx", [False, True], ids=["lms6", "lmsx"])
@pytest.mark.parametrize("vit", [1, 2])
def test_every_record_is_the_model_of_its_soft_bits(emu, lmsx, vit):
    hs, recs = Z.hits(lmsx), Z.records(emu, lmsx, vit)
    nb = Z.NBX if lmsx else Z.NB6
    assert len(recs) == len(hs)
    for i, ((name, s, mv), r) in enumerate(zip(hs, recs)):
        assert r["kind"] == Z.KIND and r["nbits"] == len(s) and r["decoded"] == int(len(s) == nb) and r["channel"] == i, name
        assert r["mv_pos"] == 0 and np.float32(r["mv"]).tobytes() == np.float32(mv).tobytes(), name
        if len(s) < nb:                                                          # the hit of the end of input: marked, everything else zero
            assert (r["len"], r["blen"], r["err"], r["vit"], r["bytes"]) == (0, 0, 0, 0, bytes(Z.BB_LEN)), name
            continue
        by, blen, err, ln = Z.model(s, mv, vit)
        print(name, "vit", vit, "blen", blen, "err", err)
        assert (r["bytes"], r["blen"], r["err"], r["len"], r["vit"]) == (by, blen, err, ln, vit), name
        assert r["len"] == 80 + nb and r["bytes"][r["blen"]:] == bytes(Z.BB_LEN - r["blen"])


def test_each_case_is_what_its_name_says(emu):
    for lmsx in (False, True):
        sync = bytes([0x00, 0x58, 0xF3, 0x3F, 0xB8])
        for vit in (1, 2):
            rec = {h[0]: r for h, r in zip(Z.hits(lmsx), Z.records(emu, lmsx, vit))}
            hit = {h[0]: h for h in Z.hits(lmsx)}
            assert rec["clean"]["bytes"][:5] == sync and rec["clean"]["err"] == 0 and rec["clean"]["blen"] == (300 if lmsx else 261)
            # received inverted: negated and the phase shifted, the same block
            assert rec["clean_inverted"]["bytes"] == rec["clean"]["bytes"] and rec["sigma09_inverted"]["bytes"] == rec["sigma09"]["bytes"]
            # a sign that does not belong to the values, and no sign at all: another block
            assert rec["sigma07_wrong_sign"]["bytes"] != rec["sigma07"]["bytes"] and rec["mv_zero"]["bytes"][:5] != sync
            # -0.0 is a 1 under >= 0 and stays -0.0 under a negation that is one: with --vit the hard bits are those of +0.0 once the score's flip made it +0.0
            z, nz, nzi = rec["all_zero"], rec["all_neg_zero"], rec["all_neg_zero_inverted"]
            assert np.signbit(hit["all_neg_zero"][1]).all() and not np.signbit(hit["all_zero"][1]).any()
            assert z["err"] == nz["err"] == nzi["err"] == 0
            if vit == 1:
                assert z["bytes"] == nz["bytes"]                                 # (s >= 0 holds for both zeros)
        # the model's tie count: the all-zero block is one of ties at every step beyond the sync positions
        _, _, _, ties = Z.V.decode_block(Z.V.block_sb(hit["all_zero"][1], 0.9, 2), with_ties=True)
        assert ties > 2000
        e = hit["erased"][1]
        assert 0.12 < float(np.mean(e == 0)) < 0.18


# ---------------------------------------------------------------- 2. record -> text against the arbiter, block by block
_seq_recs = {}
CASES = [("lms6", 6), ("lmsx", 10), ("lms6", 0), ("lmsx", 0), ("switch", 0)]


@pytest.mark.parametrize("kind,typ", CASES, ids=["lms6--lms6", "lmsx--lmsX", "lms6-auto", "lmsx-auto", "switch-auto"])
@pytest.mark.parametrize("oname", ["raw", "json"])
def test_text_and_type_after_every_block_equal_the_host_tier(emu, kind, typ, oname):
    opts, vit = Z.OPT_VIT[oname]
    seq = Z.sequence(kind)
    if (kind, vit) not in _seq_recs:                                             # (a sequence goes through more than one decoder type)
        _seq_recs[(kind, vit)] = Z.seq_records(emu, seq, vit)
    recs = _seq_recs[(kind, vit)]
    assert all(r["decoded"] == 1 and r["vit"] == vit and r["nbits"] == len(h[1]) for h, r in zip(seq, recs))
    want = Z.text_by_hit(seq, opts, typ)
    got = Z.text_by_record(seq, recs, opts, typ)
    for h, w, g in zip(seq, want, got):
        assert g[0] == w[0] and g[1] == w[1], (h[0], w, g)
    # the comparison is not one of empty strings
    text = "".join(w[0] for w in want)
    assert text.count("[OK]") >= 4, text[-400:]
    if oname == "json":
        assert len(FamilyDecoder.json_objects(text)) >= 1
    took_soft = {h[0] for h, g in zip(seq, got) if g[2]}
    if kind == "switch":
        # the length rule in both directions: the device's 4096-bit records feed a decoder that reads 4720, a 4720-bit record goes to an LMS6 decoder as soft bits
        assert took_soft == {"lms6_on_x_engine_after"}
        types = [w[1] for w in want]
        assert [t[0] for t in types] == ["LMS6", "LMS6", "LMSX", "LMSX", "LMSX", "LMSX", "LMS6", "LMS6", "LMS6", "LMS6"]
        assert [t[1] for t in types] == [False, False, True, False, False, False, True, False, False, False]
        assert "[OK]" in want[3][0] and "[OK]" in want[7][0]
    elif (kind, typ) == ("lmsx", 0):
        assert took_soft == {"lmsx_0"}                                           # an auto decoder starts as LMS6: the first LMS-X block of an LMS-X engine is too long for it
    else:
        assert not took_soft


def test_a_record_of_another_vit_or_for_ecc3_is_refused_and_a_long_one_needs_its_soft_bits(emu):
    rec = dict(Z.records(emu, False, 2)[0], mv_pos=1000)
    for kw in (dict(vit=1, json=0), dict(vit=0, json=0), dict(vit=2, ecc=3, json=0)):
        d = FamilyDecoder("LMS6", **dict(Z.RAW, **kw))
        with pytest.raises(SondeError):
            d.decoded(rec)
        d.close()
    d = FamilyDecoder("LMS6", **dict(Z.RAW, vit=0, json=1))                      # --json implies --vit: a record of vit = 1 is this decoder's
    assert "[OK]" in d.decoded(dict(Z.records(emu, False, 1)[0], mv_pos=1000))
    d.close()
    d = FamilyDecoder("LMS6", **Z.JSON)
    assert "[OK]" in d.decoded(rec)
    long_rec = dict(Z.records(emu, True, 2)[0], mv_pos=50000)                    # 4720 bits for a decoder that reads 4096
    with pytest.raises(SondeError):
        d.decoded(long_rec)
    d.close()
    assert DEVICE_KINDS_LMS == {"LMS6": 6, "LMSX": 6} and not set(DEVICE_KINDS_LMS) & set(DEVICE_KINDS_ALL) and DEVICE_KINDS_ALL == dict(DEVICE_KINDS, MRZ=31)


# ---------------------------------------------------------------- 3. the launch: grid sizes, the ring
def test_records_do_not_depend_on_the_grid_and_the_ring_wraps(emu):
    hs = Z.hits(False)[5:11]                                                     # six hits, among them zeros and a wrong sign
    softs, mvs = [h[1] for h in hs], [h[2] for h in hs]
    one, done = Z.emu_run(emu, 2, Z.NB6, softs, mvs, grid=1)
    assert done == (6, 0) and [r["channel"] for r in one] == list(range(6))
    assert [Z.rec_key(r)[2:] for r in one] == [Z.rec_key(r)[2:] for r in Z.records(emu, False, 2)[5:11]]
    for grid in (3, 9):                                                          # (9: more workgroups than records)
        got, done = Z.emu_run(emu, 2, Z.NB6, softs, mvs, grid=grid)
        assert [Z.rec_key(r) for r in got] == [Z.rec_key(r) for r in one] and done == (6, 0), grid
    body = lambda r: Z.rec_key(r)[1:]                                            # noqa: E731  (everything but the channel, which is the ring slot here)
    # six hits queued into a ring of four since the last launch (done = 0): only the last four are there, in slots 2, 3, 0, 1, decoded once each
    got, done = Z.emu_run(emu, 2, Z.NB6, softs, mvs, grid=3, max_frames=4, start=0)
    assert [r["channel"] for r in got] == [2, 3, 0, 1] and [body(r) for r in got] == [body(r) for r in one[2:]] and done == (6, 0)
    # a start counter close to the wrap of 32 bits
    got, done = Z.emu_run(emu, 2, Z.NB6, softs, mvs, grid=3, max_frames=8, start=0xFFFFFFFD)
    assert [body(r) for r in got] == [body(r) for r in one] and done == (3, 0)
    # two records into a ring of four: the other two slots keep the caller's fill
    nb = Z.NB6
    soft = np.zeros((4, nb), np.float32); soft[1] = softs[0]; soft[2] = softs[1]
    nbits = np.array([0, nb, nb, 0], np.int32); mv = np.array([0, mvs[0], mvs[1], 0], np.float32)
    out = (Lms6Hit * 4)()
    C.memset(out, 0x5A, C.sizeof(out))
    d = (C.c_uint * 2)(1, 0)
    assert emu.emu_lms6_hits_run(2, nb, soft.ctypes.data, nb, nbits.ctypes.data, mv.ctypes.data, 4, 1, 3, 2, out, d) == 0
    sz = C.sizeof(Lms6Hit)
    assert sz == emu.emu_lms6_hits_record_bytes() == 348
    raw = bytes(out)
    assert raw[:sz] == b"\x5A" * sz and raw[3 * sz:] == b"\x5A" * sz and (d[0], d[1]) == (3, 0)
    assert [body(Z.lms6_hit_dict(out[k])) for k in (1, 2)] == [body(r) for r in one[:2]]


def test_a_launch_with_nothing_queued_writes_nothing_and_bad_arguments_are_refused(emu):
    out = (Lms6Hit * 2)()                                                        # counter == done: no record is the launch's
    C.memset(out, 0xEE, C.sizeof(out))
    d = (C.c_uint * 2)(5, 0)
    soft = np.zeros((2, Z.NB6), np.float32); nb = np.zeros(2, np.int32); mv = np.zeros(2, np.float32)
    run = lambda vit, n: emu.emu_lms6_hits_run(vit, n, soft.ctypes.data, n, nb.ctypes.data, mv.ctypes.data, 2, 5, 5, 3, out, d)      # noqa: E731
    assert run(2, Z.NB6) == 0
    assert bytes(out) == b"\xEE" * C.sizeof(out) and (d[0], d[1]) == (5, 0)
    assert run(0, Z.NB6) == -1 and run(3, Z.NB6) == -1 and run(2, 4000) == -1


# ---------------------------------------------------------------- 4. a stand-alone program under the sanitizers
def test_sanitized_standalone_replay_of_the_hits(emu, tmp_path):
    """the emulator translation unit under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program with its own main (tests/emu/lms6_hits_replay.cpp),
    run as a process of its own, outside the interpreter, in the environment as it is (the sanitizer runtimes are linked into the program): the same hits, the same
    lines.  The soft-bit buffer is exactly max_frames x nb long, so a read beyond a hit is an error there."""
    exe = str(tmp_path / "lms6_hits_replay_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, Z.REPLAY_SRC, Z.EMU_SRC])

    def line(r):
        return "%d %d %d %d %d %d %d %d " % (r["channel"], r["kind"], r["nbits"], r["decoded"], r["len"], r["blen"], r["err"], r["vit"]) + r["bytes"].hex()

    for lmsx, vit in ((False, 2), (True, 1)):
        hs, recs = Z.hits(lmsx), Z.records(emu, lmsx, vit)
        nb = Z.NBX if lmsx else Z.NB6
        soft = np.zeros((len(hs), nb), np.float32)
        for i, h in enumerate(hs):
            soft[i, :len(h[1])] = h[1]
        p = tmp_path / "hits.f32"
        soft.tofile(p)
        args = [exe, str(p), str(vit), str(nb), "3", str(len(hs)), "0"]
        for h in hs:
            args += [str(len(h[1])), repr(float(h[2]))]
        r = subprocess.run(args, capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert b"ERROR" not in r.stderr and b"runtime error" not in r.stderr
        assert r.stdout.decode().splitlines() == [line(x) for x in recs], (lmsx, vit)
        assert b"%d records, done %d ticket 0" % (len(hs), len(hs)) in r.stderr


# ---------------------------------------------------------------- 5. the C entry points, as far as they go without a GPU
def test_direct_entry_arguments_are_checked_before_the_device_is_touched():
    import torch
    from radiosonde_auto_rx_amd.engine import lib
    L = lib()
    fn = L.sonde_lms6_decode_device
    fn.argtypes = [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    E_ARG, E_NOGPU = -1, -2
    soft = np.zeros((2, 4720), np.float32); n = np.array([4096, 4095], np.int32); mv = np.array([0.9, -0.9], np.float32); out = (Lms6Hit * 2)()
    S, N, M, O = soft.ctypes.data, n.ctypes.data, mv.ctypes.data, C.addressof(out)
    assert fn(0, S, 4096, N, M, 2, O) == E_ARG and fn(3, S, 4096, N, M, 2, O) == E_ARG and fn(-1, S, 4096, N, M, 2, O) == E_ARG
    assert fn(2, S, 4096, N, M, -1, O) == E_ARG
    assert fn(2, None, 4096, N, M, 2, O) == E_ARG and fn(2, S, 4096, None, M, 2, O) == E_ARG and fn(2, S, 4096, N, None, 2, O) == E_ARG
    assert fn(2, S, 4096, N, M, 2, None) == E_ARG
    for stride in (0, 4095, 4097, 4719, 4800, 386):                              # the length a complete hit has: 4096 or 4720
        assert fn(2, S, stride, N, M, 2, O) == E_ARG, stride
    neg = np.array([4096, -1], np.int32); over = np.array([4096, 4097], np.int32)
    assert fn(2, S, 4096, neg.ctypes.data, M, 2, O) == E_ARG and fn(2, S, 4096, over.ctypes.data, M, 2, O) == E_ARG
    assert fn(2, S, 4096, N, M, 0, O) == 0 and fn(1, S, 4720, N, M, 0, O) == 0                                  # nothing to do
    L.sonde_engine_set_family_lms6.argtypes = [C.c_void_p, C.c_int32]
    L.sonde_engine_fetch_family_lms6.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
    assert L.sonde_engine_set_family_lms6(None, 2) == E_ARG and L.sonde_engine_fetch_family_lms6(None, O, 2, 0) == E_ARG
    assert L.sonde_engine_set_family(None, 6, 1) == E_ARG
    fam = L.sonde_family_decode_device
    fam.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
    assert fam(6, 1, S, 4096, N, 2, O) == E_ARG and fam(6, 1, S, 4096, N, 0, O) == E_ARG                         # LMS6 is not a kind of sonde_family_hit_t
    L.sonde_lms6_dec_vit.argtypes = [C.c_void_p, C.c_void_p]
    assert L.sonde_lms6_dec_vit(None, None) == E_ARG
    if not torch.cuda.is_available():
        assert fn(2, S, 4096, N, M, 2, O) == E_NOGPU and fn(1, S, 4720, N, M, 1, O) == E_NOGPU
