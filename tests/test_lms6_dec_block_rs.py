"""sonde_lms6_dec_block_rs (include/sonde_lms6.h): the channel's host decoder taking RS(255,223) from a device record instead of decoding.  Sequences of blocks
(tests/lms6_hits_cases.sequence: LMS6, LMS-X, and auto detection across the change in both directions) go through two decoder objects with the same history, one
through sonde_lms6_dec_block_bytes and one through sonde_lms6_dec_block_rs with records made by the model of tests/lms6_rs_cases.py (the compiled reference's
rs_decode plus frmsync_X): identical text, counts and type after every block, every RS result taken from the record.  No GPU is needed."""
import ctypes as C

import numpy as np
import pytest

import lms6_hits_cases as Z
import lms6_rs_cases as R
from radiosonde_auto_rx_amd.engine import lib
from radiosonde_auto_rx_amd.family import FamilyDecoder, Lms6Rs

pytestmark = pytest.mark.skipif(not R.have_ref(), reason="compiled reference not present")

TEXT = dict(raw=0, ecc=1, vit=1, json=0)
OPTS = {"raw": (Z.RAW, 1), "text": (TEXT, 1), "json": (Z.JSON, 2)}
RUNS = [("lms6", "raw", 6), ("lms6", "text", 0), ("lms6", "json", 0), ("lmsx", "raw", 10), ("lmsx", "text", 0), ("lmsx", "json", 10),
        ("switch", "raw", 0), ("switch", "text", 0), ("switch", "json", 0)]


@pytest.fixture(scope="module")
def hits_emu():
    return Z.load_emu()


_seq = {}


def seq_with_records(E, kind, vit):
    if (kind, vit) not in _seq:
        seq = Z.sequence(kind)
        _seq[kind, vit] = (seq, Z.seq_records(E, seq, vit))
    return _seq[kind, vit]


def counts(d):
    f, ok = C.c_int64(0), C.c_int64(0)
    fn = lib().sonde_lms6_dec_counts
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    assert fn(d._h, C.byref(f), C.byref(ok)) == 0
    return f.value, ok.value


def run_both(seq, recs, opts, typ, spoil=None):
    """-> (texts by sonde_lms6_dec_block_bytes, texts by sonde_lms6_dec_block_rs, (used, missed)); spoil(rs record) damages the record beforehand"""
    a, b = FamilyDecoder("LMS6", **Z.dec_opts(opts, typ)), FamilyDecoder("LMS6", **Z.dec_opts(opts, typ))
    ta, tb = [], []
    for (_, s, mv, pos), r in zip(seq, recs):
        r = dict(r, mv_pos=pos)
        assert a.lms_block_bits() == b.lms_block_bits()
        if not r["decoded"] or r["nbits"] > a.lms_block_bits():      # (decoded from its soft bits either way: Engine.fetch_family's need_soft)
            r["soft"] = np.asarray(s, np.float32)
        rs = R.model_record(r["bytes"], r["blen"], r["decoded"])
        if spoil:
            spoil(rs)
        ta.append((a.decoded(dict(r), Z.IF_SR), a.lms_type(), counts(a)))
        tb.append((b.decoded(dict(r), Z.IF_SR, rs=rs), b.lms_type(), counts(b)))
    st = b.lms_rs_stats()
    assert a.lms_rs_stats() == (0, 0)
    a.close(); b.close()
    return ta, tb, st


@pytest.mark.parametrize("kind,form,typ", RUNS)
def test_block_rs_prints_what_block_bytes_prints(hits_emu, kind, form, typ):
    opts, vit = OPTS[form]
    seq, recs = seq_with_records(hits_emu, kind, vit)
    ta, tb, (used, missed) = run_both(seq, recs, opts, typ)
    assert tb == ta
    assert any(t[0].strip() for t in ta), "the sequence prints nothing"
    assert missed == 0 and used > 0, (used, missed)


@pytest.mark.parametrize("kind,form,typ", [("lms6", "json", 0), ("lmsx", "json", 10), ("switch", "raw", 0)])
def test_mismatching_at_falls_back_to_the_host_decoder(hits_emu, kind, form, typ):
    opts, vit = OPTS[form]
    seq, recs = seq_with_records(hits_emu, kind, vit)

    def spoil(rs):
        rs.h6.at += 1; rs.hX.at += 1
        if rs.h6X.at >= 0:
            rs.h6X.at += 1
    ta, tb, (used, missed) = run_both(seq, recs, opts, typ, spoil)
    assert tb == ta
    assert missed > 0 and used == 0, (used, missed)


def test_null_record_and_no_ecc(hits_emu):
    """rs == NULL: every RS call is a miss, decoded here; a decoder without --ecc ignores the record"""
    seq, recs = seq_with_records(hits_emu, "lms6", 1)
    fn = lib().sonde_lms6_dec_block_rs
    fn.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_double, C.POINTER(Lms6Rs), C.c_char_p, C.c_size_t]
    for ecc in (1, 0):
        a, b = (FamilyDecoder("LMS6", **Z.dec_opts(dict(raw=1, ecc=ecc, vit=1, json=0), 6)) for _ in range(2))
        buf = C.create_string_buffer(1 << 16)
        for (_, s, mv, pos), r in zip(seq, recs):
            if not r["decoded"]:
                continue
            want = a.decoded(dict(r, mv_pos=pos), Z.IF_SR)
            rs = None if ecc else C.byref(R.model_record(r["bytes"], r["blen"], 1))
            k = fn(b._h, r["bytes"][:r["blen"]], r["blen"], r["len"], r["mv"], 4800.0, 0.0, rs, buf, len(buf))
            assert k >= 0 and buf.raw[:k].decode(errors="replace") == want
        used, missed = b.lms_rs_stats()
        assert (used, missed > 0) == ((0, True) if ecc else (0, False))
        a.close(); b.close()
