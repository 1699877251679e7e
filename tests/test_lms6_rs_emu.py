"""The DEVICE RS(255,223) decoder of LMS6 / LMS-X blocks (radiosonde_auto_rx_amd/csrc/sonde_rs223_dev.h: one wavefront per codeword, a coefficient per lane; per
block record the decoder under each hypothesis the host decoder can ask for) executed on the CPU under tests/emu/wave_emu.h and compared, bit for bit, with the
reference's bch_ecc_mod.c compiled where it lies (oracle/_ref/libref_ecc.so).  The same source is compiled by hipcc into k_lms6_rs; tests/test_gpu_lms6_rs.py
runs it there."""
import ctypes as C

import pytest

import lms6_rs_cases as R
from radiosonde_auto_rx_amd.family import Lms6Rs

pytestmark = pytest.mark.skipif(not R.have_ref(), reason="compiled reference not present")


@pytest.fixture(scope="module")
def emu():
    return R.load_emu()


def test_record_layout(emu):
    assert C.sizeof(Lms6Rs) == 120 == emu.emu_lms6_rs_record_bytes()
    assert emu.emu_lms6_rs_lds_bytes() <= 4096


def test_wave_decoder_matches_reference_word_by_word(emu):
    words = R.word_cases()
    assert 250 <= len(words) <= 350
    seen = {}
    for name, w, nerr in words:
        r_ref, w_ref, p_ref, v_ref = R.ref_decode(w)
        r_dev, w_dev, p_dev, v_dev = R.emu_decode(emu, w)
        assert r_dev == r_ref, (name, r_dev, r_ref)
        assert (w_dev == w_ref).all(), name                          # repaired into the same bytes, or untouched
        assert (p_dev == p_ref).all() and (v_dev == v_ref).all(), (name, p_dev, p_ref, v_dev, v_ref)      # in the reference's order, zero behind the count
        if nerr <= R.T:
            assert r_dev == nerr, (name, r_dev)
        else:
            seen[r_dev if r_dev < 0 else "miscorrected"] = seen.get(r_dev if r_dev < 0 else "miscorrected", 0) + 1
    assert {-1, -2, -3, "miscorrected"} <= set(seen), seen


@pytest.mark.parametrize("n", [1, 3, 65, None])
def test_record_function_matches_model(emu, n):
    """`n` block cases (None: all) through an emulated launch of two workgroups: the stride, the tail, the input left alone, nothing written behind the records"""
    cases = R.block_cases()[:n]
    got, tail = R.emu_records(emu, [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases], grid=2, extra=2)
    assert tail == b"\xEE" * len(tail) and len(tail) == 240
    for (name, b, blen, dec), g in zip(cases, got):
        assert R.rs_bytes(g) == R.rs_bytes(R.model_record(b, blen, dec)), name


def test_word_cases_as_blocks_match_model(emu):
    """every word case embedded at offset 5 of a block, as the GPU test runs them: h6 is the word's own result"""
    words = R.word_cases()
    blocks = [R.word_block(w) for _, w, _ in words]
    got, _ = R.emu_records(emu, [b for b, _ in blocks], [l for _, l in blocks], grid=3)
    for (name, w, _), (b, blen), g in zip(words, blocks, got):
        assert R.rs_bytes(g) == R.rs_bytes(R.model_record(b, blen)), name
        assert g.h6.at == 5 and g.h6.err == R.ref_decode(w)[0], name
