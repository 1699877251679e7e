"""The device front end of the FM slicers (csrc/sonde_fm_front_dev.h, k_fm_front) under the CPU wave emulator (tests/emu/fm_front_emu.cpp): no GPU.

Input: the first half second of a 50 kHz float32 dropsonde capture with a DC offset (tests/dropf32_cases.py, 50k_dc94), so the IQ-dc blocks of 1/32, 1/16,
1/8 and 1/4 s all end inside it, at --iq 0.013 and --iq -0.021, in calls of 3 001, 7 and 12 345 samples.  The int16 FM stream is compared with
`iq_dec --FM --lpFM --wav --bo 16 --iq <fq> - 50000 32` on the same bytes — the recorded output (tests/golden/dropf32_emu.npz) and, where the compiled
reference build() made, a run of it — under the rule tests/test_gpu_iqdec.py applies to iq_dec's integer output: no sample more than 1 LSB off and fewer than
1 % of them off at all (the conversion truncates, so float noise next to an integer moves one LSB).  One call and the cut calls give the same bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import dropf32_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_SRC = os.path.join(EMU_DIR, "fm_front_emu.cpp")
EMU_SO = os.path.join(EMU_DIR, "libfm_front_emu.so")
DEPS = [EMU_SRC, os.path.join(EMU_DIR, "wave_emu.h")] + [os.path.join(CSRC, f) for f in ("sonde_fm_front_dev.h", "sonde_rs_dev.h", "sonde_design.cpp", "sonde_host.h")]
IQ_DEC = os.path.join(ROOT, "oracle", "_ref", "iq_dec")
SR = 50000
CUTS = [3001, 7, 12345]


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in DEPS):
        tmp = EMU_SO + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", tmp, EMU_SRC])
        os.replace(tmp, EMU_SO)
    L = C.CDLL(EMU_SO)
    L.emu_fm_front_run.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_double, C.c_int, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def capture():
    x = cases.samples(cases.CASES[cases.EMU_CASE]["gen"])[:2 * cases.EMU_N]
    assert len(x) == 2 * cases.EMU_N and abs(float(x[0::2].mean()) - 0.05) < 0.01          # the DC offset is there
    x.setflags(write=False)
    return x


_runs = {}


def _run(emu, x, fq, calls):
    key = (fq, tuple(calls))
    if key not in _runs:
        out = np.zeros(len(x) // 2, np.int16)
        c = (C.c_int * len(calls))(*calls)
        taps = emu.emu_fm_front_run(x.ctypes.data, len(x) // 2, c, len(calls), fq, SR, out.ctypes.data)
        assert taps == 101, taps                                                             # iq_dec.c: 4 * 50000 / 2000, made odd
        out.setflags(write=False)
        _runs[key] = out
    return _runs[key]


def _close(got, ref):
    d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    off = float(np.mean(d != 0))
    print("max |diff| %d LSB, %.4f %% of %d samples differ" % (d.max(), 100 * off, len(d)))
    assert d.max() <= 1 and off < 0.01, (int(d.max()), off)


@pytest.mark.parametrize("fq", cases.EMU_FQ)
def test_cut_calls_equal_the_recorded_iq_dec_stream(emu, capture, fq):
    ref = cases.load_emu()[fq]
    assert len(ref) == cases.EMU_N and np.abs(ref.astype(np.int32)).max() > 3000           # a signal, not silence
    _close(_run(emu, capture, fq, CUTS), ref)


@pytest.mark.parametrize("fq", cases.EMU_FQ)
def test_one_call_and_cut_calls_are_bit_identical(emu, capture, fq):
    one = _run(emu, capture, fq, [cases.EMU_N])
    assert np.array_equal(one, _run(emu, capture, fq, CUTS))
    assert np.array_equal(one, _run(emu, capture, fq, [64, 1, 1562, 63]))                   # cuts at and beside an IQ-dc block end (1562), calls below the tap count


@pytest.mark.parametrize("fq", cases.EMU_FQ)
def test_cut_calls_equal_the_compiled_iq_dec(emu, capture, fq):
    if not os.path.exists(IQ_DEC):
        pytest.fail("oracle/_ref/iq_dec missing: run __graft_entry__.build() where the reference lies")
    r = subprocess.run([IQ_DEC] + cases.iq_dec_args(SR, fq), input=capture.astype("<f4").tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-300:]
    ref = np.frombuffer(r.stdout[44:], "<i2")
    assert len(ref) == cases.EMU_N
    _close(_run(emu, capture, fq, CUTS), ref)


def test_the_iq_dc_blocks_end_inside_the_capture():
    """sr / 32 samples, doubled: 1562, + 3124, + 6248, + 12496 = 23430 < 25000"""
    n, ends = SR // 32, []
    while sum(ends) + n <= cases.EMU_N:
        ends.append(n)
        n *= 2
    assert len(ends) == 4 and sum(ends) == 23430
