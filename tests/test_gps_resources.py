"""Scratch, spill and LDS figures of k_gps_subsets, read from the compiler's own report of sonde_gps.hip (the csrc Makefile keeps it beside the objects:
-Rpass-analysis=kernel-resource-usage).  The cofactor code takes its index sets as template arguments and the transcendental code exists once, its inputs chosen by
selects, so that nothing goes to scratch memory; the static LDS is one job and nothing else (which also records the register count).
No GPU is needed."""
import ctypes as C
import os

import pytest

from test_kernel_resources import parse_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc", "obj", "sonde_gps.resources.txt")


@pytest.fixture(scope="module")
def kernel():
    if not os.path.exists(REPORT):
        from radiosonde_auto_rx_amd import engine
        engine.build_library()
    assert os.path.exists(REPORT), "the build leaves the compiler's resource report at " + REPORT
    rep = parse_report(open(REPORT).read())
    assert list(rep) == ["k_gps_subsets"], list(rep)
    return rep["k_gps_subsets"]


def test_no_scratch_and_no_vector_spills(kernel):
    assert kernel["scratch"] == 0 and kernel["vgpr_spill"] == 0, kernel


def test_static_lds_is_one_job(kernel):
    from radiosonde_auto_rx_amd import gps
    assert kernel["lds"] == C.sizeof(gps.GpsJob) == 680
