"""Scratch, spill and LDS figures of k_lms6_rs, read from the compiler's own report of sonde_lms6_rs.hip (the csrc Makefile keeps it beside the objects:
-Rpass-analysis=kernel-resource-usage).  The wave functions use no indexed local arrays, so nothing goes to scratch memory, and the kernel's static LDS is
Lms6RsLds and nothing else: tables, codeword, Lambda / Omega scratch and the staged block bytes, at most 4096 B, so that 32 one-wave workgroups
fit a CU's 160 KB and LDS never bounds residency.  No GPU is needed."""
import os

import pytest

from test_kernel_resources import parse_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc", "obj")
REPORT = os.path.join(OBJ, "sonde_lms6_rs.resources.txt")


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(REPORT):
        from radiosonde_auto_rx_amd import engine
        engine.build_library()
    assert os.path.exists(REPORT), "the build leaves the compiler's resource report at " + REPORT
    return parse_report(open(REPORT).read())


def test_k_lms6_rs_has_no_scratch_no_spills_and_a_small_lds(report):
    import lms6_rs_cases as R
    assert list(report) == ["k_lms6_rs"]
    k = report["k_lms6_rs"]
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0
    assert k["vgprs"] <= 128
    assert k["lds"] == R.load_emu().emu_lms6_rs_lds_bytes() <= 4096
    assert 32 * k["lds"] <= 160 * 1024
