"""Scratch, spill and LDS figures of k_lms6_hits, read from the compiler's own report of sonde_lms6_hits.hip (the csrc Makefile keeps it beside the objects:
-Rpass-analysis=kernel-resource-usage).  The wave functions use no indexed local arrays, so nothing goes to scratch memory, and the kernel's static LDS is the LDS
struct of the LMS6 soft-bit consumer and nothing else: 38 656 B, four one-wave workgroups in a CU's 160 KB.  No GPU is needed."""
import os

import pytest

from test_kernel_resources import parse_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc", "obj")
REPORT = os.path.join(OBJ, "sonde_lms6_hits.resources.txt")


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(REPORT):
        from radiosonde_auto_rx_amd import engine
        engine.build_library()
    assert os.path.exists(REPORT), "the build leaves the compiler's resource report at " + REPORT
    return parse_report(open(REPORT).read())


def test_k_lms6_hits_has_no_scratch_no_spills_and_the_consumers_struct_as_lds(report):
    import lms6_hits_cases as Z
    assert list(report) == ["k_lms6_hits"]
    k = report["k_lms6_hits"]
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0
    assert k["vgprs"] <= 128                               # one wave a workgroup: four waves a SIMD at the least
    assert k["lds"] == Z.load_emu().emu_lms6_hits_lds_bytes() <= 40960
    assert 4 * k["lds"] <= 160 * 1024                      # four workgroups in a CU's LDS
