"""Scratch, spill and LDS figures of k_mrz_hits, read from the compiler's own report of sonde_mrz_hits.hip (the csrc Makefile keeps it beside the objects:
-Rpass-analysis=kernel-resource-usage).  The wave functions use no indexed local arrays, so nothing goes to scratch memory, and the kernel's static LDS is the LDS
struct of the MRZ soft-bit consumer and nothing else — less than k_softin_mrz's, which stages its half symbols besides.  No GPU is needed."""
import os

import pytest

from test_kernel_resources import parse_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc", "obj")
REPORT = os.path.join(OBJ, "sonde_mrz_hits.resources.txt")
REPORT_SOFTIN = os.path.join(OBJ, "sonde_softin_dev.resources.txt")


@pytest.fixture(scope="module")
def reports():
    if not os.path.exists(REPORT) or not os.path.exists(REPORT_SOFTIN):
        from radiosonde_auto_rx_amd import engine
        engine.build_library()
    assert os.path.exists(REPORT), "the build leaves the compiler's resource report at " + REPORT
    return parse_report(open(REPORT).read()), parse_report(open(REPORT_SOFTIN).read())


def test_k_mrz_hits_has_no_scratch_no_spills_and_the_consumers_struct_as_lds(reports):
    import mrz_hits_cases as Z
    report, softin = reports
    assert list(report) == ["k_mrz_hits"]
    k = report["k_mrz_hits"]
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0
    assert k["vgprs"] <= 128                               # one wave a workgroup: four waves a SIMD at the least
    assert k["lds"] == Z.load_emu().emu_mrz_hits_lds_bytes() == 284
    assert "k_softin_mrz" in softin and k["lds"] <= softin["k_softin_mrz"]["lds"]
