"""Scratch, spill and LDS figures of k_m20_hits, read from the compiler's own report of sonde_m20_hits.hip (the csrc Makefile keeps it beside the objects:
-Rpass-analysis=kernel-resource-usage).  The wave functions use no indexed local arrays, so nothing goes to scratch memory, and the kernel's static LDS is the
172 frame bytes of a record and nothing else.  No GPU is needed."""
import os

import pytest

from test_kernel_resources import parse_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc", "obj", "sonde_m20_hits.resources.txt")


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(REPORT):
        from radiosonde_auto_rx_amd import engine
        engine.build_library()
    assert os.path.exists(REPORT), "the build leaves the compiler's resource report at " + REPORT
    return parse_report(open(REPORT).read())


def test_k_m20_hits_has_no_scratch_no_spills_and_the_frame_bytes_as_lds(report):
    import m20_hits_cases as M
    assert list(report) == ["k_m20_hits"]
    k = report["k_m20_hits"]
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0
    assert k["vgprs"] <= 64                                # one wave a workgroup: registers never bound the occupancy below eight waves a SIMD
    assert k["lds"] == 172 == M.load_emu().emu_m20_hits_lds_bytes()
