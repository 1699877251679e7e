"""Register, scratch and LDS figures of k_softin_wxr, read from the compiler's own report of sonde_softin_dev.hip (the csrc Makefile keeps it beside the objects:
-Rpass-analysis=kernel-resource-usage), the way tests/test_softin_mrz_mts01_resources.py reads it.  The wave function is written without indexed local arrays —
the PN9 sequence is a 64-byte constant, the check two reductions over the wave — so that nothing goes to scratch memory; the soft decisions are read once, so the
wave's LDS is its bit words and the two byte rows alone.  No GPU is needed."""
import os

import pytest

from test_kernel_resources import parse_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc", "obj", "sonde_softin_dev.resources.txt")
LDS = 216                                                    # SoftinWxrLds: bit words 72 + bytes before PN9 72 + bytes behind PN9 72


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(REPORT):
        from radiosonde_auto_rx_amd import engine
        engine.build_library()
    assert os.path.exists(REPORT), "the build leaves the compiler's resource report at " + REPORT
    return parse_report(open(REPORT).read())


def test_no_scratch_and_no_vector_spills(report):
    k = report["k_softin_wxr"]
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0
    assert k["vgprs"] <= 128                               # a wave per channel, one wave a workgroup: registers never bound the occupancy


def test_lds_is_the_waves_struct(report):
    assert report["k_softin_wxr"]["lds"] == LDS


def test_the_dropsonde_consumer_keeps_its_figures(report):
    k = report["k_softin_drop"]
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["lds"] == 2528
