"""Register, scratch and LDS figures of k_softin_meisei, read from the compiler's own report of sonde_softin_dev.hip (the csrc Makefile keeps it beside the
objects: -Rpass-analysis=kernel-resource-usage), the way tests/test_kernel_resources.py reads the report of sonde_kernels.hip.  The wave function is written
without indexed local arrays so that nothing goes to scratch memory, and a wave's LDS — the static state plus the staged half symbols of one second — must leave
eight waves on a CU.  No GPU is needed."""
import os

import pytest

from test_kernel_resources import parse_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc", "obj", "sonde_softin_dev.resources.txt")
LDS_PER_CU = 160 * 1024
SECOND = 2400                                              # half symbols a channel delivers per second, staged as float32


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(REPORT):
        from radiosonde_auto_rx_amd import engine
        engine.build_library()
    assert os.path.exists(REPORT), "the build leaves the compiler's resource report at " + REPORT
    return parse_report(open(REPORT).read())


def test_meisei_kernel_has_no_scratch_and_no_vector_spills(report):
    k = report["k_softin_meisei"]
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0
    assert k["vgprs"] <= 128                               # a wave per channel, one wave a workgroup: registers never bound the occupancy below LDS


def test_meisei_lds_with_a_second_staged_leaves_eight_waves_on_a_cu(report):
    k = report["k_softin_meisei"]
    assert k["lds"] == 272                                 # SoftinMeiseiLds: ring 192 + pending half symbol 4 + bit words 76
    assert LDS_PER_CU // (k["lds"] + 4 * SECOND) >= 8


def test_the_other_consumers_are_in_the_same_report(report):
    """the report this module reads is the softin translation unit's: the kernels DESIGN 4.7a tabulates are all there, without scratch"""
    for name in ("k_softin_m20", "k_softin_rs92", "k_softin_imet54", "k_softin_meisei"):
        assert report[name]["scratch"] == 0 and report[name]["vgpr_spill"] == 0, name
    # all nine: nothing in scratch memory, and the static LDS of a wave — each kernel's channel state, the shared helpers add none
    lds = dict(k_softin_rs41=816, k_softin_dfm=1536, k_softin_m10=1228, k_softin_m20=1628, k_softin_rs92=1648, k_softin_imet54=748, k_softin_meisei=272,
               k_softin_drop=2528, k_softin_lms6=38656)
    for name, want in lds.items():
        assert report[name]["scratch"] == 0 and report[name]["vgpr_spill"] == 0, name
        assert report[name]["lds"] == want, (name, report[name]["lds"])
