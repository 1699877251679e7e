"""Register, scratch and LDS figures of k_softin_mrz and k_softin_mts01, read from the compiler's own report of sonde_softin_dev.hip (the csrc Makefile keeps it
beside the objects: -Rpass-analysis=kernel-resource-usage), the way tests/test_softin_meisei_resources.py reads it.  Both wave functions are written without indexed
local arrays — the CRC is a lane's own shift loop and an XOR over the wave, no table — so that nothing goes to scratch memory, and a wave's LDS — the static state
plus the staged symbols of one second — must leave eight waves on a CU.  No GPU is needed."""
import os

import pytest

from test_kernel_resources import parse_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc", "obj", "sonde_softin_dev.resources.txt")
LDS_PER_CU = 160 * 1024
# kernel -> (static LDS = sizeof of the wave's LDS struct, symbols a channel delivers per second, staged as float32)
NEW = {"k_softin_mrz": (284, 2400),                         # SoftinMrzLds: ring 176 + pending half symbol 4 + bit words 52 + frame bytes 52
       "k_softin_mts01": (392, 1200)}                       # SoftinMts01Lds: ring 128 + bit words 132 + frame bytes 132


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(REPORT):
        from radiosonde_auto_rx_amd import engine
        engine.build_library()
    assert os.path.exists(REPORT), "the build leaves the compiler's resource report at " + REPORT
    return parse_report(open(REPORT).read())


@pytest.mark.parametrize("name", sorted(NEW))
def test_no_scratch_and_no_vector_spills(report, name):
    k = report[name]
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0
    assert k["vgprs"] <= 128                               # a wave per channel, one wave a workgroup: registers never bound the occupancy below LDS


@pytest.mark.parametrize("name", sorted(NEW))
def test_lds_is_the_waves_struct_and_a_second_staged_leaves_eight_waves_on_a_cu(report, name):
    lds, second = NEW[name]
    assert report[name]["lds"] == lds
    assert LDS_PER_CU // (lds + 4 * second) >= 8


def test_the_nine_earlier_kernels_keep_their_lds(report):
    lds = dict(k_softin_rs41=816, k_softin_dfm=1536, k_softin_m10=1228, k_softin_m20=1628, k_softin_rs92=1648, k_softin_imet54=748, k_softin_meisei=272,
               k_softin_drop=2528, k_softin_lms6=38656)
    for name, want in lds.items():
        assert report[name]["scratch"] == 0 and report[name]["vgpr_spill"] == 0, name
        assert report[name]["lds"] == want, (name, report[name]["lds"])
