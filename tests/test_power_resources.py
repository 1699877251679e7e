"""What the compiler reports for the survey's kernels (radiosonde_auto_rx_amd/csrc/sonde_power.hip; the csrc Makefile keeps the report beside the
objects): every size of the transform without spills or scratch, with the padded LDS array and the workgroup size the launch shape is built on
(DESIGN.md 4.17).  No GPU is needed."""
import os
import re

import pytest

from test_kernel_resources import parse_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc", "obj", "sonde_power.resources.txt")


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(REPORT):
        from radiosonde_auto_rx_amd import engine
        engine.build_library()
    assert os.path.exists(REPORT), "the build leaves the compiler's resource report at " + REPORT
    text = open(REPORT).read()
    # the survey's kernels live in an anonymous namespace: _ZN12_GLOBAL__N_1<len><name>I...; keep name and, for the transform, its size
    out = {}
    for sym, rec in parse_report(text).items():
        m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", sym)
        assert m, sym
        n = int(m.group(1))
        name, rest = sym[m.end():m.end() + n], sym[m.end() + n:]
        t = re.match(r"ILi(\d+)EE", rest)
        out[name + ("<%s>" % t.group(1) if t else "<%s>" % rest)] = rec
    return out


def test_no_kernel_of_the_survey_spills(kernels):
    assert sum(k.startswith("k_power_seg<") for k in kernels) == 7 and any(k.startswith("k_power_fold") for k in kernels) and sum(k.startswith("k_power_tail") for k in kernels) == 3
    for name, r in kernels.items():
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)


@pytest.mark.parametrize("log2n", range(8, 15))
def test_transform_lds_and_registers_fit_the_launch_shape(kernels, log2n):
    n = 1 << log2n
    r = kernels["k_power_seg<%d>" % log2n]
    assert r["lds"] == 8 * (n + n // 16 + n // 256)                    # 139776 bytes at 16384 points: one workgroup per CU; 34944 at 4096: four
    threads = min(512, max(64, n // 8))
    waves_per_simd = -(-threads // 64 // 4)                             # waves of one workgroup on each of a CU's four SIMDs
    assert r["occupancy"] >= waves_per_simd, r                          # the workgroup fits: registers never limit it below one per CU
    assert r["vgprs"] <= 512 // waves_per_simd, r
