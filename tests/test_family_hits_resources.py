"""Scratch, spill and LDS figures of the four k_family_hits<kind> kernels, read from the compiler's own report of sonde_family_hits.hip (the csrc Makefile keeps it
beside the objects: -Rpass-analysis=kernel-resource-usage).  The wave functions are written without indexed local arrays so that nothing goes to scratch memory,
and a kernel's static LDS is the LDS struct of the kind's soft-bit consumer and nothing else — never more than that consumer's kernel has.
No GPU is needed."""
import os
import re

import pytest

from test_kernel_resources import FIELDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc", "obj")
REPORT = os.path.join(OBJ, "sonde_family_hits.resources.txt")
SOFTIN_REPORT = os.path.join(OBJ, "sonde_softin_dev.resources.txt")
# SoftinMeiseiLds (ring 192 + pending half symbol 4 + bit words 76), SoftinImet54Lds (160 + 40 + 224 + 216 + 108), SoftinMts01Lds (128 + 132 +
# 132), SoftinRs92Lds (240 + 80 + 240 + 256 + 64 + 768)
LDS = {"FamilyMeisei": 272, "FamilyImet54": 748, "FamilyMts01": 392, "FamilyRs92": 1648}
SOFTIN = {"FamilyMeisei": "k_softin_meisei", "FamilyImet54": "k_softin_imet54", "FamilyMts01": "k_softin_mts01", "FamilyRs92": "k_softin_rs92"}
KIND_ID = {"FamilyMeisei": 11, "FamilyImet54": 54, "FamilyMts01": 71, "FamilyRs92": 92}


def parse(text):
    """{the kernel's template argument: {field: int}} (the instantiations share one function name)"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            t = re.match(r"_Z13k_family_hitsI\d+(Family[A-Za-z0-9]+?)Ev", m.group(1))
            cur = out.setdefault(t.group(1), {}) if t else None
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*): (\d+) \[-Rpass-analysis", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    return out


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(REPORT):
        from radiosonde_auto_rx_amd import engine
        engine.build_library()
    assert os.path.exists(REPORT), "the build leaves the compiler's resource report at " + REPORT
    return parse(open(REPORT).read())


def test_every_kind_has_a_kernel_without_scratch_and_without_vector_spills(report):
    assert sorted(report) == sorted(LDS)
    for name, k in report.items():
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, name
        assert k["vgprs"] <= 128, name                         # one wave a workgroup: registers never bound the occupancy below eight waves a SIMD


def test_static_lds_is_the_consumers_struct_and_no_more_than_the_consumers_kernel(report):
    from test_kernel_resources import parse_report
    import family_hits_cases as F
    softin = parse_report(open(SOFTIN_REPORT).read())
    emu = F.load_emu()
    for name, want in LDS.items():
        assert report[name]["lds"] == want, (name, report[name]["lds"])
        assert emu.emu_family_lds_bytes(KIND_ID[name]) == want, name           # sizeof the struct, by the host compiler
        assert report[name]["lds"] <= softin[SOFTIN[name]]["lds"], name
