"""Register, scratch and occupancy figures of the tuned kernels, read from the compiler's own report of sonde_kernels.hip (the csrc Makefile keeps
it beside the objects: -Rpass-analysis=kernel-resource-usage).  The IF-rate tail depends on them the way the decimator depends on its 168 registers:
k_search_sync and k_sync_window_fft ran with their working set in scratch memory until the addresses a thread derives from its index stopped being
hoisted over the whole state machine, and k_if_chain holds eight workgroups per CU only under 64 vector and 96 scalar registers.  No GPU is needed."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc", "obj", "sonde_kernels.resources.txt")

FIELDS = {
    "VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
    "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill", "LDS Size [bytes/block]": "lds",
}


def parse_report(text):
    """{kernel name as written in the source (template arguments kept, e.g. 'k_framesync<false>'): {field: int}}"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(_demangle(m.group(1)), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*): (\d+) \[-Rpass-analysis", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    return out


def _demangle(sym):
    """_Z<len><name>[I Lb<0|1>E E]...: the kernels here are plain functions or templates over one bool"""
    m = re.match(r"_Z(\d+)", sym)
    if not m:
        return sym
    n = int(m.group(1))
    name, rest = sym[m.end():m.end() + n], sym[m.end() + n:]
    t = re.match(r"ILb([01])EE", rest)
    return name + ("<%s>" % ("true" if t.group(1) == "1" else "false") if t else "")


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(REPORT):
        from radiosonde_auto_rx_amd import engine
        engine.build_library()
    assert os.path.exists(REPORT), "the build leaves the compiler's resource report at " + REPORT
    r = parse_report(open(REPORT).read())
    assert len(r) >= 20, sorted(r)
    return r


def test_parser_reads_a_remark_block():
    text = """sonde_kernels.hip:2085:1: remark: Function Name: _Z11k_framesyncILb0EEv8SyncArgs [-Rpass-analysis=kernel-resource-usage]
sonde_kernels.hip:2085:1: remark:     TotalSGPRs: 106 [-Rpass-analysis=kernel-resource-usage]
sonde_kernels.hip:2085:1: remark:     VGPRs: 123 [-Rpass-analysis=kernel-resource-usage]
sonde_kernels.hip:2085:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
sonde_kernels.hip:2085:1: remark:     Dynamic Stack: False [-Rpass-analysis=kernel-resource-usage]
sonde_kernels.hip:2085:1: remark:     Occupancy [waves/SIMD]: 4 [-Rpass-analysis=kernel-resource-usage]
sonde_kernels.hip:2085:1: remark:     SGPRs Spill: 148 [-Rpass-analysis=kernel-resource-usage]
sonde_kernels.hip:2085:1: remark:     VGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
sonde_kernels.hip:2085:1: remark:     LDS Size [bytes/block]: 2244 [-Rpass-analysis=kernel-resource-usage]
sonde_kernels.hip:277:1: remark: Function Name: _Z16k_mix_decimate5010MixDecArgs [-Rpass-analysis=kernel-resource-usage]
sonde_kernels.hip:277:1: remark:     VGPRs: 168 [-Rpass-analysis=kernel-resource-usage]
"""
    r = parse_report(text)
    assert r["k_framesync<false>"] == {"sgprs": 106, "vgprs": 123, "scratch": 0, "occupancy": 4, "sgpr_spill": 148, "vgpr_spill": 0, "lds": 2244}
    assert r["k_mix_decimate50"] == {"vgprs": 168}


def test_search_sync_has_no_scratch(report):
    k = report["k_search_sync"]
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["vgprs"] <= 128, k
    assert k["occupancy"] >= 4, k                        # two workgroups of eight waves per CU


@pytest.mark.parametrize("name", ["k_if_chain", "k_if_chain_multi"])
def test_if_chain_registers(report, name):
    k = report[name]
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["vgprs"] <= 72, k


def test_decimator_unchanged(report):
    k = report["k_mix_decimate50"]
    assert k["vgprs"] == 168 and k["scratch"] == 0 and k["occupancy"] == 3, k


def test_shared_bodies_not_worse(report):
    """the kernels that share k_search_sync's bodies: no more scratch than before the bodies were changed for it (48 B and 0 B)"""
    assert report["k_sync_window_fft"]["scratch"] <= 48, report["k_sync_window_fft"]
    assert report["k_framesync<false>"]["scratch"] == 0, report["k_framesync<false>"]
