"""The one owner of device memory behind the host objects (radiosonde_auto_rx_amd/csrc/sonde_devmem.h) and the page-locked host buffer
(sonde_pinned.h), compiled by plain g++ against a fake HIP allocator (tests/emu/devmem_fake.cpp: malloc and a set of live pointers, no HIP
library linked) and run on the CPU: nothing stays live behind a scope exit, behind a create that fails at ANY of its allocations, or behind a
staging buffer that regrows; nothing is freed twice (the fake ends the program on a free of a pointer that is not live); a pointer that
was assigned without being registered is left alone."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radiosonde_auto_rx_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "emu", "devmem_fake.cpp")
EXE = os.path.join(ROOT, "tests", "emu", "devmem_fake")
DEPS = [SRC, os.path.join(CSRC, "sonde_devmem.h"), os.path.join(CSRC, "sonde_pinned.h")]
HIP_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        tmp = EXE + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INCLUDE, "-o", tmp, SRC])
        os.replace(tmp, EXE)
    p = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    return p.stdout


def test_no_check_failed(report):
    assert "FAILED" not in report, report
    assert re.search(r"failed checks 0$", report.strip()), report


def test_scope_exit_frees_everything(report):
    assert "case 1: allocations 7 live after 0" in report, report


def test_every_failing_allocation_cleans_up(report):
    """the k-th of the 7 allocations of a create fails, for every k: SONDE_E_NOMEM each time, nothing live, the failed slot nullptr"""
    assert "case 2: failures 7 of 7 live after 0" in report, report


def test_regrow_empty_upload_and_unregistered_pointer(report):
    for case in (3, 4, 5):
        assert "case %d: live after 0" % case in report, report


def test_every_allocation_was_freed_once(report):
    m = re.search(r"device allocations (\d+) frees (\d+) host allocations (\d+) frees (\d+)", report)
    assert m, report
    da, df, ha, hf = map(int, m.groups())
    # by count of the program's calls that succeed — device: 5 (case 1) + 0+1+2+2+3+4+4 (case 2) + 4 + 4 + 6; host: 2 + 0+0+0+1+1+1+2 + 2 + 2
    assert (da, df, ha, hf) == (35, 35, 11, 11), m.groups()
