"""CPU-side checks of the iMet-4 engine's float32 input and run-time channels (include/sonde_imet4.h): what create answers to `bits` without a
device, the new entry points, and the float32 golden table (tests/imet4_f32_cases.py, tools/make_golden_imet4_f32.py).  No GPU is used."""
import ctypes as C
import os

import pytest

from tests import imet4_f32_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_NOGPU = -1, -2                                    # SONDE_E_ARG, SONDE_E_NOGPU (include/sonde_hip.h)
NEW = ("sonde_imet4_process_device_strided", "sonde_imet4_restart_channel", "sonde_imet4_release_channel", "sonde_imet4_channel_active")


def _create(bits, iq=1):
    from radiosonde_auto_rx_amd.engine import lib
    from radiosonde_auto_rx_amd.imet4 import Imet4Cfg, _sigs
    L = _sigs(lib())
    cfg = Imet4Cfg(sample_rate=48000, bits=bits, iq=iq, lp_iq=iq, dc=1)
    fq = (C.c_double * 1)(0.0)
    h = C.c_void_p()
    rc = L.sonde_imet4_create(C.byref(cfg), 1, fq, 12000, C.byref(h), None, None)
    if h:
        L.sonde_imet4_destroy(h)
    return rc


def test_float32_is_accepted_as_far_as_the_device_check():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert _create(32) == E_NOGPU                          # float32 IQ: a configuration the engine has, there is only no device
    assert _create(32, iq=0) == E_NOGPU                    # float32 FM audio
    assert _create(16) == E_NOGPU and _create(8) == E_NOGPU


def test_other_widths_are_refused():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert _create(24) == E_ARG
    assert _create(64) == E_ARG and _create(0) == E_ARG


def test_new_entry_points_are_exported_and_declared():
    from radiosonde_auto_rx_amd.engine import lib
    from radiosonde_auto_rx_amd.imet4 import _sigs
    L = _sigs(lib())
    hdr = open(os.path.join(ROOT, "include", "sonde_imet4.h")).read()
    for n in NEW:
        assert hasattr(L, n), n
        assert n + "(" in hdr, n


def test_calls_on_no_engine_are_refused():
    """host code in front of the device: a NULL engine is SONDE_E_ARG for each of the new calls"""
    from radiosonde_auto_rx_amd.engine import lib
    from radiosonde_auto_rx_amd.imet4 import _sigs
    L = _sigs(lib())
    assert L.sonde_imet4_restart_channel(None, 0, 0.0) == E_ARG
    assert L.sonde_imet4_release_channel(None, 0) == E_ARG
    assert L.sonde_imet4_channel_active(None, 0) == E_ARG
    assert L.sonde_imet4_process_device_strided(None, None, 0, 0) == E_ARG


def _frames(argv, out: bytes) -> int:
    lines = [l for l in out.decode("latin-1").split("\n") if l]
    if "--rawbits" in argv:
        return len(lines)
    return sum(1 for l in lines if l.startswith("("))     # the GPS line every frame of these captures prints


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_golden_table_is_honest(name):
    case = cases.CASES[name]
    assert os.path.exists(os.path.join(cases.GOLDEN, "imet4f32_%s.npz" % name)), name
    g = cases.load(name)
    assert g["argv"] == case["argv"] and g["params"] == case["gen"]
    assert len(g["stdout"]) == len(case["argv"])
    for argv, out in zip(g["argv"], g["stdout"]):
        assert "32" in argv or "{wav}" in argv
        assert _frames(argv, out) >= 3, (name, argv, _frames(argv, out))


def test_every_golden_file_has_its_case():
    have = sorted(f[len("imet4f32_"):-4] for f in os.listdir(cases.GOLDEN) if f.startswith("imet4f32_") and f.endswith(".npz"))
    assert have == sorted(cases.CASES)
