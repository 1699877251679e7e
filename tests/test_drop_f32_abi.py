"""CPU-side checks of the dropsonde engine's float32 input and run-time channels (include/sonde_drop.h): the new entry points, what
sonde_drop_design and create answer to `bits = 32` without a device, and the float32 golden table (tests/dropf32_cases.py,
tools/make_golden_drop_f32.py).  No GPU is used."""
import ctypes as C
import json
import os

import pytest

from tests import dropf32_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_NOGPU = -1, -2                                    # SONDE_E_ARG, SONDE_E_NOGPU (include/sonde_hip.h)
NEW = ("sonde_drop_process_device_strided", "sonde_drop_restart_channel", "sonde_drop_release_channel", "sonde_drop_channel_active",
       "sonde_drop_finish_channel", "sonde_drop_read_fm")


def _lib():
    from radiosonde_auto_rx_amd.drop import _sigs
    from radiosonde_auto_rx_amd.engine import lib
    return _sigs(lib())


def _design(sr, bits, input=0):
    from radiosonde_auto_rx_amd.drop import DropCfg, DropInfo
    cfg, inf = DropCfg(sample_rate=sr, input=input, bits=bits, opt_b=1), DropInfo()
    return _lib().sonde_drop_design(C.byref(cfg), C.byref(inf)), inf


def _create(sr, bits, input=0):
    from radiosonde_auto_rx_amd.drop import DropCfg
    L = _lib()
    cfg = DropCfg(sample_rate=sr, input=input, bits=bits, opt_b=1)
    fq = (C.c_double * 1)(0.0)
    h = C.c_void_p()
    rc = L.sonde_drop_create(C.byref(cfg), 1, fq, 12000, C.byref(h))
    if h:
        L.sonde_drop_destroy(h)
    return rc


def test_new_entry_points_are_exported_and_declared():
    L = _lib()
    hdr = open(os.path.join(ROOT, "include", "sonde_drop.h")).read()
    for n in NEW:
        assert hasattr(L, n), n
        assert n + "(" in hdr, n


@pytest.mark.parametrize("sr", [48000, 50000])
def test_design_answers_for_float32_where_iq_dec_does_not_decimate(sr):
    rc, inf = _design(sr, 32)
    assert rc == 0
    assert (inf.if_rate, inf.dec_m, inf.taps_dec) == (sr, 1, 0)
    assert inf.taps_fm == {48000: 97, 50000: 101}[sr]      # 4 sr / 2000, made odd (iq_dec.c:743)
    assert abs(inf.sps - sr / 4800.0) < 1e-5
    rc16, inf16 = _design(sr, 16)                          # the same numbers as for the integer widths
    assert rc16 == 0 and (inf16.if_rate, inf16.dec_m, inf16.taps_fm, inf16.sps) == (inf.if_rate, inf.dec_m, inf.taps_fm, inf.sps)


def test_design_refuses_float32_elsewhere():
    assert _design(48000, 32, input=1)[0] == E_ARG         # the FM form
    assert _design(96000, 32)[0] == E_ARG                  # iq_dec decimates: IF 48000, dec 2
    assert _design(100000, 32)[0] == E_ARG                 # IF 50000, dec 2
    assert _design(96000, 16)[0] == 0 and _design(96000, 16)[1].dec_m == 2
    assert _design(48000, 24)[0] == E_ARG and _design(48000, 64)[0] == E_ARG


def test_create_refuses_before_it_looks_for_a_device():
    assert _create(48000, 32, input=1) == E_ARG
    assert _create(96000, 32) == E_ARG
    assert _create(100000, 32) == E_ARG
    assert _create(48000, 24) == E_ARG


def test_float32_is_accepted_as_far_as_the_device_check():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert _create(48000, 32) == E_NOGPU and _create(50000, 32) == E_NOGPU
    assert _create(48000, 16) == E_NOGPU


def test_calls_on_no_engine_are_refused():
    """host code in front of the device: a NULL engine is SONDE_E_ARG for each of the new calls"""
    L = _lib()
    assert L.sonde_drop_process_device_strided(None, None, 0, 0) == E_ARG
    assert L.sonde_drop_restart_channel(None, 0, 0.0) == E_ARG
    assert L.sonde_drop_release_channel(None, 0) == E_ARG
    assert L.sonde_drop_channel_active(None, 0) == E_ARG
    assert L.sonde_drop_finish_channel(None, 0) == E_ARG
    assert L.sonde_drop_read_fm(None, 0, 0, 0, None) == E_ARG


def test_python_mirror_has_the_calls():
    from radiosonde_auto_rx_amd.drop import DropEngine, design
    for n in ("restart_channel", "release_channel", "finish_channel", "channel_active", "process_device", "read_fm"):
        assert callable(getattr(DropEngine, n)), n
    assert design(50000, bits=32)["taps_fm"] == 101


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_golden_table_is_honest(name):
    case = cases.CASES[name]
    assert os.path.exists(os.path.join(cases.GOLDEN, "dropf32_%s.npz" % name)), name
    g = cases.load(name)
    assert g["argv"] == case["argv"] and g["params"] == json.loads(json.dumps(case["gen"])) and g["fq"] == case["fq"]
    assert len(g["stdout"]) == len(case["argv"]) and g["rc"] == [0] * len(case["argv"])
    assert case["gen"]["sr"] in (48000, 50000) and all("-b" in a for a in case["argv"])
    n = len(cases.samples(case["gen"])) // 2
    assert n <= 2 * case["gen"]["sr"], n                   # at most 2 s of signal
    if not case["gen"].get("invert"):
        assert sum(o.count(b"\n") for o in g["stdout"]) >= 3, name
    else:                                                  # nothing without -i, every frame with it
        assert g["stdout"][0] == b"" and g["stdout"][1].count(b'"type"') == 3


def test_every_golden_file_has_its_case():
    have = sorted(f[len("dropf32_"):-4] for f in os.listdir(cases.GOLDEN) if f.startswith("dropf32_") and f.endswith(".npz"))
    assert have == sorted(list(cases.CASES) + list(cases.WIDE) + ["emu"])
