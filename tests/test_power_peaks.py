"""Host side of the spectrum survey (include/sonde_power.h), no GPU: sonde_power_peaks against auto_rx's own peak pick
(autorx/scan.py:1007-1063 with autorx/utils.py detect_peaks) — recorded cases always, live random cases where the reference tree is present —,
the rtl_power log line through auto_rx's two readers, and the configuration checks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import power_cases as pc                                   # noqa: E402
from radiosonde_auto_rx_amd import power as pw                        # noqa: E402
from radiosonde_auto_rx_amd.engine import ABI_VERSION, SondeError     # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
E_ARG, E_NOGPU = -1, -2                                # SONDE_E_ARG, SONDE_E_NOGPU (include/sonde_hip.h)


def _same(a, b):
    return (a == b) or (np.isnan(a) and np.isnan(b))


def _pick(c):
    freq = np.linspace(c["f_low"], c["f_high"], len(c["power"]))
    return pw.pick_peaks(freq, c["power"], c["step"], return_floor=True, **pc.case_kwargs(c))


def test_recorded_cases_match_auto_rx_exactly():
    g = np.load(os.path.join(GOLDEN, "power_peaks.npz"))
    meta = g["meta"]
    assert len(meta) >= 200
    seen = dict(short=0, even=0, odd=0, nan=0, none=0, never=0, cut=0, plateau=0, lo=0, hi=0, edge=0)
    for i, m in enumerate(meta):
        power = g["power"][g["power_off"][i]:g["power_off"][i + 1]]
        want = g["peaks"][g["peaks_off"][i]:g["peaks_off"][i + 1]]
        never = g["never"][g["never_off"][i]:g["never_off"][i + 1]]
        c = dict(power=power, f_low=m[0], f_high=m[1], step=m[2], snr_threshold=m[3], min_distance=m[4], quantization=m[5], min_freq=m[6], max_freq=m[7],
                 never_scan=list(never), max_peaks=int(m[8]))
        got, nf = _pick(c)
        assert _same(nf, m[9]), (i, nf, m[9])
        assert len(got) == len(want) and (got == want).all(), (i, got, want)
        n = len(power)
        seen["short"] += n < 3; seen["even"] += n % 2 == 0; seen["odd"] += n % 2; seen["nan"] += bool(np.isnan(power).any())
        seen["none"] += len(want) == 0; seen["never"] += len(never) > 0; seen["cut"] += len(want) == int(m[8]) and int(m[8]) < 10
        seen["plateau"] += bool((power[1:] == power[:-1]).any()); seen["lo"] += m[6] > 100.0; seen["hi"] += m[7] < 1000.0
        seen["edge"] += i % 12 == 3
    assert all(v >= 10 for v in seen.values()), seen


def test_live_random_cases_match_auto_rx_exactly():
    mods = pc.autorx_modules()
    if mods is None:
        pytest.skip("reference tree not present (the recorded cases cover the same draw)")
    rng = np.random.default_rng(77)
    npeaks = 0
    for i in range(2000):
        c = pc.random_case(rng, i)
        freq = np.linspace(c["f_low"], c["f_high"], len(c["power"]))
        want, wnf = pc.autorx_pick(mods[0], freq, c["power"], c["step"], **pc.case_kwargs(c))
        got, nf = _pick(c)
        assert _same(nf, wnf), (i, nf, wnf)
        assert len(got) == len(want) and (got == want).all(), (i, got, want)
        npeaks += len(got)
    assert npeaks > 2000


def test_fixture_spectra_give_the_recorded_peaks():
    """the float64 spectra of the three GPU fixtures: same pick as auto_rx recorded, and the margins the fixtures were chosen for"""
    g = np.load(os.path.join(GOLDEN, "power_fixture.npz"))
    for name, (nfft, window, seed, snr, mind) in pc.PEAKS.items():
        lo, hi, step = pc.bin_freqs(nfft, pc.CROP)
        db = g[name + "/db"]
        got, nf = pw.pick_peaks(np.linspace(lo, hi, len(db)), db, step, snr_threshold=snr, min_distance=mind, return_floor=True, **pc.PICK)
        assert (got == g[name + "/peaks"]).all() and nf == float(g[name + "/floor"])
        assert g[name + "/margins"].min() >= 0.05


def test_csv_line_reads_back_through_auto_rx():
    g = np.load(os.path.join(GOLDEN, "power_csv.npz"))
    lo, hi, step = g["args"]
    line = pw.csv_line(1_700_000_000, lo, hi, step, 600_000, g["db"])
    fields = line.rstrip("\n").split(", ")
    assert line.endswith("\n") and fields[0] == "2023-11-14" and fields[1] == "22:13:20" and fields[5] == "600000" and len(fields) == 6 + len(g["db"])
    assert fields[6:9] == ["%.2f" % v for v in g["db"][:3]]
    mods = pc.autorx_modules()
    if mods is not None:                                  # live: both readers of auto_rx
        import tempfile
        with tempfile.NamedTemporaryFile("w", suffix=".csv", delete=False) as f:
            f.write(line)
        try:
            reads = [mods[1].read_rtl_power_log(f.name, "test"), mods[0].read_rtl_power(f.name)]
        finally:
            os.unlink(f.name)
    else:                                                 # recorded: what they returned for this very line
        assert line == str(g["line"])
        reads = [(g["freq"], g["power"], float(g["step"]))]
    for freq, power, st in reads:
        assert (freq == np.linspace(lo, hi, len(g["db"]))).all() and st == step
        assert np.max(np.abs(power - g["db"])) <= 0.005
    # a buffer too small gets nothing but the length
    buf = C.create_string_buffer(16)
    db = np.ascontiguousarray(g["db"], np.float32)
    assert pw._lib().sonde_power_csv_line(1_700_000_000, lo, hi, step, 600_000, db.ctypes.data_as(C.c_void_p), len(db), buf, 16) == len(line) and buf.value == b""


def _create(**kw):
    d = dict(abi_version=ABI_VERSION, device=0, n_streams=1, sample_rate=2_400_000, bits=16, nfft=4096, window=pw.HANN, max_chunk=2_400_000, center_hz=402e6, crop=0.25)
    d.update(kw)
    cfg = pw.PowerCfg(**d)
    h = C.c_void_p()
    rc = pw._lib().sonde_power_create(C.byref(cfg), C.byref(h))
    if rc == 0:
        pw._lib().sonde_power_destroy(h)
    return rc


def test_config_is_validated_before_the_device_is_touched():
    for bad in (dict(nfft=3000), dict(nfft=128), dict(nfft=32768), dict(nfft=0), dict(bits=12), dict(crop=1.0), dict(crop=-0.1), dict(crop=float("nan")),
                dict(window=2), dict(n_streams=0), dict(sample_rate=0), dict(max_chunk=0), dict(abi_version=ABI_VERSION + 1), dict(center_hz=float("inf"))):
        assert _create(**bad) == E_ARG, bad
    assert pw._lib().sonde_power_create(None, None) == E_ARG


def test_create_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert _create() == E_NOGPU
    for nfft in (256, 16384):
        assert _create(nfft=nfft, window=pw.RECT, bits=8, crop=0.0) == E_NOGPU
    with pytest.raises(SondeError):
        pw.PowerSurvey(2_400_000, 4096)


def test_peaks_argument_checks():
    L = pw._lib()
    nf = C.c_double(0)
    assert L.sonde_power_peaks(None, 5, 0.0, 1.0, 1.0, 10.0, 1e3, 1e4, 0.0, 1e9, None, 0, 10, C.byref(nf), None, 0) == E_ARG
    assert L.sonde_power_peaks(None, 0, 0.0, 1.0, 1.0, 10.0, 1e3, 1e4, 0.0, 1e9, None, 0, 10, C.byref(nf), None, 0) == 0 and np.isnan(nf.value)
