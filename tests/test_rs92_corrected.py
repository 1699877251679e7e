"""sonde_rs92_dec_corrected — print_frame for a frame that has already been through rs92_ecc (what the device soft-bit consumer hands the host) — against
sonde_rs92_dec_bytes on the uncorrected frame: the same text, frame after frame through one decoder each (the calibration rows a decoder collects carry over), on the
frames of the RS92 golden scenarios (tools/make_golden.py RS92_FIELD_SCENARIOS), some with injected byte errors and some beyond correction.  The corrected bytes and
rs_decode's value come from a third decoder's `-r -v` line.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import rs92_softin_cases as M
from tools import synth_rs92 as R

sys.path.insert(0, os.path.join(M.ROOT, "tools"))
import make_golden  # noqa: E402


@pytest.fixture(scope="module")
def host():
    return M.load_host()


@pytest.fixture(scope="module")
def orbits(tmp_path_factory):
    return make_golden.rs92_orbit_files(str(tmp_path_factory.mktemp("rs92corr")))


def _scenario_frames(name, eph):
    sc = make_golden.RS92_FIELD_SCENARIOS[name]
    kw = {k: v for k, v in sc.items() if k not in ("n", "ngp", "aux", "sigma")}
    cal = R.cal_rows(seed=5, freq_khz=1680500, ngp_key=bytes(range(0x31, 0x41))) if sc.get("ngp") else None
    return R.flight(sc["n"], eph, cal=cal, ngp=bool(sc.get("ngp")), aux=sc.get("aux", (0, 0, 0, 0)), **kw)


def _damaged(frames, seed):
    """every third frame clean, the others with 1..12 byte errors in bytes 6..239, two beyond correction (14 and 30 errors)"""
    rng = np.random.default_rng(seed)
    out = []
    for k, f in enumerate(frames):
        f = bytearray(f)
        nerr = 0 if k % 3 == 0 else 14 if k == 4 else 30 if k == 7 else 1 + (5 * k) % 12
        for p in rng.choice(np.arange(6, 240), nerr, replace=False):
            f[int(p)] ^= int(rng.integers(1, 256))
        out.append(bytes(f))
    return out


OPTS = {
    "raw": (dict(raw=1, verbose=1), None),
    "autorx_eph": (dict(M.AUTORX, inv=1, version=b"test"), "E"),
    "vv_ecc2_eph": (dict(verbose=4, aux=1, ptu=1, ecc=2, gpsepoch=-1), "E"),
    "g2_vel2_alm": (dict(verbose=1, gps_verbose=2, gps_vel=2, gpsepoch=-1), "A"),
    "vel_alm_epoch2": (dict(verbose=1, gps_vel=4, gpsepoch=2), "A"),
}


@pytest.mark.parametrize("opts", sorted(OPTS))
@pytest.mark.parametrize("name", ["rs92f_sgp_36", "rs92f_ngp_36", "rs92f_spoiled_8"])
def test_corrected_frame_prints_what_the_uncorrected_one_does(host, orbits, name, opts):
    eph, E, A = orbits
    kw, orb = OPTS[opts]
    if name == "rs92f_ngp_36":
        kw = dict(kw, ngp=1)
    files = dict(ephemeris=E if orb == "E" else None, almanac=A if orb == "A" else None)
    a, b, r = M.host_dec(host, **files, **kw), M.host_dec(host, **files, **kw), M.host_dec(host, raw=1, verbose=1)
    buf, line = C.create_string_buffer(1 << 16), C.create_string_buffer(1024)
    seen, total, text = set(), 0, b""
    for f in _damaged(_scenario_frames(name, eph), 11):
        n = host.sonde_rs92_dec_bytes(a, f, 240, buf, len(buf))
        assert n >= 0
        want = buf.raw[:n]
        assert host.sonde_rs92_dec_bytes(r, f, 240, line, 1024) > 0
        ec, fixed = M.parse_raw_line(line.value.decode().rstrip("\n"))
        assert (fixed == f) == (ec <= 0)
        n = host.sonde_rs92_dec_corrected(b, fixed, ec, buf, len(buf))
        assert n >= 0 and buf.raw[:n] == want
        seen.add(min(ec, 1)); total += n; text += want
    for d in (a, b, r):
        host.sonde_rs92_dec_destroy(d)
    assert seen == {-1, 0, 1} and total > 500
    if orb and kw.get("json"):
        assert text.count(b'"lat"') >= 5                      # (positions and their JSON were part of what was compared)


def test_corrected_refuses_bad_arguments(host):
    d = M.host_dec(host, raw=1)
    buf = C.create_string_buffer(1024)
    f = M.frames()[0]
    assert host.sonde_rs92_dec_corrected(None, f, 0, buf, 1024) < 0
    assert host.sonde_rs92_dec_corrected(d, None, 0, buf, 1024) < 0
    assert host.sonde_rs92_dec_corrected(d, f, 0, buf, 100) < 0     # 480 hex characters do not fit
    assert host.sonde_rs92_dec_corrected(d, f, 0, buf, 1024) == 481
    host.sonde_rs92_dec_destroy(d)
