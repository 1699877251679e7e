"""sonde_mts01_dec_decoded (include/sonde_mts01.h): what a soft-bit consumer's fetch call prints a frame with — the device's 131 bytes, the device's CRC value and
the DEVICE's verdict, through the body print_frame shares.  Fed the arbiter's bytes and verdicts (tests/mts01_softin_cases.py: the host tier a symbol at a time) it
must print, byte for byte, what sonde_mts01_dec_push_soft prints for the same stream under every output form; fed a wrong verdict it prints that verdict, which
proves it computes none."""
import ctypes as C

import numpy as np
import pytest

import mts01_softin_cases as M
from tools import synth


@pytest.fixture(scope="module")
def host():
    return M.load_host()


_stream = {}


def _s():
    """20 seconds at sigma 0.25 (a frame a second; some fail their CRC) with a frame without a NUL and one with an early NUL among them"""
    if "s" not in _stream:
        rng = np.random.default_rng(21)
        s = np.concatenate([M.soft(synth.mts01_onair_bits(20)), M.cases()["no_nul"]["s"], M.cases()["early_nul"]["s"]])
        _stream["s"] = (s + M.noise(rng, len(s), 0.25)).astype(np.float32)
    return _stream["s"]


def _decoded(host, frames, **kw):
    h = M.host_dec(host, **kw)
    buf = C.create_string_buffer(8192)
    out = []
    for f in frames:
        n = host.sonde_mts01_dec_decoded(h, f[1], f[2], f[4], buf, 8192)
        assert n >= 0
        out.append(buf.raw[:n].decode("latin-1"))
    host.sonde_mts01_dec_destroy(h)
    return out


FORMS = {"-r": dict(raw=1), "-R": dict(raw=2), "default": {}, "-v": dict(verbose=1), "--json": dict(json=1, version="oracle", jsn_freq_khz=403000),
         "-v --json": dict(verbose=1, json=1)}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_decoded_text_equals_the_host_tier(host, form):
    s = _s()
    frames = M.host_frames(host, s, cache="decoded")
    assert len(frames) == 22 and sum(f[4] for f in frames) >= 12
    want = M.host_text(host, s, **FORMS[form])
    assert "".join(_decoded(host, frames, **FORMS[form])) == want
    if "json" in FORMS[form]:
        assert want.count('"type": "MTS01"') == sum(f[4] for f in frames)
    if form == "-R":
        assert all(len(l) == 1048 + 131 for l in want.splitlines())


def test_the_verdict_and_the_crc_value_are_the_callers(host):
    frames = M.host_frames(host, _s(), cache="decoded")
    good = [f for f in frames if f[4]][:4]
    assert [t.rstrip()[-4:] for t in _decoded(host, good, raw=1)] == ["[OK]"] * 4
    flipped = [(f[0], f[1], 0xBEEF, f[3], 0, f[5]) for f in good]
    lines = _decoded(host, flipped, raw=1)
    assert [t.rstrip()[-4:] for t in lines] == ["[NO]"] * 4 and all(":BEEF]" in t for t in lines)
    assert all("[NO]" in t and '"type"' not in t for t in _decoded(host, flipped, json=1))
    assert all("[OK]" in t and '"type"' in t for t in _decoded(host, good, json=1))


def test_argument_checks(host):
    h = M.host_dec(host, raw=1)
    big = C.create_string_buffer(4096)
    small = C.create_string_buffer(64)
    assert host.sonde_mts01_dec_decoded(None, bytes(131), 0, 1, big, 4096) == -1
    assert host.sonde_mts01_dec_decoded(h, None, 0, 1, big, 4096) == -1
    assert host.sonde_mts01_dec_decoded(h, bytes(131), 0, 1, None, 4096) == -1
    assert host.sonde_mts01_dec_decoded(h, bytes(131), 0, 1, small, 64) == -1        # the text does not fit
    assert host.sonde_mts01_dec_decoded(h, bytes(131), 0x1234, 0, big, 4096) == 3 * 131 + 14 + 7 + 1
    host.sonde_mts01_dec_destroy(h)
