"""sonde_mrz_dec_decoded (include/sonde_mrz.h): what a soft-bit consumer's fetch call prints a frame with — the device's bits and the DEVICE's CRC verdict, through
the body print_frame shares.  Fed the arbiter's bits and verdicts (tests/mrz_softin_cases.py: the host tier a half symbol at a time) it must print, byte for byte,
what sonde_mrz_dec_push_soft prints for the same stream under every output form; fed a wrong verdict it prints that verdict, which proves it computes none."""
import ctypes as C

import numpy as np
import pytest

import mrz_softin_cases as M
from tools import synth


@pytest.fixture(scope="module")
def host():
    return M.load_host()


_streams = {}


def _stream(kind):
    """20 seconds at sigma 0.1: long enough for the date (configuration word 15) and both serial numbers, so the JSON starts; two copies a second, so --uniq drops
    lines; "latlon": the frame length goes to 384 bits behind the first good frame"""
    if kind not in _streams:
        rng = np.random.default_rng(20)
        frames = [synth.mrz_frame(k, latlon=(kind == "latlon")) for k in range(20) for _ in range(2)]
        s = M.train(rng, frames)
        _streams[kind] = (s + M.noise(rng, len(s), 0.1)).astype(np.float32)
    return _streams[kind]


def _decoded(host, s, frames, **kw):
    h = M.host_dec(host, **kw)
    buf = C.create_string_buffer(4096)
    out = []
    for f in frames:
        n = host.sonde_mrz_dec_decoded(h, f[3], f[1], f[4], buf, 4096)
        assert n >= 0
        out.append(buf.raw[:n].decode())
        assert host.sonde_mrz_dec_frame_bits(h) + 22 == (f[1] if not f[4] or kw.get("raw") == 2 else (f[5] + 6) * 8)      # in step with the device's verdict
    host.sonde_mrz_dec_destroy(h)
    return out


FORMS = {"-r": dict(raw=1), "-R": dict(raw=2), "default": {}, "-v": dict(verbose=1), "-vv --ptu --dbg": dict(verbose=2, ptu=1, dbg=1),
         "--json --ptu": dict(json=1, ptu=1, version="oracle", jsn_freq_khz=403000), "--json --ptu --uniq": dict(json=1, ptu=1, uniq=1)}


@pytest.mark.parametrize("kind", ["ecef", "latlon"])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_decoded_text_equals_the_host_tier(host, kind, form):
    s = _stream(kind)
    raw2 = FORMS[form].get("raw") == 2
    frames = M.host_frames(host, s, raw2=raw2, cache=("decoded", kind, raw2))
    assert len(frames) >= 30 and (raw2 or sum(f[4] for f in frames) >= 30)
    assert raw2 or {f[1] for f in frames} == ({408} if kind == "ecef" else {408, 384})
    want = M.host_text(host, s, **FORMS[form])
    got = _decoded(host, s, frames, **FORMS[form])
    assert "".join(got) == want
    if "json" in FORMS[form]:
        assert want.count('"type": "MRZ"') >= 4                  # (date and both serial numbers are known from second 15 on)
    if "uniq" in FORMS[form]:
        assert sum(1 for t in got if t == "") >= 10               # the second copy of a second prints nothing


def test_the_verdict_is_the_callers(host):
    s = _stream("ecef")
    frames = [f for f in M.host_frames(host, s, cache=("decoded", "ecef", False))]
    good = [f for f in frames if f[4]][:4]
    bad = [f for f in frames if not f[4]][:1] or [(0, 408, 0, bytes(52), 0, 45)]
    assert [t.rstrip()[-4:] for t in _decoded(host, s, good, raw=1)] == ["[OK]"] * 4
    flipped = [f[:4] + (0,) + f[5:] for f in good]
    assert [t.rstrip()[-4:] for t in _decoded(host, s, flipped, raw=1)] == ["[NO]"] * 4
    forced = [f[:4] + (1,) + f[5:] for f in bad]
    assert [t.rstrip()[-4:] for t in _decoded(host, s, forced, raw=1)] == ["[OK]"]
    assert all("[NO]" in t for t in _decoded(host, s, flipped)) and all("[OK]" in t for t in _decoded(host, s, good))


def test_argument_checks(host):
    h = M.host_dec(host, raw=1)
    buf = C.create_string_buffer(64)
    big = C.create_string_buffer(4096)
    assert host.sonde_mrz_dec_decoded(None, bytes(52), 408, 1, big, 4096) == -1
    assert host.sonde_mrz_dec_decoded(h, None, 408, 1, big, 4096) == -1
    assert host.sonde_mrz_dec_decoded(h, bytes(52), 400, 1, big, 4096) == -1
    assert host.sonde_mrz_dec_decoded(h, bytes(52), 408, 1, None, 4096) == -1
    assert host.sonde_mrz_dec_decoded(h, bytes(52), 408, 1, buf, 64) == -1           # the text does not fit
    assert host.sonde_mrz_dec_decoded(h, bytes(52), 384, 0, big, 4096) == 3 * 47 + 6
    host.sonde_mrz_dec_destroy(h)
