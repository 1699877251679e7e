"""SoftinDev(kind="rs92") — `rs92mod --softin [-i] --ecc` for many channels on the device (k_softin_rs92 = radiosonde_auto_rx_amd/csrc/sonde_softin_rs92_dev.h
compiled by hipcc): the consumer half of auto_rx's pipe `fsk_demod --cs16 -b -20000 -u 20000 -s 2 48000 4800 - - | rs92mod -vx -v --crc --ecc --vel --json --softin -i
-e <rinex> --ptu`.  Arbiters: the same source under the CPU wave emulator on the streams of tests/rs92_softin_cases.py (ec, hdr_bit and the frame bytes exactly, mv to
within one float ulp: the device's double divide and sqrt come ahead of the rounding to float), the host tier sonde_rs92_dec_push_soft for the text and its JSON, and
the compiled reference behind the modem."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rs92_softin_cases as M
from golden_cases import need_ref

ROOT = M.ROOT
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emu():
    return M.load_emu()


@pytest.fixture(scope="module")
def host():
    return M.load_host()


@pytest.fixture(scope="module")
def rinex(tmp_path_factory):
    return M.rinex_file(tmp_path_factory.mktemp("rs92gpu"))


def _same(got, want):
    """records of one channel (fetch_rs92 dicts) against the emulator's Recs: everything exact but mv, mv within one ulp"""
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        g, w = M.full(g), M.full(w)
        assert g[:3] == w[:3]
        assert M.mv_within_one_ulp(g, w)


def _device(streams, calls, inv=0, softinv=False, opts=None, rinex=None):
    """equally long streams, a channel each, through one consumer in calls of calls[0], calls[1], .. symbols (the last length repeats): per channel the fetched dicts,
    the consumer's counts"""
    import torch
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    S = np.ascontiguousarray(np.stack(streams), np.float32)
    n = S.shape[1]
    o = dict(M.AUTORX, inv=inv)
    o.update(opts or {})
    sf = SoftinDev(len(streams), kind="rs92", softinv=softinv, rs92_opts=o, ephemeris=rinex)
    d = torch.from_numpy(S).cuda()
    recs = {c: [] for c in range(len(streams))}
    pos, i = 0, 0
    while pos < n:
        k = min(calls[min(i, len(calls) - 1)], n - pos)
        chunk = d[:, pos:pos + k].contiguous()
        sf.push_device(chunk.data_ptr(), k, k)
        for f in sf.fetch_rs92():
            recs[f["channel"]].append(f)
        pos += k; i += 1
    cnt = sf.counts()
    sf.close()
    return recs, cnt


def _counts(recs, dropped=0):
    """the tallies the fetched records imply (frames = delivered ones, as for the other kinds; the dropped ones are counted apart)"""
    ecs = [f["ec"] for r in recs.values() for f in r]
    return dict(frames=len(ecs), ecc_ok=sum(e >= 0 for e in ecs), repaired=sum(e > 0 for e in ecs), symbols=sum(e for e in ecs if e > 0), dropped=dropped)


# ---------------------------------------------------------------- 1. the emulator's cases on the device, three channels a consumer
def _groups():
    by = {}
    for name in sorted(M.cases()):
        c = M.cases()[name]
        by.setdefault((c["inv"], c["softinv"]), []).append(name)
    out = []
    for (inv, softinv), names in sorted(by.items()):
        while len(names) % 3:
            names.append(names[0])                            # (a consumer's third channel: one of its streams again)
        out += [(inv, softinv, tuple(names[i:i + 3])) for i in range(0, len(names), 3)]
    return out


GROUPS = _groups()
_emu_recs = {}


def _padded(names, seed):
    """the group's streams brought to one length by a quiet tail (no header in it: the records stay those of the case)"""
    rng = np.random.default_rng(seed)
    ss = [M.cases()[nm]["s"] for nm in names]
    n = max(len(s) for s in ss)
    return [np.concatenate([s, M.noise(rng, n - len(s), 0.05)]) for s in ss]


def _mixed_calls(n, seed):
    """different lengths call after call: a dozen of the short cuts, then one of the long ones"""
    rng = np.random.default_rng(seed)
    out, tot = [], 0
    while tot < n:
        out += [int(v) for v in rng.choice(M.CUTS[:7], 12)] + [int(rng.choice(M.CUTS[7:]))]
        tot = sum(out)
    return out


@pytest.mark.parametrize("cut", [False, True], ids=["one_call", "cut"])
@pytest.mark.parametrize("group", GROUPS, ids=["-".join(g[2]) for g in GROUPS])
def test_cases_on_the_device_equal_emulator_and_host_text(emu, host, rinex, group, cut):
    inv, softinv, names = group
    streams = _padded(names, 7)
    n = len(streams[0])
    calls = _mixed_calls(n, 31 + GROUPS.index(group)) if cut else [n]
    recs, cnt = _device(streams, calls, inv, softinv, opts=dict(version="t"), rinex=rinex)
    for c, nm in enumerate(names):
        if nm not in _emu_recs:
            case = M.cases()[nm]
            _emu_recs[nm] = M.emu_frames(emu, case["s"], [len(case["s"])], inv, softinv)[0]
        want = _emu_recs[nm]
        assert len(want) == M.cases()[nm]["n"]
        _same(recs[c], want)
        text = "".join(f["text"] for f in recs[c])
        assert text == M.host_text(host, streams[c], inv, softinv, ephemeris=rinex, version=b"t")
        assert text.count('"lat"') == sum(w.ec >= 0 for w in want)          # every accepted frame of the flight has its position
    assert cnt == _counts(recs)


# ---------------------------------------------------------------- 2. channel indexing
def test_320_channels_in_one_launch_keep_their_frames_apart(host):
    from tools import synth_rs92 as R
    rng = np.random.default_rng(320)
    nch = 320
    fl = R.flight(nch, M.ephs(), frame0=100)
    n = 2 * (nch - 1) + 3 + M.ONAIR + 70
    streams = []
    for c in range(nch):
        s = np.concatenate([M.noise(rng, 2 * c + 3, 0.05), M.soft(R.frame_symbols(fl[c]), rng, (0.8, 1.2))])
        streams.append(np.concatenate([s, M.noise(rng, n - len(s), 0.05)]))
    recs, cnt = _device(streams, [n], opts=dict(raw=1, json=0))
    for c in range(nch):
        assert len(recs[c]) == 1
        f = recs[c][0]
        assert (f["ec"], f["hdr_bit"], f["frame"]) == (0, 2 * c + 3 + 120, fl[c])
        assert f["text"] == M.raw_line(fl[c], 0) + "\n"
    assert len({r[0]["frame"] for r in recs.values()}) == nch
    assert cnt == dict(frames=nch, ecc_ok=nch, repaired=0, symbols=0, dropped=0)


# ---------------------------------------------------------------- 3. the record cap
def test_record_cap_on_the_device(emu):
    rng = np.random.default_rng(9)
    first = M.cap_stream(22)
    s = np.concatenate([first, M.soft(M.fsym(23)), M.noise(rng, 80, 0.05)])
    calls = [len(first), len(s) - len(first)]
    want, dropped, _ = M.emu_frames(emu, s, calls, cap=20)
    assert dropped == 2 and len(want) == 21
    recs, cnt = _device([s], calls, opts=dict(raw=1, json=0))
    _same(recs[0], want)
    assert recs[0][-1]["frame"] == M.frames()[23]
    assert cnt == _counts(recs, dropped=2)


# ---------------------------------------------------------------- 4. refusals
def test_create_and_fetch_refusals(rinex):
    from radiosonde_auto_rx_amd.engine import SondeError, SondeM20Frame, SONDE_RS92
    from radiosonde_auto_rx_amd.fsk import SoftinDev, _lib, Rs92SoftinRec
    L = _lib()
    h = C.c_void_p()
    assert L.sonde_softin_dev_create(1, SONDE_RS92, 0, 0, 0, 0, C.byref(h)) == -1              # SONDE_E_ARG: the kind needs its options
    with pytest.raises(SondeError):
        SoftinDev(1, kind="rs92", rs92_opts=dict(gps_verbose=8))
    with pytest.raises(SondeError):
        SoftinDev(1, kind="rs92", rs92_opts=dict(dbg=1))
    sf = SoftinDev(1, kind="m20")
    buf = (Rs92SoftinRec * 2)()
    assert L.sonde_softin_dev_fetch_rs92(sf._h, buf, 2) == -1
    assert L.sonde_softin_dev_rs92_load_ephemeris(sf._h, os.fsencode(rinex)) == -1 == L.sonde_softin_dev_rs92_load_almanac(sf._h, os.fsencode(rinex))
    with pytest.raises(SondeError):
        sf.fetch_rs92()
    sf.close()
    sf = SoftinDev(2, kind="rs92", ephemeris=rinex)
    m20 = (SondeM20Frame * 2)()
    assert L.sonde_softin_dev_fetch_m20(sf._h, m20, 2) == -1
    for name in ("fetch", "fetch_dfm", "fetch_m10", "fetch_drop", "fetch_lms6"):
        with pytest.raises(SondeError):
            getattr(sf, name)()
    assert sf.fetch_rs92() == [] and L.sonde_softin_dev_fetch_rs92(sf._h, None, 2) == -1 and L.sonde_softin_dev_fetch_rs92(None, buf, 2) == -1
    with pytest.raises(SondeError):
        sf.load_rs92_ephemeris(os.path.join(os.path.dirname(rinex), "missing.nav"))
    with pytest.raises(SondeError):
        sf.load_rs92_almanac(rinex)                                                            # (not an almanac)
    assert sf.counts() == dict(frames=0, ecc_ok=0, repaired=0, symbols=0, dropped=0)
    sf.close()


# ---------------------------------------------------------------- 5. auto_rx's pipe
@pytest.fixture(scope="module")
def pipe(rinex):
    """per polarity: (capture, text of `fsk_demod --cs16 -b -20000 -u 20000 -s 2 48000 4800 - - | rs92mod -vx -v --crc --ecc --vel --json --softin -i -e <rinex> --ptu`)"""
    need_ref()
    from tools import synth_rs92 as R
    ref = os.path.join(ROOT, "oracle", "_ref")
    out = {}
    for invert in (False, True):
        x = R.rs92_capture(M.frames()[:4], sr=48000, invert=invert)
        p1 = subprocess.run([os.path.join(ref, "fsk_demod"), "--cs16", "-b", "-20000", "-u", "20000", "-s", "2", "48000", "4800", "-", "-"], input=x.tobytes(),
                            capture_output=True, timeout=300)
        assert p1.returncode == 0
        p2 = subprocess.run([M.REF, "-vx", "-v", "--crc", "--ecc", "--vel", "--json", "--softin", "-i", "-e", rinex, "--ptu"], input=p1.stdout, capture_output=True, timeout=120)
        assert p2.returncode == 0
        out[invert] = (x, p2.stdout.decode())
    return out


def _run_pipe(x, nch, order, rinex):
    """the capture on nch identical channels, a second per call: order "push" (process + push_fsk) or "halves" (the documented order: wait (k - 1), collect (k - 2),
    submit_fsk (k - 1), submit_device (k)) -> per channel the fetched dicts, the counts"""
    import torch
    from radiosonde_auto_rx_amd.fsk import FskModem, SoftinDev
    sr = 48000
    md = FskModem(sr, 4800, n_channels=nch, P=10, lower=-20000, upper=20000)      # (P = 10: fsk_demod's default without -p)
    sf = SoftinDev(nch, kind="rs92", rs92_opts=dict(ptu=1, version="oracle"), ephemeris=rinex)
    X = torch.from_numpy(np.stack([x] * nch)).cuda()
    n = X.shape[1] // 2
    out = {c: [] for c in range(nch)}

    def take():
        for f in sf.fetch_rs92():
            out[f["channel"]].append(f)

    for s0 in range(0, n, sr):
        m = min(sr, n - s0)
        ptr = X.data_ptr() + 2 * s0 * X.element_size()
        if order == "push":
            md.process_device(ptr, n, m); sf.push_fsk(md)
        else:
            if s0 > 0:
                md.wait(); sf.collect(); sf.submit_fsk(md)
            md.submit_device(ptr, n, m)
        take()
    if order != "push":
        md.wait(); sf.collect(); sf.submit_fsk(md); sf.collect(); take()
    cnt = sf.counts()
    md.close(); sf.close()
    return out, cnt


@pytest.mark.parametrize("invert", [False, True], ids=["plain", "inverted"])
def test_rs92_modem_to_text_on_the_device_equals_the_reference_pipe(pipe, rinex, invert):
    x, want = pipe[invert]
    assert sum(want.count('"lat"') for _, want in pipe.values()) >= 3          # one of the two polarities is the one -i decodes
    got, cnt = _run_pipe(x, 2, "halves", rinex)
    text = "".join(f["text"] for f in got[0])
    assert want.startswith(text)
    rest = [l for l in want[len(text):].splitlines() if l.strip()]
    assert len(rest) <= 1                                                       # (the partial frame the reference prints at end of input)
    assert text.count('"lat"') == want.count('"lat"')
    assert [M.full(f) for f in got[1]] == [M.full(f) for f in got[0]] and [f["text"] for f in got[1]] == [f["text"] for f in got[0]]
    assert cnt == _counts(got)
    push, cnt2 = _run_pipe(x, 2, "push", rinex)
    assert cnt2 == cnt
    for c in range(2):
        assert [M.full(f) for f in push[c]] == [M.full(f) for f in got[c]] and [f["text"] for f in push[c]] == [f["text"] for f in got[c]]
