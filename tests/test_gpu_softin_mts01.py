"""SoftinDev(kind="mts01") — `mts01mod --softin` for many channels on the device (k_softin_mts01 = radiosonde_auto_rx_amd/csrc/sonde_softin_mts01_dev.h compiled
by hipcc).  Arbiters: the same source under the CPU wave emulator and the host tier sonde_mts01_dec_push_soft on the streams of tests/mts01_softin_cases.py
(everything exact but mv, mv to within one float ulp: the device's double divide and sqrt come ahead of the rounding to float, the allowance the other device
suites give)."""
import ctypes as C

import numpy as np
import pytest

import mts01_softin_cases as M

pytestmark = pytest.mark.gpu
GPU_CUTS = [2400, 1000, 251, 31, 32, 33, 65]                # (1- and 2-symbol cuts stay with the emulator: a few hundred launches a test at the most)


@pytest.fixture(scope="module")
def emu():
    return M.load_emu()


@pytest.fixture(scope="module")
def host():
    return M.load_host()


def _device(streams, calls, softinv=False, opts=None):
    """equally long streams, a channel each, through one consumer in calls of calls[0], calls[1], .. symbols (the last length repeats): per channel the fetched
    dicts, the consumer's counts"""
    import torch
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    S = np.ascontiguousarray(np.stack(streams), np.float32)
    n = S.shape[1]
    o = dict(raw=1, json=0)
    o.update(opts or {})
    sf = SoftinDev(len(streams), kind="mts01", softinv=softinv, mts01_opts=o)
    d = torch.from_numpy(S).cuda()
    recs = {c: [] for c in range(len(streams))}
    pos, i = 0, 0
    while pos < n:
        k = min(calls[min(i, len(calls) - 1)], n - pos)
        chunk = d[:, pos:pos + k].contiguous()
        torch.cuda.synchronize()                                 # (the copy runs on PyTorch's stream, the consumer on its own: the chunk must be complete first)
        sf.push_device(chunk.data_ptr(), k, k)
        for f in sf.fetch_mts01():
            recs[f["channel"]].append(f)
        pos += k; i += 1
    cnt = sf.counts()
    sf.close()
    return recs, cnt


def _counts(recs, dropped=0):
    fs = [f for r in recs.values() for f in r]
    return dict(frames=len(fs), ecc_ok=sum(f["crc_ok"] for f in fs), repaired=0, symbols=0, dropped=dropped)


def _same(got, want):
    """records of one channel (fetch_mts01 dicts) against the emulator's Recs: everything exact but mv, mv within one ulp; the text is the `-r` line"""
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert M.key(g) == M.key(w)
        assert M.mv_within_one_ulp(g["mv"], w.mv)
        assert g["text"] == M.raw_line(w) + "\n"


def _padded(ss, seed):
    """streams brought to one length by a quiet tail (no header in it: the records stay those of the stream)"""
    rng = np.random.default_rng(seed)
    n = max(len(s) for s in ss)
    return [np.concatenate([s, M.noise(rng, n - len(s), 0.05)]) for s in ss]


# ---------------------------------------------------------------- 1. the emulator's cases on the device, three channels a consumer
def _groups():
    by = {}
    for name, o in sorted(M.case_opts().items()):              # (no stream is built, no library loaded while the module is collected)
        by.setdefault(o, []).append(name)
    out = []
    for k, names in sorted(by.items()):
        while len(names) % 3:
            names.append(names[0])                            # (a consumer's third channel: one of its streams again)
        out += [(k, tuple(names[i:i + 3])) for i in range(0, len(names), 3)]
    return out


GROUPS = _groups()
_emu_recs = {}


def _emu_of(emu, nm):
    if nm not in _emu_recs:
        c = M.cases()[nm]
        _emu_recs[nm] = M.emu_frames(emu, c["s"], [len(c["s"])], c["softinv"])[0]
        assert len(_emu_recs[nm]) == c["n"]
    return _emu_recs[nm]


@pytest.mark.parametrize("group", GROUPS, ids=["-".join(g[1]) for g in GROUPS])
def test_cases_in_one_call_on_three_channels_equal_emulator_and_arbiter(emu, host, group):
    softinv, names = group
    streams = _padded([M.cases()[nm]["s"] for nm in names], 7)
    recs, cnt = _device(streams, [len(streams[0])], softinv)
    for c, nm in enumerate(names):
        _same(recs[c], _emu_of(emu, nm))
        want = M.host_frames(host, M.cases()[nm]["s"], softinv, cache=nm)
        assert [f["text"] for f in recs[c]] == [w[5] + "\n" for w in want] and len(want) == M.cases()[nm]["n"]
    assert cnt == _counts(recs)


def test_five_channels_under_cuts_equal_one_call(emu):
    names = ["clean", "back_to_back", "sigma03", "ring_behind_frame", "inverted"]
    streams = _padded([M.cases()[nm]["s"] for nm in names], 5)
    one, cnt1 = _device(streams, [len(streams[0])])
    for c, nm in enumerate(names):
        _same(one[c], _emu_of(emu, nm))
    for cut in GPU_CUTS:
        recs, cnt = _device(streams, [cut])
        for c in one:                                            # (the same operations in the same order: mv bit for bit as well)
            assert len(recs[c]) == len(one[c]), (cut, c)
            for g, w in zip(recs[c], one[c]):
                assert g == w, (cut, c, {k: (g[k], w[k]) for k in g if g[k] != w[k] and k != "bytes" and k != "bits"})
        assert cnt == cnt1, cut


def test_text_forms_from_the_devices_bytes_equal_the_host_tier(host):
    """default, -v, --json and -R text of three channels: what the host tier prints for the same stream"""
    names = ["clean", "no_nul", "early_nul"]
    streams = _padded([M.cases()[nm]["s"] for nm in names], 3)
    for opts in (dict(raw=0), dict(raw=0, verbose=1), dict(raw=0, json=1, version="oracle"), dict(raw=2)):
        recs, _ = _device(streams, [len(streams[0])], opts=opts)
        for c in range(3):
            assert "".join(f["text"] for f in recs[c]) == M.host_text(host, streams[c], **opts)


# ---------------------------------------------------------------- 2. the unstaged call and the record buffer
def test_a_call_longer_than_the_staging_buffer(host):
    s = M.long_stream()
    assert len(s) > M.STAGE_MAX
    want = M.host_frames(host, s, cache="long")
    z = np.zeros_like(s)
    recs, cnt = _device([s, -s, s, z, z], [len(s)])                # (4 * 5 + 16 = 36 records a call: the 36 fit)
    assert [M.key(f) for f in recs[0]] == [M.key(w) for w in want] == [M.key(f) for f in recs[2]] and len(want) == 12 and recs[3] == recs[4] == []
    assert [f["hdr_bit"] for f in recs[1]] == [w[0] for w in want] and not any(f["crc_ok"] for f in recs[1])
    assert cnt == _counts(recs) and cnt["ecc_ok"] == 2 * sum(w[4] for w in want) >= 10       # (1048 bits at sigma 0.3: some frames fail their CRC)


def test_record_buffer_overflow(host):
    """4 * 1 + 16 = 20 records a call: 23 frames back to back in one call on one channel give 20 delivered and 3 dropped, and the call after it is intact.
    24 840 symbols a call: above the staging limit."""
    rng = np.random.default_rng(20)
    first = M.soft(M.onair([M.fbits(k) for k in range(23)], lead=0, gap=0))
    second = np.concatenate([M.soft(M.onair([M.fbits(23)], lead=0)), M.noise(rng, 80, 0.05)])
    assert len(first) > M.STAGE_MAX
    recs, cnt = _device([np.concatenate([first, second])], [len(first), len(second)])
    want = M.host_frames(host, np.concatenate([first, second]))
    assert len(want) == 24
    assert [M.key(f) for f in recs[0]] == [M.key(w) for w in want[:20] + want[23:]]
    assert cnt == _counts(recs, dropped=3) and cnt["frames"] == 21 and cnt["ecc_ok"] == 21


# ---------------------------------------------------------------- 3. refusals
def test_create_and_fetch_refusals_and_create_destroy_without_a_push():
    from radiosonde_auto_rx_amd.engine import SondeError, SondeFrame, SondeDfmFrame, SondeM10Frame, SondeM20Frame, SONDE_MTS01
    from radiosonde_auto_rx_amd.family import Mts01Opts
    from radiosonde_auto_rx_amd.fsk import SoftinDev, _lib, MeiseiSoftinRec, Imet54SoftinRec, Rs92SoftinRec, Lms6SoftinRec, MrzSoftinRec, Mts01SoftinRec
    from radiosonde_auto_rx_amd.drop import DropFrame
    L = _lib()
    h = C.c_void_p()
    assert L.sonde_softin_dev_create(1, SONDE_MTS01, 0, 0, 0, 0, C.byref(h)) == -1              # SONDE_E_ARG: the kind needs its options
    assert L.sonde_softin_dev_create_mts01(0, C.byref(Mts01Opts()), 0, C.byref(h)) == -1
    assert L.sonde_softin_dev_create_mts01(1, None, 0, C.byref(h)) == -1
    assert L.sonde_softin_dev_create_mts01(1, C.byref(Mts01Opts()), 0, None) == -1
    assert L.sonde_softin_dev_create_mts01(1, C.byref(Mts01Opts(raw=3)), 0, C.byref(h)) == -1     # as sonde_mts01_dec_create returns it
    buf = (Mts01SoftinRec * 2)()
    for kind in ("rs41", "dfm", "m10", "m20", "drop", "lms6", "rs92", "imet54", "meisei", "mrz"):
        sf = SoftinDev(1, kind=kind)
        assert L.sonde_softin_dev_fetch_mts01(sf._h, buf, 2) == -1
        with pytest.raises(SondeError):
            sf.fetch_mts01()
        sf.close()
    sf = SoftinDev(2, kind="mts01")
    for fn, typ in (("fetch", SondeFrame), ("fetch_dfm", SondeDfmFrame), ("fetch_m10", SondeM10Frame), ("fetch_m20", SondeM20Frame), ("fetch_drop", DropFrame),
                    ("fetch_lms6", Lms6SoftinRec), ("fetch_rs92", Rs92SoftinRec), ("fetch_imet54", Imet54SoftinRec), ("fetch_meisei", MeiseiSoftinRec),
                    ("fetch_mrz", MrzSoftinRec)):
        other = (typ * 2)()
        assert getattr(L, "sonde_softin_dev_" + fn)(sf._h, other, 2) == -1
        with pytest.raises(SondeError):
            getattr(sf, fn)()
    assert L.sonde_softin_dev_set_m20_skip(sf._h, 0) == -1
    assert sf.fetch_mts01() == [] and L.sonde_softin_dev_fetch_mts01(sf._h, None, 2) == -1 and L.sonde_softin_dev_fetch_mts01(None, buf, 2) == -1
    assert sf.counts() == dict(frames=0, ecc_ok=0, repaired=0, symbols=0, dropped=0)
    sf.close()                                                    # created and destroyed without a push
