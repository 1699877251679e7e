"""SoftinDev(kind="mrz") — `mp3h1mod --softin [-i] [--auto] [--ofs n]` for many channels on the device (k_softin_mrz = radiosonde_auto_rx_amd/csrc/
sonde_softin_mrz_dev.h compiled by hipcc): the consumer half of auto_rx's pipe `fsk_demod --cs16 -s -b -10000 -u 10000 2 48000 2400 - - | mp3h1mod --auto --json
--softin --ptu`.  Arbiters: the same source under the CPU wave emulator and the host tier sonde_mrz_dec_push_soft on the streams of tests/mrz_softin_cases.py
(everything exact but mv, mv to within one float ulp: the device's double divide and sqrt come ahead of the rounding to float, the allowance the other device
suites give), and the host tier on the modem's own soft decisions behind the real modem."""
import ctypes as C

import numpy as np
import pytest

import mrz_softin_cases as M
from tools import synth

pytestmark = pytest.mark.gpu
GPU_CUTS = [2400, 1000, 251, 43, 44, 45, 65]                # (1- and 2-symbol cuts stay with the emulator: a few hundred launches a test at the most)


@pytest.fixture(scope="module")
def emu():
    return M.load_emu()


@pytest.fixture(scope="module")
def host():
    return M.load_host()


def _mrz_opts(o, **kw):
    d = dict(json=0, ptu=0)
    d.update(M.dec_opts(o))
    d.update(kw)
    return d


def _device(streams, calls, o, opts=None):
    """equally long streams, a channel each, through one consumer in calls of calls[0], calls[1], .. half symbols (the last length repeats): per channel the fetched
    dicts, the consumer's counts"""
    import torch
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    S = np.ascontiguousarray(np.stack(streams), np.float32)
    n = S.shape[1]
    sf = SoftinDev(len(streams), kind="mrz", softinv=o["softinv"], mrz_opts=_mrz_opts(o, **(opts or {})))
    d = torch.from_numpy(S).cuda()
    recs = {c: [] for c in range(len(streams))}
    pos, i = 0, 0
    while pos < n:
        k = min(calls[min(i, len(calls) - 1)], n - pos)
        chunk = d[:, pos:pos + k].contiguous()
        torch.cuda.synchronize()                                 # (the copy runs on PyTorch's stream, the consumer on its own: the chunk must be complete first)
        sf.push_device(chunk.data_ptr(), k, k)
        for f in sf.fetch_mrz():
            recs[f["channel"]].append(f)
        pos += k; i += 1
    cnt = sf.counts()
    sf.close()
    return recs, cnt


def _counts(recs, dropped=0):
    fs = [f for r in recs.values() for f in r]
    return dict(frames=len(fs), ecc_ok=sum(f["crc_ok"] for f in fs), repaired=0, symbols=0, dropped=dropped)


def _same(got, want, o):
    """records of one channel (fetch_mrz dicts) against the emulator's Recs: everything exact but mv, mv within one ulp; the text is the `-r` / `-R` line"""
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert M.key(g) == M.key(w)
        assert M.mv_within_one_ulp(g["mv"], w.mv)
        assert g["text"] == M.raw_line(w, o["ofs"], o["raw2"]) + "\n"


def _padded(ss, o=None):
    """streams brought to one length by more of the idle pattern 0101 .. every stream ends with (no header in it), in the stream's own polarity (a stream's last
    half symbol is a 0)"""
    n = max(len(s) for s in ss)
    return [np.concatenate([s, np.float32(-np.sign(s[-1])) * M.idle(None, n - len(s) + 4)[:n - len(s)]]).astype(np.float32) for s in ss]


# ---------------------------------------------------------------- 1. the emulator's cases on the device, three channels a consumer
def _groups():
    by = {}
    for name, o in sorted(M.case_opts().items()):              # (no stream is built, no library loaded while the module is collected)
        by.setdefault(tuple(sorted((k, str(v)) for k, v in o.items())), []).append(name)
    out = []
    for _, names in sorted(by.items()):
        while len(names) % 3:
            names.append(names[0])                            # (a consumer's third channel: one of its streams again)
        out += [tuple(names[i:i + 3]) for i in range(0, len(names), 3)]
    return out


GROUPS = _groups()
_emu_recs = {}


def _emu_of(emu, nm):
    if nm not in _emu_recs:
        c = M.cases()[nm]
        _emu_recs[nm] = M.emu_frames(emu, c["s"], [len(c["s"])], **M.opts(c))[0]
        assert len(_emu_recs[nm]) == c["n"]
    return _emu_recs[nm]


@pytest.mark.parametrize("names", GROUPS, ids=["-".join(g) for g in GROUPS])
def test_cases_in_one_call_on_three_channels_equal_emulator_and_arbiter(emu, host, names):
    o = M.case_opts()[names[0]]
    streams = _padded([M.cases()[nm]["s"] for nm in names], o)
    recs, cnt = _device(streams, [len(streams[0])], o)
    for c, nm in enumerate(names):
        _same(recs[c], _emu_of(emu, nm), o)
        want = M.host_frames(host, M.cases()[nm]["s"], cache=nm, **M.opts(M.cases()[nm]))
        assert [f["text"] for f in recs[c]] == [w[6] + "\n" for w in want] and len(want) == M.cases()[nm]["n"]
    assert cnt == _counts(recs)


def test_five_channels_under_cuts_equal_one_call(emu):
    names = ["switch_back", "clean_latlon", "sigma03", "ring_behind_frame", "dropped_then_true"]
    o = M.case_opts()[names[0]]
    assert all(M.case_opts()[nm] == o for nm in names)
    streams = _padded([M.cases()[nm]["s"] for nm in names], o)
    one, cnt1 = _device(streams, [len(streams[0])], o)
    for c, nm in enumerate(names):
        _same(one[c], _emu_of(emu, nm), o)
    for cut in GPU_CUTS:
        recs, cnt = _device(streams, [cut], o)
        for c in one:                                            # (the same operations in the same order: mv bit for bit as well)
            assert len(recs[c]) == len(one[c]), (cut, c)
            for g, w in zip(recs[c], one[c]):
                assert g == w, (cut, c, {k: (g[k], w[k]) for k in g if g[k] != w[k] and k != "bytes" and k != "bits"})
        assert cnt == cnt1, cut


def test_auto_flips_once_and_stays_flipped_across_calls(emu):
    o = M.case_opts()["inverted_auto"]
    s = M.cases()["inverted_auto"]["s"]
    recs, _ = _device([s, -s, s], [1000], o)
    _same(recs[0], _emu_of(emu, "inverted_auto"), o)
    assert [f["inv"] for f in recs[0]] == [1, 1] and [f["inv"] for f in recs[1]] == [0, 0] and [f["mv"] for f in recs[1]] == [-f["mv"] for f in recs[0]]
    assert [M.key(f)[3:] for f in recs[1]] == [M.key(f)[3:] for f in recs[0]] == [M.key(f)[3:] for f in recs[2]]


# ---------------------------------------------------------------- 2. the unstaged call and the record buffer
def test_a_call_longer_than_the_staging_buffer(emu, host):
    s = M.long_stream()
    assert len(s) > M.STAGE_MAX
    want = M.host_frames(host, s, cache="long")
    o = M.case_opts()["clean_ecef"]
    recs, cnt = _device([s, np.zeros_like(s), s], [len(s)], o)      # (8 * 3 + 16 = 40 records a call: the 32 fit)
    assert [M.key(f) for f in recs[0]] == [M.key(w) for w in want] == [M.key(f) for f in recs[2]] and len(want) == 16 and recs[1] == []
    assert [f["nbits"] for f in recs[0]] == [408] * 5 + [384] * 11
    assert cnt == _counts(recs) and cnt["ecc_ok"] == 32


def test_record_buffer_overflow_and_the_switch_behind_dropped_frames(host):
    """8 * 1 + 16 = 24 records a call: 30 frames in one call on one channel — 24 ECEF, then six lat / lon — give 24 delivered and 6 dropped, the lat / lon frame
    that switches the length among the dropped; the frame of the next call is read at 384 bits, so the dropped frames were decoded, verdict and switch included.
    26 000 half symbols a call: above the staging limit."""
    rng = np.random.default_rng(24)
    first = M.train(rng, [M.ecef(k) for k in range(24)] + [M.latlon(k) for k in range(24, 30)], lead=9, end=0)
    second = M.train(rng, [M.latlon(31)], lead=60)
    o = M.case_opts()["clean_ecef"]
    recs, cnt = _device([np.concatenate([first, second])], [len(first), len(second)], o)
    want = M.host_frames(host, np.concatenate([first, second]))
    assert len(want) == 31 and [w[1] for w in want] == [408] * 25 + [384] * 6 and len(first) > M.STAGE_MAX
    assert [M.key(f) for f in recs[0]] == [M.key(w) for w in want[:24] + want[30:]]
    assert cnt == _counts(recs, dropped=6) and cnt["frames"] == 25
    assert recs[0][-1]["nbits"] == 384 and recs[0][-1]["crc_ok"] == 1


# ---------------------------------------------------------------- 3. refusals
def test_create_and_fetch_refusals_and_create_destroy_without_a_push():
    from radiosonde_auto_rx_amd.engine import SondeError, SondeFrame, SondeDfmFrame, SondeM10Frame, SondeM20Frame, SONDE_MRZ, SONDE_MTS01
    from radiosonde_auto_rx_amd.family import MrzOpts
    from radiosonde_auto_rx_amd.fsk import SoftinDev, _lib, MeiseiSoftinRec, Imet54SoftinRec, Rs92SoftinRec, Lms6SoftinRec, MrzSoftinRec, Mts01SoftinRec
    from radiosonde_auto_rx_amd.drop import DropFrame
    assert (SONDE_MRZ, SONDE_MTS01) == (31, 71)
    L = _lib()
    h = C.c_void_p()
    assert L.sonde_softin_dev_create(1, SONDE_MRZ, 0, 0, 0, 0, C.byref(h)) == -1                # SONDE_E_ARG: the kind needs its options
    assert L.sonde_softin_dev_create_mrz(0, C.byref(MrzOpts()), 0, C.byref(h)) == -1
    assert L.sonde_softin_dev_create_mrz(1, None, 0, C.byref(h)) == -1
    assert L.sonde_softin_dev_create_mrz(1, C.byref(MrzOpts()), 0, None) == -1
    assert L.sonde_softin_dev_create_mrz(1, C.byref(MrzOpts(bits_ofs=65, bits_ofs_given=1)), 0, C.byref(h)) == -1     # as sonde_mrz_dec_create returns it
    buf = (MrzSoftinRec * 2)()
    for kind in ("rs41", "dfm", "m10", "m20", "drop", "lms6", "rs92", "imet54", "meisei", "mts01"):
        sf = SoftinDev(1, kind=kind)
        assert L.sonde_softin_dev_fetch_mrz(sf._h, buf, 2) == -1
        with pytest.raises(SondeError):
            sf.fetch_mrz()
        sf.close()
    sf = SoftinDev(2, kind="mrz")
    for fn, typ in (("fetch", SondeFrame), ("fetch_dfm", SondeDfmFrame), ("fetch_m10", SondeM10Frame), ("fetch_m20", SondeM20Frame), ("fetch_drop", DropFrame),
                    ("fetch_lms6", Lms6SoftinRec), ("fetch_rs92", Rs92SoftinRec), ("fetch_imet54", Imet54SoftinRec), ("fetch_meisei", MeiseiSoftinRec),
                    ("fetch_mts01", Mts01SoftinRec)):
        other = (typ * 2)()
        assert getattr(L, "sonde_softin_dev_" + fn)(sf._h, other, 2) == -1
        with pytest.raises(SondeError):
            getattr(sf, fn)()
    assert L.sonde_softin_dev_set_m20_skip(sf._h, 0) == -1
    assert sf.fetch_mrz() == [] and L.sonde_softin_dev_fetch_mrz(sf._h, None, 2) == -1 and L.sonde_softin_dev_fetch_mrz(None, buf, 2) == -1
    assert sf.counts() == dict(frames=0, ecc_ok=0, repaired=0, symbols=0, dropped=0)
    sf.close()                                                    # created and destroyed without a push


# ---------------------------------------------------------------- 4. behind the real modem
def test_mrz_capture_behind_the_modem_equals_the_host_tier_on_the_modems_soft_decisions(host):
    """mrz_capture, 3 s, two channels — the second inverted, both with --auto — through sonde_fsk (fsk_demod --cs16 -s -b -10000 -u 10000 2 48000 2400) and the
    consumer in the overlapped order (wait, collect, submit_fsk, submit_device): text and JSON are the host tier's on the soft decisions the modem produced"""
    import torch
    from radiosonde_auto_rx_amd.fsk import FskModem, SoftinDev
    sr = 48000
    x = np.stack([synth.mrz_capture(sr=sr, seconds=3.0, seed=31), synth.mrz_capture(sr=sr, seconds=3.0, seed=32, invert=True)])
    md = FskModem(sr, 2400, n_channels=2, P=10, lower=-10000, upper=10000)
    opts = dict(aut=1, json=1, ptu=1, version="oracle")
    sf = SoftinDev(2, kind="mrz", mrz_opts=opts)
    X = torch.from_numpy(x).cuda()
    n = X.shape[1] // 2
    out, sd = {0: [], 1: []}, {0: [], 1: []}

    def behind():
        md.wait()
        for c in range(2):
            sd[c].append(md.fetch(c)[0].reshape(-1).copy())
        sf.collect(); sf.submit_fsk(md)

    for s0 in range(0, n, sr):
        if s0 > 0:
            behind()
        md.submit_device(X.data_ptr() + 2 * s0 * X.element_size(), n, min(sr, n - s0))
        for f in sf.fetch_mrz():
            out[f["channel"]].append(f)
    behind(); sf.collect()
    for f in sf.fetch_mrz():
        out[f["channel"]].append(f)
    cnt = sf.counts()
    md.close(); sf.close()
    for c in range(2):
        soft = np.concatenate(sd[c])
        text = "".join(f["text"] for f in out[c])
        assert text == M.host_text(host, soft, **opts)
        assert len(out[c]) >= 3 and sum(f["crc_ok"] for f in out[c]) >= 2 and text.count("[OK]") == sum(f["crc_ok"] for f in out[c])
        assert len({f["inv"] for f in out[c]}) == 1                # --auto settles at the first hit
        raw = M.host_text(host, soft, raw=1, aut=1).splitlines()
        assert [M.raw_line(f) for f in out[c]] == raw
    assert out[0][0]["inv"] != out[1][0]["inv"]                    # the second channel is the first one's inverse
    assert cnt == _counts(out) and cnt["dropped"] == 0
