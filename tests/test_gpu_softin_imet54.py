"""SoftinDev(kind="imet54") — `imet54mod --softin [-i] [--auto] [--ecc]` for many channels on the device (k_softin_imet54 = radiosonde_auto_rx_amd/csrc/
sonde_softin_imet54_dev.h compiled by hipcc): the consumer half of auto_rx's pipe `fsk_demod --cs16 -b -10000 -u 10000 -s 2 48000 4800 - - | imet54mod --ecc --json
--softin -i --ptu`.  Arbiters: the compiled reference on the same symbol streams and behind the modem, the host tier sonde_imet54_dec_push_soft, and the same source
under the CPU wave emulator on the streams of tests/imet54_softin_cases.py (everything exact but mv, mv to within one float ulp: the device's double divide and sqrt
come ahead of the rounding to float, the allowance the M20 suite gives)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import imet54_softin_cases as M
from golden_cases import need_ref
from tools import synth

ROOT = M.ROOT
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emu():
    return M.load_emu()


@pytest.fixture(scope="module")
def host():
    return M.load_host()


def _device(streams, calls, softinv=False, opts=None):
    """equally long streams, a channel each, through one consumer in calls of calls[0], calls[1], .. symbols (the last length repeats): per channel the fetched dicts,
    the consumer's counts"""
    import torch
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    S = np.ascontiguousarray(np.stack(streams), np.float32)
    n = S.shape[1]
    o = dict(raw=1, ecc=1, json=0, ptu=0, inv=0)
    o.update(opts or {})
    sf = SoftinDev(len(streams), kind="imet54", softinv=softinv, imet54_opts=o)
    d = torch.from_numpy(S).cuda()
    recs = {c: [] for c in range(len(streams))}
    pos, i = 0, 0
    while pos < n:
        k = min(calls[min(i, len(calls) - 1)], n - pos)
        chunk = d[:, pos:pos + k].contiguous()
        sf.push_device(chunk.data_ptr(), k, k)
        for f in sf.fetch_imet54():
            recs[f["channel"]].append(f)
        pos += k; i += 1
    cnt = sf.counts()
    sf.close()
    return recs, cnt


def _counts(recs, dropped=0):
    """the tallies the fetched records imply (frames = delivered ones; accepted = the JSON rule without the status bits)"""
    fs = [f for r in recs.values() for f in r]
    return dict(frames=len(fs), ecc_ok=sum((f["ecc_frm"] >= 0 and f["crc"] != 0) or f["ecc_std"] == 0 for f in fs), repaired=sum(f["ecc_frm"] > 0 for f in fs),
                symbols=sum(f["ecc_frm"] for f in fs if f["ecc_frm"] > 0), dropped=dropped)


def _same(got, want, ecc=1):
    """records of one channel (fetch_imet54 dicts) against the emulator's Recs: everything exact but mv, mv within one ulp"""
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert M.key(g) == M.key(w)
        assert g["crc"] == (1 if w.crc_std else 2 if w.crc_cont else 0)
        assert M.mv_within_one_ulp(g["mv"], w.mv)
        assert g["text"] == M.raw_line(w, ecc) + "\n"


def _mixed_calls(n, seed):
    """different lengths call after call: a dozen of the short cuts, then one of the long ones"""
    rng = np.random.default_rng(seed)
    short, long_ = [c for c in M.CUTS if c < 100], [c for c in M.CUTS if c >= 100]
    out, tot = [], 0
    while tot < n:
        out += [int(v) for v in rng.choice(short, 12)] + [int(rng.choice(long_))]
        tot = sum(out)
    return out


def _padded(ss, seed):
    """streams brought to one length by a quiet tail (no header in it: the records stay those of the stream)"""
    rng = np.random.default_rng(seed)
    n = max(len(s) for s in ss)
    return [np.concatenate([s, M.noise(rng, n - len(s), 0.05)]) for s in ss]


# ---------------------------------------------------------------- 1. three channels under random call cuts against the compiled reference and the host tier
def _flight(seed, polarity):
    """three frames — jittered amplitudes, 0 .. 2 flipped bits in every codeword of the second, sigma 0.2 on the third — with random gaps; polarity +1 / -1 per frame"""
    rng = np.random.default_rng(seed)
    parts = [M.noise(rng, int(rng.integers(5, 90)), 0.05)]
    for k in range(3):
        bits = M.damaged_bits(seed + k, rng, 2, check=("std", "cont", "none")[(seed + k) % 3]) if k == 1 else M.fbits(M.frame(seed + k, check=("std", "cont")[k % 2]))
        s = M.soft(M.onair(bits, pre=int(rng.integers(0, 60)), idle=int(rng.integers(0, 50))), rng, (0.7, 1.3))
        if k == 2:
            s = s + M.noise(rng, len(s), 0.2)
        parts += [np.float32(polarity[k]) * s, M.noise(rng, int(rng.integers(41, 120)), 0.05)]
    return np.concatenate(parts)


FLIGHTS = {"-r --ecc": (dict(raw=1, ecc=1), ["-r", "--ecc"], (1, 1, 1)),
           "--json --ptu -i": (dict(raw=0, ecc=0, json=1, ptu=1, inv=1, version="oracle"), ["--json", "--ptu", "-i"], (-1, -1, -1)),
           "--auto": (dict(raw=0, ecc=0, aut=1), ["--auto"], (1, -1, -1))}


@pytest.mark.parametrize("name", sorted(FLIGHTS))
def test_three_channels_under_random_cuts_equal_reference_and_host_tier(host, name):
    need_ref()
    opts, args, pol = FLIGHTS[name]
    streams = _padded([_flight(100 * (1 + sorted(FLIGHTS).index(name)) + 10 * c, pol) for c in range(3)], 3)
    n = len(streams[0])
    recs, cnt = _device(streams, M.random_cuts(n, 77 + len(name), 1, 3000), opts=opts)
    nframes = 0
    for c in range(3):
        r = subprocess.run([M.REF, "--softin"] + args, input=streams[c].tobytes(), capture_output=True, timeout=120)
        assert r.returncode == 0
        text = "".join(f["text"] for f in recs[c])
        assert text.splitlines() == r.stdout.decode().splitlines()
        o = dict(opts); inv = o.pop("inv", 0)
        assert text == M.host_text(host, streams[c], inv, **o)
        nframes += len(recs[c])
    assert nframes >= 8                                          # (a damaged header may cost a frame; the reference says which)
    assert cnt == _counts(recs)


# ---------------------------------------------------------------- 2. the emulator's cases on the device, three channels a consumer
def _groups():
    by = {}
    for name, o in sorted(M.case_opts().items()):              # (no stream is built, no library loaded while the module is collected)
        by.setdefault(o, []).append(name)
    out = []
    for k, names in sorted(by.items()):
        while len(names) % 3:
            names.append(names[0])                            # (a consumer's third channel: one of its streams again)
        out += [k + (tuple(names[i:i + 3]),) for i in range(0, len(names), 3)]
    return out


GROUPS = _groups()
_emu_recs = {}


@pytest.mark.parametrize("group", GROUPS, ids=["-".join(g[4]) for g in GROUPS])
def test_cases_on_the_device_equal_the_emulator(emu, group):
    """threshold, ring, polarity, Hamming-bound and check-sum inputs: in one call and under mixed cuts"""
    inv, softinv, aut, ecc, names = group
    streams = _padded([M.cases()[nm]["s"] for nm in names], 7)
    n = len(streams[0])
    for calls in ([n], _mixed_calls(n, 31 + GROUPS.index(group))):
        recs, cnt = _device(streams, calls, softinv, opts=dict(inv=inv, aut=aut, ecc=ecc))
        for c, nm in enumerate(names):
            if nm not in _emu_recs:
                case = M.cases()[nm]
                _emu_recs[nm] = M.emu_frames(emu, case["s"], [len(case["s"])], inv, softinv, aut, ecc)[0]
            assert len(_emu_recs[nm]) == M.cases()[nm]["n"]
            _same(recs[c], _emu_recs[nm], ecc)
        assert cnt == _counts(recs)


# ---------------------------------------------------------------- 3. channel indexing
def test_130_channels_in_one_launch_each_with_its_own_lead():
    rng = np.random.default_rng(130)
    nch = 130
    frames = [M.frame(c, sn=54000000 + c) for c in range(nch)]
    n = nch - 1 + 20 + 40 + M.NSYM + 70
    streams = []
    for c in range(nch):
        s = np.concatenate([M.noise(rng, c, 0.05), M.soft(M.onair(M.fbits(frames[c]), pre=20, idle=0), rng, (0.8, 1.2))])
        streams.append(np.concatenate([s, M.noise(rng, n - len(s), 0.05)]))
    recs, cnt = _device(streams, [n])
    for c in range(nch):
        assert len(recs[c]) == 1
        f = recs[c][0]
        assert (f["hdr_bit"], f["frame"], f["ecc_frm"], f["crc"]) == (c + 60, frames[c], 0, 1)
        assert f["text"] == frames[c].hex().upper() + " [OK]\n"
    assert len({r[0]["frame"] for r in recs.values()}) == nch
    assert cnt == dict(frames=nch, ecc_ok=nch, repaired=0, symbols=0, dropped=0)


# ---------------------------------------------------------------- 4. the record buffer
def test_record_buffer_overflow_with_two_channels():
    """4 * 2 + 16 = 24 records a call: 13 frames back to back on both channels give 24 delivered and 2 dropped (which two is the order the waves finished in); each
    channel's records are the first of its frames in order, and the call after it is intact"""
    rng = np.random.default_rng(24)
    frames = [[M.frame(50 * c + k, sn=54000100 + c) for k in range(14)] for c in range(2)]
    first = [np.concatenate([M.soft(M.onair(M.fbits(f), pre=0, idle=0)) for f in frames[c][:13]]) for c in range(2)]
    last = [np.concatenate([M.soft(M.onair(M.fbits(frames[c][13]), pre=0, idle=0)), M.noise(rng, 80, 0.05)]) for c in range(2)]
    streams = [np.concatenate([first[c], last[c]]) for c in range(2)]
    recs, cnt = _device(streams, [len(first[0]), len(last[0])])
    assert sum(len(r) for r in recs.values()) == 24 + 2 and cnt["dropped"] == 2 and cnt["frames"] == 26
    for c in range(2):
        got = [f["frame"] for f in recs[c]]
        k = len(got) - 1
        assert 11 <= k <= 13 and got[:k] == frames[c][:k] and got[k] == frames[c][13]
        assert [f["hdr_bit"] for f in recs[c]] == [40 + 2240 * i for i in range(k)] + [40 + 2240 * 13]
    assert cnt == _counts(recs, dropped=2)


# ---------------------------------------------------------------- 5. refusals
def test_create_and_fetch_refusals():
    from radiosonde_auto_rx_amd.engine import SondeError, SondeFrame, SondeDfmFrame, SondeM10Frame, SondeM20Frame, SONDE_IMET54
    from radiosonde_auto_rx_amd.family import Imet54Opts
    from radiosonde_auto_rx_amd.fsk import SoftinDev, _lib, Imet54SoftinRec, Rs92SoftinRec, Lms6SoftinRec
    from radiosonde_auto_rx_amd.drop import DropFrame
    L = _lib()
    h = C.c_void_p()
    assert L.sonde_softin_dev_create(1, SONDE_IMET54, 0, 0, 0, 0, C.byref(h)) == -1             # SONDE_E_ARG: the kind needs its options
    o = Imet54Opts(raw=2)
    assert L.sonde_softin_dev_create_imet54(1, C.byref(o), 0, C.byref(h)) == -1                 # as sonde_imet54_dec_create refuses it
    assert L.sonde_softin_dev_create_imet54(0, C.byref(Imet54Opts()), 0, C.byref(h)) == -1
    assert L.sonde_softin_dev_create_imet54(1, None, 0, C.byref(h)) == -1
    assert L.sonde_softin_dev_create_imet54(1, C.byref(Imet54Opts()), 0, None) == -1
    with pytest.raises(SondeError):
        SoftinDev(1, kind="imet54", imet54_opts=dict(raw=3))
    buf = (Imet54SoftinRec * 2)()
    for kind in ("rs41", "dfm", "m10", "m20", "drop", "lms6", "rs92"):
        sf = SoftinDev(1, kind=kind)
        assert L.sonde_softin_dev_fetch_imet54(sf._h, buf, 2) == -1
        with pytest.raises(SondeError):
            sf.fetch_imet54()
        sf.close()
    sf = SoftinDev(2, kind="imet54")
    for fn, typ in (("fetch", SondeFrame), ("fetch_dfm", SondeDfmFrame), ("fetch_m10", SondeM10Frame), ("fetch_m20", SondeM20Frame), ("fetch_drop", DropFrame),
                    ("fetch_lms6", Lms6SoftinRec), ("fetch_rs92", Rs92SoftinRec)):
        other = (typ * 2)()
        assert getattr(L, "sonde_softin_dev_" + fn)(sf._h, other, 2) == -1
        with pytest.raises(SondeError):
            getattr(sf, fn)()
    assert L.sonde_softin_dev_set_m20_skip(sf._h, 0) == -1
    assert sf.fetch_imet54() == [] and L.sonde_softin_dev_fetch_imet54(sf._h, None, 2) == -1 and L.sonde_softin_dev_fetch_imet54(None, buf, 2) == -1
    assert sf.counts() == dict(frames=0, ecc_ok=0, repaired=0, symbols=0, dropped=0)
    sf.close()


# ---------------------------------------------------------------- 6. auto_rx's pipe
@pytest.fixture(scope="module")
def pipe():
    """(capture, text of `fsk_demod --cs16 -b -10000 -u 10000 -s 2 48000 4800 - - | imet54mod --ecc --json --softin -i --ptu`)"""
    need_ref()
    ref = os.path.join(ROOT, "oracle", "_ref")
    x = synth.imet54_capture(sr=48000, seconds=5.5, noise_sigma=0.05, seed=82)
    p1 = subprocess.run([os.path.join(ref, "fsk_demod"), "--cs16", "-b", "-10000", "-u", "10000", "-s", "2", "48000", "4800", "-", "-"], input=x.tobytes(),
                        capture_output=True, timeout=300)
    assert p1.returncode == 0
    p2 = subprocess.run([M.REF, "--ecc", "--json", "--softin", "-i", "--ptu"], input=p1.stdout, capture_output=True, timeout=120)
    assert p2.returncode == 0
    return x, p2.stdout.decode()


def _run_pipe(x, nch, order):
    """the capture on nch identical channels, a second per call: order "push" (process + push_fsk), "halves" (wait, collect, submit_fsk, submit_device) or "behind"
    (wait, submit_device, collect, submit_fsk_behind) -> per channel the fetched dicts, the counts"""
    import torch
    from radiosonde_auto_rx_amd.fsk import FskModem, SoftinDev
    sr = 48000
    md = FskModem(sr, 4800, n_channels=nch, P=10, lower=-10000, upper=10000)      # (P = 10: fsk_demod's default without -p)
    sf = SoftinDev(nch, kind="imet54", imet54_opts=dict(version="oracle"))
    X = torch.from_numpy(np.stack([x] * nch)).cuda()
    n = X.shape[1] // 2
    out = {c: [] for c in range(nch)}

    def take():
        for f in sf.fetch_imet54():
            out[f["channel"]].append(f)

    for s0 in range(0, n, sr):
        m = min(sr, n - s0)
        ptr = X.data_ptr() + 2 * s0 * X.element_size()
        if order == "push":
            md.process_device(ptr, n, m); sf.push_fsk(md)
        elif order == "halves":
            if s0 > 0:
                md.wait(); sf.collect(); sf.submit_fsk(md)
            md.submit_device(ptr, n, m)
        else:
            if s0 > 0:
                md.wait()
            md.submit_device(ptr, n, m)
            if s0 > 0:
                sf.collect(); sf.submit_fsk_behind(md)
        take()
    if order == "halves":
        md.wait(); sf.collect(); sf.submit_fsk(md); sf.collect(); take()
    elif order == "behind":
        md.wait(); sf.collect(); sf.submit_fsk_behind(md); sf.collect(); take()
    cnt = sf.counts()
    md.close(); sf.close()
    return out, cnt


def _rec(f):
    return (f["hdr_bit"], f["frame"], f["ecc_frm"], f["ecc_tlm"], f["ecc_std"], f["crc"], f["mv"], f["text"])


@pytest.mark.parametrize("order", ["halves", "behind"])
def test_imet54_modem_to_text_on_the_device_equals_the_reference_pipe(pipe, order):
    x, want = pipe
    assert want.count('"type": "IMET5"') >= 3
    got, cnt = _run_pipe(x, 2, order)
    text = "".join(f["text"] for f in got[0])
    assert want.startswith(text)
    rest = [l for l in want[len(text):].splitlines() if l.strip()]
    assert len(rest) <= 2                                        # (the partial frame the reference prints at end of input: a line, or a line and its JSON)
    assert text.count('"type": "IMET5"') >= 3
    assert [_rec(f) for f in got[1]] == [_rec(f) for f in got[0]]
    assert cnt == _counts(got) and cnt["dropped"] == 0


def test_pipelined_order_with_a_channel_the_modem_repeats(pipe, monkeypatch, capfd):
    """test hook SONDE_FSK_TEST_ABORT: channel 1 gives up in every launch — the modem's wait repeats it before the consumer reads"""
    x = pipe[0]
    plain, cnt0 = _run_pipe(x, 2, "push")
    capfd.readouterr()
    monkeypatch.setenv("SONDE_FSK_TEST_ABORT", "1")
    got, cnt = _run_pipe(x, 2, "behind")
    assert "repeating them frame by frame" in capfd.readouterr().err
    assert len(plain[0]) >= 3 and cnt == cnt0
    for c in range(2):
        assert [_rec(f) for f in got[c]] == [_rec(f) for f in plain[c]] == [_rec(f) for f in plain[0]]
