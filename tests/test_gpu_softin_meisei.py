"""SoftinDev(kind="meisei") — `meisei100mod --softin [--ecc]` for many channels on the device (k_softin_meisei = radiosonde_auto_rx_amd/csrc/
sonde_softin_meisei_dev.h compiled by hipcc): the consumer half of auto_rx's pipe `fsk_demod --cs16 -s -b -15000 -u 15000 2 48000 2400 - - | meisei100mod --softin
--json --ptu --ecc`.  Arbiters: the compiled reference on the same half-symbol streams and behind the modem, the host tier sonde_meisei_dec_push_soft, and the same
source under the CPU wave emulator on the streams of tests/meisei_softin_cases.py (everything exact but mv, mv to within one float ulp: the device's double divide
and sqrt come ahead of the rounding to float, the allowance the M20 suite gives)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import meisei_softin_cases as M
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
    """equally long streams, a channel each, through one consumer in calls of calls[0], calls[1], .. half symbols (the last length repeats): per channel the fetched
    dicts, the consumer's counts"""
    import torch
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    S = np.ascontiguousarray(np.stack(streams), np.float32)
    n = S.shape[1]
    o = dict(raw=1, ecc=1, verbose=1, json=0, ptu=0)
    o.update(opts or {})
    sf = SoftinDev(len(streams), kind="meisei", softinv=softinv, meisei_opts=o)
    d = torch.from_numpy(S).cuda()
    recs = {c: [] for c in range(len(streams))}
    pos, i = 0, 0
    while pos < n:
        k = min(calls[min(i, len(calls) - 1)], n - pos)
        chunk = d[:, pos:pos + k].contiguous()
        sf.push_device(chunk.data_ptr(), k, k)
        for f in sf.fetch_meisei():
            recs[f["channel"]].append(f)
        pos += k; i += 1
    cnt = sf.counts()
    sf.close()
    return recs, cnt


def _counts(recs, dropped=0):
    """the tallies the fetched records imply (frames = delivered ones; accepted = no block 0xE / 0xF; repaired = any block 1 or 2; symbols = corrected bits)"""
    fs = [f for r in recs.values() for f in r]
    for f in fs:
        assert f["err_frm"] == sum(e >= 0xE for e in f["block_err"]) and f["err_blks"] == sum(e != 0 for e in f["block_err"])
    return dict(frames=len(fs), ecc_ok=sum(f["err_frm"] == 0 for f in fs), repaired=sum(any(e in (1, 2) for e in f["block_err"]) for f in fs),
                symbols=sum(e for f in fs for e in f["block_err"] if e < 0xE), dropped=dropped)


def _same(got, want, ecc=1):
    """records of one channel (fetch_meisei dicts) against the emulator's Recs: everything exact but mv, mv within one ulp"""
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert M.key(g) == M.key(w)
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


def _ref_lines(args, s):
    r = subprocess.run([M.REF] + args, input=np.ascontiguousarray(s, np.float32).tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0
    return r.stdout.decode()


# ---------------------------------------------------------------- 1. three channels under random call cuts against the compiled reference and the host tier
def _flight(seed, variant, polarity):
    """five continuous frames behind a random lead — jittered amplitudes, one or two flipped bits in some blocks of the second, five in one block of the third,
    sigma 0.2 on the fourth — the whole stream in one polarity"""
    rng = np.random.default_rng(seed)
    s = M.soft(M.fsym(seed % 50, variant, 5), rng, (0.7, 1.3))
    for blk in rng.choice(12, 5, replace=False):
        for j in rng.choice(46, int(rng.integers(1, 3)), replace=False):
            s[1200 * 1 + 2 * (M.block_at(int(blk)) + int(j))] *= -1
    for j in rng.choice(46, 5, replace=False):
        s[1200 * 2 + 2 * (M.block_at(seed % 12) + int(j)) + 1] *= -1
    s[3600:4800] += M.noise(rng, 1200, 0.2)
    return np.float32(polarity) * np.concatenate([M.noise(rng, int(rng.integers(5, 90)), 0.05), s, M.noise(rng, int(rng.integers(50, 120)), 0.05)])


FLIGHTS = {"-r --ecc -v": (dict(raw=1, ecc=1, verbose=1), ["-r", "--ecc", "-v"]),
           "--json --ptu --ecc": (dict(raw=0, verbose=0, json=1, ptu=1, ecc=1, version="oracle"), ["--json", "--ptu", "--ecc"])}


@pytest.mark.parametrize("name", sorted(FLIGHTS))
def test_three_channels_under_random_cuts_equal_reference_and_host_tier(host, name):
    need_ref()
    opts, args = FLIGHTS[name]
    k = sorted(FLIGHTS).index(name)
    streams = _padded([_flight(100 * (1 + k) + 10 * c, ("ims100", "rs11g", "ims100")[c], (1, 1, -1)[c]) for c in range(3)], 3)
    n = len(streams[0])
    recs, cnt = _device(streams, M.random_cuts(n, 77 + len(name), 1, 3000), opts=opts)
    for c in range(3):
        text = "".join(f["text"] for f in recs[c])
        ref = _ref_lines(["--softin"] + args, streams[c])
        assert ref == text + "\n"                                # (the newline the reference prints before it exits)
        assert text == M.host_text(host, streams[c], **opts)
        assert len(recs[c]) == 5
    seen = set(e for r in recs.values() for f in r for e in f["block_err"])
    assert {0, 1, 2} <= seen and (0xE in seen or 0xF in seen)
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


@pytest.mark.parametrize("group", GROUPS, ids=["-".join(g[2]) for g in GROUPS])
def test_cases_on_the_device_equal_the_emulator(emu, group):
    """threshold, ring, polarity, zero and BCH inputs: in one call and under mixed cuts"""
    softinv, ecc, names = group
    streams = _padded([M.cases()[nm]["s"] for nm in names], 7)
    n = len(streams[0])
    for calls in ([n], _mixed_calls(n, 31 + GROUPS.index(group))):
        recs, cnt = _device(streams, calls, softinv, opts=dict(ecc=ecc))
        for c, nm in enumerate(names):
            if nm not in _emu_recs:
                case = M.cases()[nm]
                _emu_recs[nm] = M.emu_frames(emu, case["s"], [len(case["s"])], softinv, ecc)[0]
            assert len(_emu_recs[nm]) == M.cases()[nm]["n"]
            _same(recs[c], _emu_recs[nm], ecc)
        assert cnt == _counts(recs)


# ---------------------------------------------------------------- 3. channel indexing and every alignment
def test_130_channels_in_one_launch_each_with_its_own_lead(host):
    """the same two frames behind leads of 0 .. 129 half symbols: more than two waves' worth of channels, every alignment of the header against a round of 64
    positions and against a bit pair"""
    rng = np.random.default_rng(130)
    nch = 130
    body = M.soft(M.fsym(3, "ims100", 2), rng, (0.8, 1.2))
    n = nch - 1 + len(body) + 70
    streams = []
    for c in range(nch):
        s = np.concatenate([M.noise(rng, c, 0.05), body])
        streams.append(np.concatenate([s, M.noise(rng, n - len(s), 0.05)]))
    want = M.host_frames(host, streams[0])
    assert [w[0] for w in want] == [48, 1248]
    recs, cnt = _device(streams, [n])
    for c in range(nch):
        assert [(f["hdr_bit"], f["bits"], f["block_err"]) for f in recs[c]] == [(w[0] + c, w[1], w[2]) for w in want], c
        assert [f["text"] for f in recs[c]] == [w[3] + "\n" for w in want]
    assert cnt == dict(frames=2 * nch, ecc_ok=2 * nch, repaired=0, symbols=0, dropped=0)


# ---------------------------------------------------------------- 4. the record buffer
def test_record_buffer_overflow_with_two_channels(host):
    """4 * 2 + 16 = 24 records a call: 13 frames back to back on both channels give 24 delivered and 2 dropped (which two is the order the waves finished in); each
    channel's records are the first of its frames in order, and the call after it is intact.  15 600 half symbols a call: above the staging limit."""
    rng = np.random.default_rng(24)
    first = [M.soft(M.fsym(50 * c, ("ims100", "rs11g")[c], 13)) for c in range(2)]
    last = [np.concatenate([M.soft(M.fsym(50 * c + 13, ("ims100", "rs11g")[c], 1)), M.noise(rng, 80, 0.05)]) for c in range(2)]
    streams = [np.concatenate([first[c], last[c]]) for c in range(2)]
    assert len(first[0]) > M.STAGE_MAX
    recs, cnt = _device(streams, [len(first[0]), len(last[0])])
    assert sum(len(r) for r in recs.values()) == 24 + 2 and cnt["dropped"] == 2 and cnt["frames"] == 26
    for c in range(2):
        want = M.host_frames(host, streams[c])
        assert len(want) == 14
        got = [M.key(f) for f in recs[c]]
        k = len(got) - 1
        assert 11 <= k <= 13 and got[:k] == [M.key(w) for w in want[:k]] and got[k] == M.key(want[13])
        assert [f["hdr_bit"] for f in recs[c]] == [48 + 1200 * i for i in range(k)] + [48 + 1200 * 13]
    assert cnt == _counts(recs, dropped=2)


# ---------------------------------------------------------------- 5. every syndrome through the kernel
def test_4096_syndromes_of_one_message_as_frames_on_6_channels(emu, host):
    """342 frames of 12 blocks, 57 a channel, six frames a call and channel (36 records a call against 40 slots): verdicts and bits equal the emulator's"""
    frames = M.sweep_frames(M.syndrome_blocks(host, M.bch_messages()[5]))
    assert frames.shape == (342, 600)
    per = 57
    streams = [np.concatenate([M.soft(M.sym_of_bits(frames[per * c + i])) for i in range(per)] + [np.zeros(60, np.float32)]) for c in range(6)]
    recs, cnt = _device(streams, [7200])
    classes = set()
    for c in range(6):
        assert len(recs[c]) == per
        for i, f in enumerate(recs[c]):
            r = M.Rec()
            assert emu.emu_meisei_end(M.pack(frames[per * c + i]), 1, C.byref(r)) == 0
            assert (f["bits"], f["block_err"]) == (bytes(r.bits), bytes(r.block_err)), (c, i)
            classes |= set(f["block_err"])
    assert classes == {0, 1, 2, 0xE, 0xF}
    assert cnt == _counts(recs)


# ---------------------------------------------------------------- 6. refusals
def test_create_and_fetch_refusals():
    from radiosonde_auto_rx_amd.engine import SondeError, SondeFrame, SondeDfmFrame, SondeM10Frame, SondeM20Frame, SONDE_MEISEI
    from radiosonde_auto_rx_amd.family import MeiseiOpts
    from radiosonde_auto_rx_amd.fsk import SoftinDev, _lib, MeiseiSoftinRec, Imet54SoftinRec, Rs92SoftinRec, Lms6SoftinRec
    from radiosonde_auto_rx_amd.drop import DropFrame
    assert SONDE_MEISEI == 11
    L = _lib()
    h = C.c_void_p()
    assert L.sonde_softin_dev_create(1, SONDE_MEISEI, 0, 0, 0, 0, C.byref(h)) == -1             # SONDE_E_ARG: the kind needs its options
    assert L.sonde_softin_dev_create_meisei(0, C.byref(MeiseiOpts()), 0, C.byref(h)) == -1
    assert L.sonde_softin_dev_create_meisei(1, None, 0, C.byref(h)) == -1
    assert L.sonde_softin_dev_create_meisei(1, C.byref(MeiseiOpts()), 0, None) == -1
    buf = (MeiseiSoftinRec * 2)()
    for kind in ("rs41", "dfm", "m10", "m20", "drop", "lms6", "rs92", "imet54"):
        sf = SoftinDev(1, kind=kind)
        assert L.sonde_softin_dev_fetch_meisei(sf._h, buf, 2) == -1
        with pytest.raises(SondeError):
            sf.fetch_meisei()
        sf.close()
    sf = SoftinDev(2, kind="meisei")
    for fn, typ in (("fetch", SondeFrame), ("fetch_dfm", SondeDfmFrame), ("fetch_m10", SondeM10Frame), ("fetch_m20", SondeM20Frame), ("fetch_drop", DropFrame),
                    ("fetch_lms6", Lms6SoftinRec), ("fetch_rs92", Rs92SoftinRec), ("fetch_imet54", Imet54SoftinRec)):
        other = (typ * 2)()
        assert getattr(L, "sonde_softin_dev_" + fn)(sf._h, other, 2) == -1
        with pytest.raises(SondeError):
            getattr(sf, fn)()
    assert L.sonde_softin_dev_set_m20_skip(sf._h, 0) == -1
    assert sf.fetch_meisei() == [] and L.sonde_softin_dev_fetch_meisei(sf._h, None, 2) == -1 and L.sonde_softin_dev_fetch_meisei(None, buf, 2) == -1
    assert sf.counts() == dict(frames=0, ecc_ok=0, repaired=0, symbols=0, dropped=0)
    sf.close()


# ---------------------------------------------------------------- 7. auto_rx's pipe
NOISE = 0.05                                               # tests/test_meisei_pipe_reference.py: the reference pipe alone decodes every frame at this figure


def _capture(variant):
    return synth.meisei_capture(sr=48000, noise_sigma=NOISE, variant=variant, seed=82 if variant == "ims100" else 83)


def _ref_pipe(x):
    ref = os.path.join(ROOT, "oracle", "_ref")
    p1 = subprocess.run([os.path.join(ref, "fsk_demod"), "--cs16", "-s", "-b", "-15000", "-u", "15000", "2", "48000", "2400", "-", "-"], input=x.tobytes(),
                        capture_output=True, timeout=300)
    assert p1.returncode == 0
    p2 = subprocess.run([M.REF, "--softin", "--json", "--ptu", "--ecc"], input=p1.stdout, capture_output=True, timeout=120)
    assert p2.returncode == 0
    return p2.stdout.decode()


_pipes = {}


def _pipe(variant):
    """(capture, text of `fsk_demod --cs16 -s -b -15000 -u 15000 2 48000 2400 - - | meisei100mod --softin --json --ptu --ecc`)"""
    need_ref()
    if variant not in _pipes:
        x = _capture(variant)
        _pipes[variant] = (x, _ref_pipe(x))
    return _pipes[variant]


def _run_pipe(x, nch, order):
    """the capture on nch identical channels, a second per call: order "push" (process + push_fsk), "halves" (wait, collect, submit_fsk, submit_device) or "behind"
    (wait, submit_device, collect, submit_fsk_behind) -> per channel the fetched dicts, the counts"""
    import torch
    from radiosonde_auto_rx_amd.fsk import FskModem, SoftinDev
    sr = 48000
    md = FskModem(sr, 2400, n_channels=nch, P=10, lower=-15000, upper=15000)      # (P = 10: fsk_demod's default without -p)
    sf = SoftinDev(nch, kind="meisei", meisei_opts=dict(version="oracle"))     # (the compiled reference names itself "oracle")
    X = torch.from_numpy(np.stack([x] * nch)).cuda()
    n = X.shape[1] // 2
    out = {c: [] for c in range(nch)}

    def take():
        for f in sf.fetch_meisei():
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
    return (f["hdr_bit"], f["bits"], f["block_err"], f["mv"], f["text"])


def _lines(text):
    return [l for l in text.splitlines() if l.strip()]


@pytest.mark.parametrize("variant,order", [("ims100", "push"), ("ims100", "halves"), ("rs11g", "behind")])
def test_meisei_modem_to_text_on_the_device_equals_the_reference_pipe(variant, order):
    x, want = _pipe(variant)
    got, cnt = _run_pipe(x, 2, order)
    text = "".join(f["text"] for f in got[0])
    assert want == text + "\n"                                   # every line, none left out; the reference adds a newline before it exits
    assert text.count('"type": "MEISEI"') >= 4
    assert [_rec(f) for f in got[1]] == [_rec(f) for f in got[0]]
    assert cnt == _counts(got) and cnt["dropped"] == 0


def test_pipelined_order_with_a_channel_the_modem_repeats(monkeypatch, capfd):
    """test hook SONDE_FSK_TEST_ABORT: channel 1 gives up in every launch — the modem's wait repeats it before the consumer reads"""
    x, want = _pipe("ims100")
    plain, cnt0 = _run_pipe(x, 2, "push")
    capfd.readouterr()
    monkeypatch.setenv("SONDE_FSK_TEST_ABORT", "1")
    got, cnt = _run_pipe(x, 2, "behind")
    assert "repeating them frame by frame" in capfd.readouterr().err
    assert len(plain[0]) >= 8 and cnt == cnt0
    for c in range(2):
        assert [_rec(f) for f in got[c]] == [_rec(f) for f in plain[c]] == [_rec(f) for f in plain[0]]
    assert "".join(f["text"] for f in got[1]) + "\n" == want
