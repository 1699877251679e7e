"""SoftinDev(kind="m20") — `m20mod --softin` for many channels on the device (k_softin_m20 = radiosonde_auto_rx_amd/csrc/sonde_softin_mxx_dev.h compiled by hipcc): the
consumer half of auto_rx's pipe `fsk_demod --cs16 -b -10000 -u 10000 -s -p 5 2 48000 9600 - - | m20mod --json --ptu -vvv --softin -i`.  Arbiters: the compiled reference
(oracle/_ref/m20mod --softin, fsk_demod), the host framer (sonde_softin_create(SONDE_M20) ...) and the same source under the CPU wave emulator on the inputs of
tests/test_softin_m20_emu.py (tests/m20_softin_cases.py).  nbits, len, cs_ok, cs_calc, blk_ok, fw, mv_pos and the frame bytes agree exactly, and with them the found /
not-found decision; mv to within one float ulp (the device's double divide and sqrt ahead of the rounding to float).

Length bytes from 0x80 up cannot come out of a symbol stream (tests/test_softin_m20_emu.py says why): their clamp is checked under the emulator only."""
import os
import subprocess

import numpy as np
import pytest

import m20_softin_cases as M
from golden_cases import need_ref

ROOT = M.ROOT
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emu():
    return M.load_emu()


@pytest.fixture(scope="module")
def host():
    return M.load_host()


def _same(got, want):
    """records of one channel against the arbiter's: everything exact but mv, mv within one ulp"""
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert M.rec_no_mv(g) == M.rec_no_mv(w)
        assert M.mv_within_one_ulp(g, w), (M.mv_of(g), M.mv_of(w))


def _device(streams, calls, skip, softinv=False, rng=None):
    """equally long streams, a channel each, through one consumer in calls of calls[0], calls[1], .. symbols (the last length repeats; rng: drawn from `calls` instead):
    per channel the records and lines in fetch order, the consumer's counts"""
    import torch
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    S = np.ascontiguousarray(np.stack(streams), np.float32)
    n = S.shape[1]
    sf = SoftinDev(len(streams), kind="m20", softinv=softinv, skip=bool(skip))
    d = torch.from_numpy(S).cuda()
    recs, lines = {c: [] for c in range(len(streams))}, {c: [] for c in range(len(streams))}
    pos, i = 0, 0
    while pos < n:
        k = min(int(rng.choice(calls)) if rng is not None else calls[min(i, len(calls) - 1)], n - pos)
        chunk = d[:, pos:pos + k].contiguous()
        sf.push_device(chunk.data_ptr(), k, k)
        for f in sf.fetch_m20():
            recs[f["channel"]].append(M.rec(f)); lines[f["channel"]].append(f["line"].rstrip())
        pos += k; i += 1
    cnt = sf.counts()
    sf.close()
    return recs, lines, cnt


# ---------------------------------------------------------------- 1. streams in device memory
@pytest.mark.parametrize("skip", [True, False], ids=["skip", "noskip"])
@pytest.mark.parametrize("invert", [False, True], ids=["plain", "inverted"])
def test_m20_soft_streams_in_device_memory_equal_reference_m20mod(host, invert, skip):
    have_ref = need_ref()
    rng = np.random.default_rng(1200 + 2 * int(invert) + int(skip))
    nch = 3
    streams = []
    for c in range(nch):
        parts = [M.noise(rng, 100 + 7 * c)]
        for k in range(3):
            s = M.soft(M.frame_symbols(M.m20_bytes(10 * c + k)), rng, (0.6, 1.4))
            if k == 1:
                idx = 44 + 32 + 16 + rng.choice(1000, size=4 + c, replace=False); s[idx] = -s[idx]       # a damaged frame (within the 0x44 bytes summed): checksum [NO]
            parts += [s, M.noise(rng, 2800 + 11 * k)]                                                    # the skipped rest of the second and a bit more
        streams.append(np.concatenate(parts))
    n = min(len(s) for s in streams)
    streams = [(-s[:n] if invert else s[:n]) for s in streams]
    recs, lines, cnt = _device(streams, [9600, 4800, 1000, 251], skip, rng=rng)
    total = ok = 0
    for c in range(nch):
        want, want_lines = M.host_frames(host, streams[c], skip)
        assert len(want) == 3 and [r[2] for r in want] == [1, 0, 1]
        _same(recs[c], want)
        assert lines[c] == want_lines
        if have_ref:
            r = subprocess.run([M.REF, "--softin", "-r", "-v" if skip else "-vvv"], input=streams[c].tobytes(), capture_output=True, timeout=120)
            assert lines[c] == [l.rstrip() for l in r.stdout.decode().splitlines() if l.strip()]
        total += len(recs[c]); ok += sum(r[2] for r in recs[c])
    assert cnt == dict(frames=total, ecc_ok=ok, repaired=0, symbols=0, dropped=0)


# ---------------------------------------------------------------- 2. the emulator's cases on the device
def _against_emulator(emu, streams, calls, skip, softinv=False):
    recs, lines, cnt = _device(streams, calls, skip, softinv=softinv)
    n = 0
    for c, s in enumerate(streams):
        want, dropped, _ = M.emu_frames(emu, s, calls, skip, softinv=softinv)
        assert dropped == 0
        _same(recs[c], want)
        n += len(want)
    assert cnt["frames"] == n and cnt["dropped"] == 0
    return recs


def test_threshold_cases_on_the_device_equal_the_emulator(emu, host):
    """three flips found, four not, the amplitudes that put the score within 1e-3 of 0.8 on either side, windows of exact zeros, the inverted stream with and without
    --softinv: a channel each"""
    amps, lo, hi = M.edge_amplitudes(host)
    streams = [M.threshold_stream(3), M.threshold_stream(4)] + [M.threshold_stream(3, amp=a) for a in amps]
    for softinv, sign in ((False, 1.0), (True, -1.0), (False, -1.0)):
        recs = _against_emulator(emu, [np.float32(sign) * s for s in streams], [9600], 1, softinv=softinv)
        found = [len(recs[c]) for c in range(len(streams))]
        assert found[:2] == [1, 0] and found[2:] == [int(a >= hi) for a in amps] and 0 < sum(found[2:]) < len(amps)
    rng = np.random.default_rng(8)
    fr = M.soft(M.frame_symbols(M.m20_bytes(2), preamble=False), rng, (0.9, 1.1))
    z = np.concatenate([np.zeros(40, np.float32), M.noise(rng, 50), np.zeros(32, np.float32), fr, M.noise(rng, 50)])
    for calls in ([9600], [7]):
        recs = _against_emulator(emu, [z, np.zeros(len(z), np.float32)], calls, 1)
        assert len(recs[0]) == 1 and recs[1] == [] and np.isfinite(M.mv_of(recs[0][0]))


@pytest.mark.parametrize("skip", [1, 0], ids=["skip", "noskip"])
def test_length_and_check_variants_on_the_device_equal_the_emulator(emu, skip):
    v = M.variant_frames()
    names = sorted(v)
    eq = M.equal_pair_stream()
    streams = [M.variant_stream(v[k][0]) for k in names] + [M.variant_stream(M.m20_bytes(12), header_in_payload=True)]
    streams.append(np.concatenate([eq, M.noise(np.random.default_rng(1), len(streams[0]) - len(eq))]))
    recs = _against_emulator(emu, streams, [1000], skip)
    for c, k in enumerate(names):
        f = dict(zip(("nbits", "len", "cs_ok", "cs_calc", "blk_ok", "fw"), recs[c][0][:6]))
        assert recs[c][0][8][:165] == v[k][0]
        for key, val in v[k][1].items():
            assert f[key] == val, (k, key)
    assert len(recs[len(names)]) == 1 and len(recs[len(names) + 1]) == 1
    gaps = [2721, 2720, 2719, 2717]
    ss = [M.skip_end_stream(g) for g in gaps]
    n = min(len(s) for s in ss)
    recs = _against_emulator(emu, [s[:n] for s in ss], [333], skip)
    assert all(len(recs[c]) == 2 for c in range(len(gaps)))


def test_density_without_the_skip_and_the_full_record_buffer(emu, host):
    """four frames in a 9600-symbol call; and more frames in one call than the 4 * 1 + 16 records of a one-channel consumer: 20 delivered, two counted as dropped, the call
    after it intact"""
    s = M.dense_stream(8)
    recs = _against_emulator(emu, [s], [2672 * 4, 9600], 0)
    assert [r[6] for r in recs[0]] == [32 + 2672 * k for k in range(8)]
    s = np.concatenate([M.dense_stream(22, seed=12), M.dense_stream(2, seed=13)])
    calls = [22 * 2672 + 10, 9600]
    got, _, cnt = _device([s], calls, 0)
    want, dropped, _ = M.emu_frames(emu, s, calls, 0, cap=20)
    assert dropped == 2 and len(want) == 22
    _same(got[0], want)
    assert cnt["dropped"] == 2 and cnt["frames"] == 22
    _same(got[0], [r for i, r in enumerate(M.host_frames(host, s, 0)[0]) if i not in (20, 21)])


# ---------------------------------------------------------------- 3. channel indexing
def test_130_channels_in_one_launch_keep_their_frames_apart(host):
    rng = np.random.default_rng(130)
    nch, n = 130, 3 * 129 + 5 + 2716 + 80
    streams = []
    for c in range(nch):
        fr = M.soft(M.frame_symbols(M.m20_bytes(c, seed=9000 + c)), rng, (0.8, 1.2))
        s = np.concatenate([M.noise(rng, 3 * c + 5), fr])
        streams.append(np.concatenate([s, M.noise(rng, n - len(s))]))
    recs, lines, cnt = _device(streams, [n], 1)
    for c in range(nch):
        want, want_lines = M.host_frames(host, streams[c], 1)
        assert len(want) == 1 and want[0][6] == 3 * c + 5 + 44 + 32
        _same(recs[c], want)
        assert lines[c] == want_lines
    assert len({r[0][8] for r in recs.values()}) == nch and cnt["frames"] == nch == cnt["ecc_ok"]


# ---------------------------------------------------------------- 4. auto_rx's pipe
@pytest.fixture(scope="module")
def pipe():
    """(capture, reference raw lines, reference text) of `fsk_demod --cs16 -b -10000 -u 10000 -s -p 5 2 48000 9600 - - | m20mod --json --ptu -vvv --softin -i`"""
    need_ref()
    from tools import synth
    x = synth.m10_capture(sr=48000, seconds=5.0, baud=9600, dev_hz=4800, frame_fn=lambda k: synth.m20_frame(k))
    ref = os.path.join(ROOT, "oracle", "_ref")
    p1 = subprocess.run([os.path.join(ref, "fsk_demod"), "--cs16", "-b", "-10000", "-u", "10000", "-s", "-p", "5", "2", "48000", "9600", "-", "-"],
                        input=x.tobytes(), capture_output=True, timeout=300)
    text = subprocess.run([M.REF, "--json", "--ptu", "-vvv", "--softin", "-i"], input=p1.stdout, capture_output=True, timeout=120).stdout.decode()
    raw = subprocess.run([M.REF, "-r", "-vvv", "--softin", "-i"], input=p1.stdout, capture_output=True, timeout=120).stdout.decode()
    return x, [l.rstrip() for l in raw.splitlines() if l.strip()], text


def _run_pipe(x, nch, order):
    """the capture on nch identical channels, a second per call: order "push" (process + push_fsk), "halves" (wait, collect, submit_fsk, submit_device) or "behind"
    (wait, submit_device, collect, submit_fsk_behind) -> per channel the fetched dicts"""
    import torch
    from radiosonde_auto_rx_amd.fsk import FskModem, SoftinDev
    sr = 48000
    md = FskModem(sr, 9600, n_channels=nch, P=5, lower=-10000, upper=10000)
    sf = SoftinDev(nch, kind="m20", skip=False)
    X = torch.from_numpy(np.stack([x] * nch)).cuda()
    n = X.shape[1] // 2
    out = {c: [] for c in range(nch)}

    def take():
        for f in sf.fetch_m20(verbose=1):
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


def test_m20_modem_to_frames_on_the_device_equals_the_reference_pipe(pipe):
    from radiosonde_auto_rx_amd.telemetry import M20Telemetry
    x, want_raw, want_text = pipe
    assert len(want_raw) >= 4
    out, cnt = _run_pipe(x, 2, "push")
    n = len(out[0])
    lines = [f["line"].rstrip() for f in out[0]]
    assert n >= 4 and lines == want_raw[:n] and len(want_raw) - n <= 1               # (at most the frame the reference prints at EOF is missing)
    assert [M.rec(f) for f in out[1]] == [M.rec(f) for f in out[0]]
    tel = M20Telemetry(verbose=3, ptu=True, version="oracle")
    text = "".join(tel.decode(f) for f in out[0])
    tel.close()
    assert len(text) > 1000 and want_text.startswith(text) and want_text[len(text):].count("{") <= 1
    assert cnt["frames"] == 2 * n and cnt["ecc_ok"] >= 2 * (n - 1) and cnt["dropped"] == 0


@pytest.mark.parametrize("order", ["halves", "behind"])
@pytest.mark.parametrize("abort", [False, True], ids=["plain", "modem_repeats_channel_1"])
def test_pipelined_orders_give_the_frames_of_push_fsk(pipe, monkeypatch, capfd, order, abort):
    """submit_fsk / collect and submit_fsk_behind against process + push_fsk; also when the modem has to repeat a channel (test hook SONDE_FSK_TEST_ABORT: channel 1 gives
    up in every launch) — the modem's wait repeats it before the consumer reads"""
    x = pipe[0]
    plain, cnt0 = _run_pipe(x, 3, "push")
    capfd.readouterr()
    if abort:
        monkeypatch.setenv("SONDE_FSK_TEST_ABORT", "1")
    got, cnt = _run_pipe(x, 3, order)
    err = capfd.readouterr().err
    assert ("repeating them frame by frame" in err) == abort
    assert len(plain[0]) >= 4 and cnt == cnt0
    for c in range(3):
        assert [M.rec(f) for f in got[c]] == [M.rec(f) for f in plain[c]] == [M.rec(f) for f in plain[0]]


# ---------------------------------------------------------------- 5. argument checks
def test_m20_calls_on_another_kind_are_argument_errors():
    import ctypes as C
    from radiosonde_auto_rx_amd.engine import SondeError, SondeM20Frame
    from radiosonde_auto_rx_amd.fsk import SoftinDev, _lib
    sf = SoftinDev(1, kind="m10", ecc=0, inv=False)
    buf = (SondeM20Frame * 4)()
    assert _lib().sonde_softin_dev_fetch_m20(sf._h, buf, 4) == -1 == _lib().sonde_softin_dev_set_m20_skip(sf._h, 0)          # SONDE_E_ARG
    with pytest.raises(SondeError):
        sf.fetch_m20()
    with pytest.raises(SondeError):
        sf.set_m20_skip(False)
    sf.close()
    sf = SoftinDev(1, kind="m20")
    assert sf.fetch_m20() == [] and _lib().sonde_softin_dev_fetch_m20(sf._h, None, 4) == -1 and _lib().sonde_softin_dev_fetch_m20(None, buf, 4) == -1
    sf.set_m20_skip(False); sf.set_m20_skip(True)
    sf.close()
