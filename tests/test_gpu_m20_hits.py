"""M20 hits decoded on the device in base-rate and mixed engines (k_m20_hits behind the frame sync, radiosonde_auto_rx_amd/csrc/sonde_m20_hits.hip) against the
host code they replace (mxx_bytes + sonde_m20_frame_finish inside sonde_engine_fetch_m20, kept as the A/B path: sonde_engine_set_device_ecc(0) / SONDE_HOST_ECC=1)
and against the CPU emulation of the same source (tests/test_m20_hits_emu.py): the same records in all 208 bytes — on constructed records through
sonde_m20_decode_device, on noisy captures whose streams end inside a frame, with lagged fetches, in a mixed engine beside the other three types, with a ring that
wraps, and behind a channel restart.  (That either path equals the reference's decoder is what test_gpu_m10.py, test_gpu_mixed.py, test_gpu_chain.py and
test_gpu_broker.py check — with the device path, the default.)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR = 48_000


def _frame165(k, j, **kw):
    """a frame that fills all 165 bytes the engine slices: tools/synth.m20_frame and random bytes behind it (so that a frame's tail is not all zeros)"""
    from tools import synth
    return synth.m20_frame(j, rng=np.random.default_rng(500 + 31 * k + j), **kw) + bytes(np.random.default_rng(900 + 31 * k + j).integers(0, 256, 95, dtype=np.uint8))


_cap = {}


def _capture3():
    """3 channels at 48 kHz, cut at 2.42 s: frames at 0.2 + 0.03 k, + 1 s, + 2 s — every stream ends inside its third frame; noise 0.02 .. 0.5, checksum, block and
    firmware variants"""
    if "x" not in _cap:
        from tools import synth
        fqs = [synth.snap_fq(f, SR) for f in (0.0, 0.05, -0.06)]

        def fn(k):
            return lambda j: _frame165(k, j, fw=(6, 8)[(j + k) % 2], blk=("ok", "zero", "bad")[(j + 2 * k) % 3], good_checksum=(j + k) % 3 != 1)
        x = np.stack([synth.m10_capture(sr=SR, seconds=2.6, fq=fq, baud=9600.0, noise_sigma=(0.02, 0.2, 0.5)[k], seed=220 + k, t_first=0.2 + 0.03 * k,
                                        f_offset_hz=90.0 * (k - 1), frame_fn=fn(k)) for k, fq in enumerate(fqs)])[:, :2 * int(2.42 * SR)]
        _cap["x"] = (fqs, x)
    return _cap["x"]


def _recs(buf, n):
    """records of a raw fetch -> [(channel, the record's 208 bytes)]"""
    from radiosonde_auto_rx_amd.engine import SondeM20Frame
    return [(buf[i].channel, bytes(SondeM20Frame.from_buffer_copy(buf[i]))) for i in range(n)]


def _by_channel(recs):
    """(the order in which different channels' records are queued is not defined — a channel's own is)"""
    d = {}
    for ch, r in recs:
        d.setdefault(ch, []).append(r)
    return d


def _run(fqs, x, *, dev=True, lag=0, max_frames=64, chunk=None, with_soft=False, sr=SR):
    """a single-type M20 engine over the capture -> (records, soft bits per record, overflowed)"""
    from radiosonde_auto_rx_amd.engine import Engine, lib
    eng = Engine(fqs, sr, sonde="m20", ecc=0, max_chunk=sr, max_frames=max_frames)
    eng.set_device_ecc(dev)
    D = eng.info["decM"]
    n = x.shape[-1] // 2
    chunk = chunk or (sr // 2 + 30 * D)                          # no multiple of a second
    out, soft = [], []

    def take(buf, k):
        out.extend(_recs(buf, k))
        if with_soft and k:
            s = np.zeros((k, eng.nbits), np.float32)
            assert lib().sonde_engine_fetch_soft(eng._h, s.ctypes.data_as(C.c_void_p), k) == k
            soft.extend(s[i].copy() for i in range(k))
    for pos in range(0, n, chunk):
        m = min(chunk, n - pos) // D * D
        if m <= 0:
            break
        eng.process_host(x[..., 2 * pos:2 * (pos + m)])
        take(*eng.fetch_m20_raw(lag=lag))
    take(*eng.fetch_m20_raw(finish=True))
    ovf = eng.overflowed()
    eng.close()
    return out, soft, ovf


_runs = {}


def _default_run():
    if "d" not in _runs:
        fqs, x = _capture3()
        _runs["d"] = _run(fqs, x, with_soft=True)
    return _runs["d"]


# ---------------------------------------------------------------- 1. the kernel on constructed records
def test_constructed_records_equal_the_emulator_byte_for_byte():
    import m20_hits_cases as M
    from radiosonde_auto_rx_amd.engine import decode_m20_hits_device
    recs, nch = M.records()
    want, want_chars, _ = M.emu_run(M.load_emu(), recs, nch, grid=nch)
    got, chars = decode_m20_hits_device(np.stack([r[1] for r in recs]), [r[2] for r in recs], [r[3] for r in recs], nch, mv=[r[4] for r in recs], with_chars=True)
    assert C.sizeof(got[0]) == 208
    for (name, *_), g, w in zip(recs, got, want):
        assert bytes(g) == bytes(w), name
    assert np.array_equal(chars, want_chars)
    assert {f.cs_ok for f in want} == {0, 1} and {f.blk_ok for f in want} == {-1, 0, 1}
    # one channel, fewer workgroups than records: the chain alone, in the given order
    chain = [r for r in recs if r[0].startswith("chain")]
    got1, chars1 = decode_m20_hits_device(np.stack([r[1] for r in chain]), [r[2] for r in chain], 0, 1, mv=[r[4] for r in chain], with_chars=True)
    want1, want1_chars, _ = M.emu_run(M.load_emu(), [(n, b, nb, 0, mv) for n, b, nb, _, mv in chain], 1)
    assert [bytes(got1[i]) for i in range(3)] == [bytes(w) for w in want1] and np.array_equal(chars1, want1_chars)


# ---------------------------------------------------------------- 2. a single-type engine: device path against host path
def test_engine_frames_on_the_device_equal_the_host_decode_and_the_soft_bits_follow():
    fqs, x = _capture3()
    a, sa, ovf = _default_run()
    b, sb, _ = _run(fqs, x, dev=False, with_soft=True)
    assert not ovf and len(a) == len(b) and len(a) >= 6
    assert _by_channel(a) == _by_channel(b)
    from radiosonde_auto_rx_amd.engine import SondeM20Frame
    fr = [SondeM20Frame.from_buffer_copy(r) for _, r in a]
    assert {bool(f.cs_ok) for f in fr} == {True, False} and any(f.nbits < 1320 for f in fr) and any(f.nbits == 1320 for f in fr)
    # the soft bits fetched afterwards (lazily, from their ring slots on the device path): the same ones, hit by hit
    key = lambda r: (r[0], r[1][28:32])                          # noqa: E731  (channel, mv_pos)
    soft_b = {key(r): s for r, s in zip(b, sb)}
    assert len(sa) == len(a) and len(soft_b) == len(b)
    for r, s in zip(a, sa):
        assert np.array_equal(s, soft_b[key(r)])


# ---------------------------------------------------------------- 3. lagged fetches, the switch
def test_lagged_fetches_give_the_unlagged_frames_and_a_switch_with_records_queued_is_refused():
    from radiosonde_auto_rx_amd.engine import Engine, lib
    fqs, x = _capture3()
    a, _, _ = _default_run()
    b, _, ovf = _run(fqs, x, lag=1)
    assert not ovf and _by_channel(b) == _by_channel(a) and len(b) == len(a)
    h, _, _ = _run(fqs, x, dev=False, lag=1)                     # (the host path behind a lagged fetch as well)
    assert _by_channel(h) == _by_channel(a)
    # the switch: between records only.  (A frame is queued once the search window it lies in is complete, which takes a second call here.)
    eng = Engine(fqs, SR, sonde="m20", ecc=0, max_chunk=SR, max_frames=64)
    eng.process_host(x[..., :2 * SR])
    eng.process_host(x[..., 2 * SR:4 * SR])                      # the first frames are queued, nothing is fetched
    assert lib().sonde_engine_set_device_ecc(eng._h, 0) == -1    # SONDE_E_ARG: fetch first
    first = _recs(*eng.fetch_m20_raw())                          # decoded on the device
    assert len(first) >= 2 and lib().sonde_engine_set_device_ecc(eng._h, 0) == 0
    eng.process_host(x[..., 4 * SR:])
    second = _recs(*eng.fetch_m20_raw(finish=True))              # decoded on the host
    assert len(second) >= 2 and lib().sonde_engine_set_device_ecc(eng._h, 1) == 0
    eng.close()
    want = _by_channel(a)
    for ch, rs in _by_channel(first + second).items():
        assert len(rs) == len(want[ch])
        for r, w in zip(rs, want[ch]):
            nv = int.from_bytes(r[4:8], "little")
            # a full frame does not depend on where the channel's characters were kept before; of a frame the end of input cut short, the bytes its own bits fill
            assert r == w if nv == 1320 else (r[:4] == w[:4] and r[28:36 + nv // 8] == w[28:36 + nv // 8] and nv == int.from_bytes(w[4:8], "little")), ch
    assert any(int.from_bytes(r[4:8], "little") == 1320 for _, r in second)


# ---------------------------------------------------------------- 4. a mixed engine
def test_m20_channels_of_a_mixed_engine_equal_a_single_type_engine(monkeypatch):
    from tools import synth
    from radiosonde_auto_rx_amd.engine import MixedEngine
    sr = 480_000
    kinds = ["m20", "rs41", "dfm", "m20", "m10"]
    rng = np.random.default_rng(20)
    fqs = [synth.snap_fq(float(rng.uniform(-0.3, 0.3)), sr) for _ in kinds]
    secs = 2.6                                                   # (cut at 2.42 s below: the M20 streams end inside their third frames)
    caps = []
    for k, kd in enumerate(kinds):
        if kd == "m20":
            caps.append(synth.m10_capture(sr=sr, seconds=secs, fq=fqs[k], baud=9600.0, noise_sigma=0.03 + 0.05 * k, seed=320 + k, t_first=0.2 + 0.03 * k,
                                          frame_fn=lambda j, k=k: _frame165(k, j, fw=(6, 8)[j % 2], good_checksum=(j + k) % 3 != 1)))
        elif kd == "rs41":
            caps.append(synth.rs41_capture(sr=sr, seconds=secs, fq=fqs[k], seed=330, noise_sigma=0.05, bit_errors=6, t_first=0.15))
        elif kd == "dfm":
            caps.append(synth.dfm_capture(sr=sr, seconds=secs, fq=fqs[k], noise_sigma=0.1, seed=331, bit_errors_per_frame=1, t_first=0.05))
        else:
            caps.append(synth.m10_capture(sr=sr, seconds=secs, fq=fqs[k], noise_sigma=0.1, seed=332, t_first=0.25,
                                          frame_fn=lambda j: synth.m10_frame(j, rng=np.random.default_rng(740 + j), good_checksum=j != 1)))
    n = int(2.42 * sr)
    x = np.stack([c[:2 * n] for c in caps])

    def mixed(lag):
        eng = MixedEngine(fqs, kinds, sr, max_chunk=sr, max_frames=64)
        D = eng.info["decM"]
        chunk = sr // 2 + 30 * D
        m20 = []
        for pos in range(0, n, chunk):
            m = min(chunk, n - pos) // D * D
            if m <= 0:
                break
            eng.process_host(x[:, 2 * pos:2 * (pos + m)])
            m20 += _recs(*eng.fetch_m20_raw(lag=lag))
        others = dict(rs41=[(f["channel"], f["mv_pos"], f["line"]) for f in eng.fetch_frames(finish=True)],
                      dfm=[(f["channel"], f["mv_pos"], f["line"]) for f in eng.fetch_dfm(finish=True)],
                      m10=[(f["channel"], f["mv_pos"], f["line"]) for f in eng.fetch_mxx(finish=True)])
        m20 += _recs(*eng.fetch_m20_raw(finish=True))
        assert not eng.overflowed()
        eng.close()
        return m20, others
    sel = [c for c, kd in enumerate(kinds) if kd == "m20"]
    single, _, _ = _run([fqs[c] for c in sel], np.ascontiguousarray(x[sel]), sr=sr)
    want = {}
    for ch, r in single:                                         # the single engine's channel numbers -> the mixed engine's
        want.setdefault(sel[ch], []).append(int(sel[ch]).to_bytes(4, "little") + r[4:])
    m0, o0 = mixed(0)
    m1, o1 = mixed(1)
    assert sorted(want) == sel and all(len(v) >= 3 for v in want.values())
    assert _by_channel(m0) == want and _by_channel(m1) == want
    assert o0 == o1 and all(len(v) >= 2 for v in o0.values())
    # every block code on the host (the switch read at create): the M20 frames are the same, and so are the other types' with the variable unset
    monkeypatch.setenv("SONDE_HOST_ECC", "1")
    mh, oh = mixed(0)
    monkeypatch.delenv("SONDE_HOST_ECC")
    assert _by_channel(mh) == want and oh == o0


# ---------------------------------------------------------------- 5. a ring that wraps while the fetches keep up
def test_a_small_ring_wraps_and_nothing_is_lost():
    fqs, x = _capture3()
    want = {ch: rs for ch, rs in _by_channel(_default_run()[0]).items() if ch < 2}
    for lag in (0, 1):
        # channels 0 and 1 alone: 6 records through 4 slots; a fetch never finds more than two frames a channel (the last call's and the end of input's)
        b, _, ovf = _run(fqs[:2], np.ascontiguousarray(x[:2]), max_frames=4, lag=lag)
        assert not ovf and len(b) == 6 and _by_channel(b) == want, lag


# ---------------------------------------------------------------- 6. the channel restart clears the characters
def test_a_restarted_channel_starts_on_zero_characters():
    from tools import synth
    from radiosonde_auto_rx_amd.engine import Engine, SondeM20Frame
    one = synth.m10_capture(sr=SR, seconds=1.3, baud=9600.0, noise_sigma=0.02, seed=410, t_first=0.2, frame_fn=lambda j: _frame165(7, j))
    two = synth.m10_capture(sr=SR, seconds=1.3, baud=9600.0, noise_sigma=0.02, seed=411, t_first=0.2, frame_fn=lambda j: _frame165(8, j))
    cut = int(SR * (0.2 + (80 + 2 * 700) / 9600.0))              # the second stream ends about 700 bits into its frame

    def run(dev, restart):
        eng = Engine([0.0], SR, sonde="m20", ecc=0, max_chunk=2 * SR, max_frames=16)
        eng.set_device_ecc(dev)
        eng.process_host(one[None, :])
        first = _recs(*eng.fetch_m20_raw())
        if restart:
            eng.restart_channel(0)
        eng.process_host(two[None, :2 * cut])
        last = _recs(*eng.fetch_m20_raw(finish=True))
        eng.close()
        assert len(first) == 1 and len(last) == 1
        return SondeM20Frame.from_buffer_copy(first[0][1]), SondeM20Frame.from_buffer_copy(last[0][1])
    f1, f2 = run(True, True)
    assert f1.nbits == 1320 and 600 < f2.nbits < 800 and any(f1.frame[110:165])
    assert not any(f2.frame[f2.nbits // 8 + 1:])                 # zeros behind the terminator
    h1, h2 = run(False, True)
    assert bytes(h1) == bytes(f1) and bytes(h2) == bytes(f2)
    c1, c2 = run(True, False)                                    # without the restart the first frame's tail is still there
    assert bytes(c1) == bytes(f1) and c2.nbits < 1320 and bytes(c2.frame[c2.nbits // 8 + 1:165]) == bytes(f1.frame[c2.nbits // 8 + 1:165])
