"""The dropsonde engine on float32 IQ with channels handed out at run time (DropEngine(bits=32): k_fm_front + k_drop_slice_rt + k_drop_restart).
 - float32 samples that are an int16 capture / 32768 against the int16 IQ engine on that capture: the FM stream within the 1-LSB rule of iq_dec's integer
   output (tests/test_gpu_iqdec.py), the frames identical;
 - the printer's text from the engine's frames against the reference pipeline `iq_dec --FM --lpFM --wav --bo 16 --iq <fq> - <sr> 32 | rd94rd41drop -b ...` on the
   float32 goldens (tests/dropf32_cases.py), byte for byte, the end of every stream through finish_channel;
 - one stream in calls of 12 000, 12 345, 3 001 and 7 samples: identical frames, identical FM stream;
 - four slots, rows further apart than a call is long, released rows full of NaN: release, restart (also in the middle of an IQ-dc block), reuse, finish of one
   slot, each against a one-channel engine fed the same samples;
 - what is refused.
Every capture is at 48 or 50 kHz and at most 2 s long."""
import functools

import numpy as np
import pytest

from tests import dropf32_cases as cases
from tests.test_drop_fields import _printer

pytestmark = pytest.mark.gpu
E_ARG, E_RANGE = -1, -4


def _engine(sr, fqs, chunk, argv=("-b",)):
    from radiosonde_auto_rx_amd.drop import DropEngine
    return DropEngine(fqs, sr, bits=32, invert="-i" in argv, opt_b="-b" in argv, max_chunk=chunk)


def _calls(n, lengths):
    """(start, length) of the calls over n samples; the last length repeats"""
    out, at, k = [], 0, 0
    while at < n:
        m = min(lengths[min(k, len(lengths) - 1)], n - at)
        out.append((at, m))
        at, k = at + m, k + 1
    return out


def _solo(x, sr, fq, lengths, argv=("-b",), end="finish_channel", fm=True):
    """one channel over the float32 capture x in calls of `lengths` -> (frames, the FM stream as read_fm gives it call by call, frames per call)"""
    n = len(x) // 2
    eng = _engine(sr, [fq], max(lengths), argv)
    frames, stream, per_call = [], [], []
    for at, m in _calls(n, lengths):
        eng.process_host(x[None, 2 * at:2 * (at + m)])
        got = eng.fetch_frames()
        frames += got
        per_call.append(got)
        if fm:
            stream.append(eng.read_fm(0, at, m))
    if end == "finish_channel":
        assert eng.channel_active(0)
        eng.finish_channel(0)
        assert not eng.channel_active(0)
    elif end == "finish":
        eng.finish()
    tail = eng.fetch_frames()
    eng.close()
    return frames + tail, (np.concatenate(stream) if fm else None), per_call + [tail]


def _close(got, ref):
    d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    off = float(np.mean(d != 0))
    print("FM: max |diff| %d LSB, %.4f %% of %d samples differ" % (d.max(), 100 * off, len(d)))
    assert d.max() <= 1 and off < 0.01, (int(d.max()), off)


# ---------------------------------------------------------------- float32 equals int16 where it can
@pytest.mark.parametrize("kind,invert", [(94, False), (41, False), (41, True)])
def test_float32_of_an_int16_capture_equals_the_int16_engine(kind, invert):
    from radiosonde_auto_rx_amd.drop import DropEngine
    from radiosonde_auto_rx_amd.engine import Engine, TAP_FM
    from tools import synth
    sr, chunk = 48000, 12000
    xi = synth.drop_capture(sr=sr, n_frames=3, lead_s=0.2, kind=kind, seed=90 + kind + int(invert), invert=invert, f_offset_hz=250.0)
    n = len(xi) // 2
    assert n <= 2 * sr
    xf = (xi.astype(np.float32) / np.float32(32768.0)).astype(np.float32)                   # exact: what f32read_cblock makes of the int16 sample
    argv = ["-b", "-i"] if invert else ["-b"]
    e16 = DropEngine([0.0], sr, bits=16, invert=invert, opt_b=True, max_chunk=chunk)
    f16 = []
    for at, m in _calls(n, [chunk]):
        e16.process_host(xi[None, 2 * at:2 * (at + m)])
        f16 += e16.fetch_frames()
    e16.finish()
    f16 += e16.fetch_frames()
    e16.close()
    f32, fm32, _ = _solo(xf, sr, 0.0, [chunk], argv, end="finish")
    assert len(f16) == 3 and all(f["complete"] and f["nraw"] == 2400 for f in f16), f16
    assert f32 == f16                                                                        # bytes, err94, err41, sample, nraw, complete, channel
    # the front end the int16 engine runs inside (FmSliceEngine::create_front), its FM ring through the same conversion
    fe = Engine([0.0], sr, sonde="frontend", lp_iq=False, lp_fm=True, lpiq_bw=10000, if_rate=48000, max_chunk=chunk)
    ref = []
    for at, m in _calls(n, [chunk]):
        fe.process_host(xi[2 * at:2 * (at + m)])
        v = fe.read_tap(0, TAP_FM, at, m).astype(np.float32) * np.float32(128.0)
        ref.append(np.trunc(v * np.float32(256.0)).astype(np.int64).astype(np.int16))
    fe.close()
    _close(fm32, np.concatenate(ref))


# ---------------------------------------------------------------- the reference pipeline on float32
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_engine_text_equals_the_reference_pipeline(name):
    case, g = cases.CASES[name], cases.load(name)
    x = cases.samples(case["gen"])
    sr = case["gen"]["sr"]
    assert len(x) // 2 <= 2 * sr
    if name == "50k_big41":
        assert np.abs(x).max() > 1.0
    for argv, ref in zip(g["argv"], g["stdout"]):
        frames, _, _ = _solo(x, sr, case["fq"], [sr // 4], argv, fm=False)
        p = _printer(argv)
        text = "".join(p.frame(f["bytes"]) for f in frames)
        print(name, argv, "frames", len(frames), "lines", text.count("\n"), ref.count(b"\n"), "equal", text.encode() == ref)
        assert text.encode() == ref, (name, argv, text[-900:], ref[-900:])
        if "cut" in name:
            assert [f["complete"] for f in frames] == [True, True, False] and 40 < frames[-1]["nraw"] < 2400
        if case["gen"].get("invert") and "-i" not in argv:
            assert frames == []


# ---------------------------------------------------------------- chunking
@functools.lru_cache(maxsize=None)
def _short_capture():
    from tools import synth
    x = synth.to_f32(synth.drop_capture(sr=50000, n_frames=1, lead_s=0.1, kind=94, seed=95, fq=0.014)) + np.float32(0.02)   # (a DC offset: the IQ-dc averages matter)
    x = np.ascontiguousarray(x, np.float32)
    x.setflags(write=False)
    return x


def test_frames_and_fm_stream_do_not_depend_on_the_calls():
    x = _short_capture()
    assert len(x) // 2 < 40000
    base_f, base_fm, _ = _solo(x, 50000, 0.014, [12000])
    assert len(base_f) == 1 and base_f[0]["complete"], base_f
    for lengths in ([12345], [3001], [7], [12000, 7, 12345, 3001, 7, 7]):
        f, fm, _ = _solo(x, 50000, 0.014, lengths)
        assert f == base_f, lengths
        assert np.array_equal(fm, base_fm), lengths


# ---------------------------------------------------------------- slots
N, STRIDE, SLOTS = 5000, 6000, 4


@functools.lru_cache(maxsize=None)
def _cap(name):
    x = cases.samples(cases.CASES[name]["gen"])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _solo_case(name, ncalls=None, end="finish_channel"):
    """a one-channel engine over the capture (its first ncalls calls of N samples) -> (frames per call + [what the end gave], FM stream)"""
    x = _cap(name)
    if ncalls is not None:
        x = x[:2 * N * ncalls]
    _, fm, per_call = _solo(x, 50000, cases.CASES[name]["fq"], [N], end=end)
    return per_call, fm


def test_slots_are_released_restarted_reused_and_finished_one_by_one():
    import torch
    A, B, Cc = "50k_94_fq014", "50k_dc94", "50k_41_fqm010"
    fq = {n: cases.CASES[n]["fq"] for n in (A, B, Cc)}
    eng = _engine(50000, [0.0] * SLOTS, N)
    for c in range(SLOTS):
        eng.release_channel(c)
        assert not eng.channel_active(c)
    buf = torch.full((SLOTS, STRIDE, 2), float("nan"), dtype=torch.float32, device="cuda")
    feeds = {}                                                   # slot -> (capture, its first call)
    got = {c: [] for c in range(SLOTS)}                          # slot -> frames per call since its restart
    fm = {c: [] for c in range(SLOTS)}

    def start(slot, name, i, f=None):
        eng.restart_channel(slot, fq[name] if f is None else f)
        assert eng.channel_active(slot)
        feeds[slot], got[slot], fm[slot] = (name, i), [], []

    def call(i):
        host = np.full((SLOTS, STRIDE, 2), np.nan, np.float32)   # released rows, and every row behind its N samples: NaN
        for slot, (name, i0) in feeds.items():
            x = _cap(name).reshape(-1, 2)
            seg = x[(i - i0) * N:(i - i0 + 1) * N]
            host[slot, :len(seg)] = seg
            host[slot, len(seg):N] = 0.0                         # (behind the end of a capture: silence)
        buf.copy_(torch.from_numpy(host))
        torch.cuda.synchronize()
        eng.process_device(buf.data_ptr(), N, ch_stride=STRIDE)
        frames = eng.fetch_frames()
        assert all(f["channel"] in feeds for f in frames), frames
        for slot, (name, i0) in feeds.items():
            got[slot].append([dict(f, channel=0) for f in frames if f["channel"] == slot])
            fm[slot].append(eng.read_fm(slot, (i - i0) * N, N))

    def same_as_solo(slot, name, ncalls):
        per_call, solo_fm = _solo_case(name)
        assert got[slot][:ncalls] == per_call[:ncalls], (slot, name)
        cat = np.concatenate(fm[slot][:ncalls])[:len(solo_fm)]  # (the capture's last call is shorter than N)
        assert np.array_equal(cat, solo_fm[:len(cat)]), (slot, name)

    call(0)                                                      # every slot released, NaN everywhere: nothing comes out
    assert eng.fetch_frames() == []
    start(0, A, 1)
    call(1)
    start(2, Cc, 2, 0.3)                                         # one call of something else: 5000 samples end inside the third IQ-dc block (1562 + 3124 + 314)
    call(2)
    start(2, B, 3)                                               # call 3: slot 2 restarted with a fq of its own, in the middle of that block
    call(3)
    start(1, Cc, 4)
    for i in range(4, 15):
        call(i)
    # slot 1 after 11 calls (55 000 samples: inside the second frame, its header open): its end equals sonde_drop_finish of a one-channel engine there
    cut_calls, _ = _solo_case(Cc, 11, "finish")
    assert got[1] == cut_calls[:11]
    eng.finish_channel(1)
    tail = [dict(f, channel=0) for f in eng.fetch_frames()]
    assert tail == cut_calls[11] and len(tail) == 1 and not tail[0]["complete"] and 40 < tail[0]["nraw"] < 2400, (tail, cut_calls[11])
    assert not eng.channel_active(1)
    del feeds[1]
    for i in range(15, 23):
        call(i)
    nA, nB = len(_solo_case(A)[0]) - 1, len(_solo_case(B)[0]) - 1  # calls of the whole captures (20 each)
    assert nA == 20 and nB == 20
    same_as_solo(0, A, nA)                                       # slot 0 ran throughout: as in an engine where nothing else ever happens
    same_as_solo(2, B, nB)                                       # slot 2 from its restart: a fresh engine fed the same samples, `sample` counting from there
    assert sum(len(c) for c in got[0]) == 3 and sum(len(c) for c in got[2]) == 3
    assert [f["sample"] for c in got[2] for f in c] == [f["sample"] for c in _solo_case(B)[0] for f in c]
    # a released slot is restarted on another capture and reused
    eng.release_channel(2)
    del feeds[2]
    call(23)
    start(2, Cc, 24)
    for i in range(24, 37):
        call(i)
    same_as_solo(2, Cc, 13)
    assert sum(len(c) for c in got[2]) == 2
    eng.close()


# ---------------------------------------------------------------- refusals
def _code(fn):
    from radiosonde_auto_rx_amd.engine import SondeError
    with pytest.raises(SondeError) as ei:
        fn()
    return ei.value.args[0]


def test_refusals():
    from radiosonde_auto_rx_amd.drop import IN_FM, DropEngine
    assert _code(lambda: DropEngine((), 48000, bits=32, input=IN_FM, n_channels=1)) == E_ARG
    assert _code(lambda: DropEngine([0.0], 96000, bits=32)) == E_ARG
    assert _code(lambda: DropEngine([0.0], 100000, bits=32)) == E_ARG
    e16 = DropEngine([0.0, 0.0], 48000, bits=16, max_chunk=4800)
    z = np.zeros((2, 2 * 4800), np.float32)
    for fn in (lambda: e16.restart_channel(0, 0.1), lambda: e16.release_channel(0), lambda: e16.finish_channel(0), lambda: e16.channel_active(0),
               lambda: e16.read_fm(0, 0, 1), lambda: e16.process_device(1 << 20, 4800, ch_stride=4800)):
        assert _code(fn) == E_ARG
    e16.close()
    e = _engine(50000, [0.0, 0.0], 5000)
    for fn in (lambda: e.restart_channel(2, 0.1), lambda: e.restart_channel(-1, 0.1), lambda: e.release_channel(2), lambda: e.finish_channel(2),
               lambda: e.channel_active(-1), lambda: e.read_fm(2, 0, 1),
               lambda: e.restart_channel(0, 0.5001), lambda: e.restart_channel(0, -0.6), lambda: e.restart_channel(0, float("nan")),
               lambda: e.process_device(1 << 20, 4800, ch_stride=4799)):
        assert _code(fn) == E_ARG
    assert _code(lambda: e.process_host(np.zeros((2, 2 * 5001), np.float32))) == E_RANGE
    assert _code(lambda: e.read_fm(0, 0, 1)) == E_RANGE        # nothing processed yet
    e.process_host(z[:, :2 * 4800])                            # the engine still works
    assert e.fetch_frames() == [] and len(e.read_fm(1, 4700, 100)) == 100
    e.release_channel(1)                                       # a released slot has no stream to count in
    assert _code(lambda: e.read_fm(1, 4700, 100)) == E_ARG
    e.close()
