"""k_search_sync (one launch per call: the frame sync evaluates each header window it reaches with the reference's transform in its own LDS)
against the round structure it replaced on single-type engines (k_sync_plan -> k_sync_window_fft -> k_framesync, kept for mixed engines and
selected here with Engine.set_search_rounds).  Both engines see the same bytes in the same calls; after every call their frames (bytes, ECC
value, score, position), summary records and per-channel sync state must be equal, and the one-launch search may only transform fewer windows."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SR = 96_000
SECONDS = 4.3


def _captures():
    """8 channels: received sondes (clean, noisy with bit errors, frequency offset), digital silence in front of a sonde, a sonde that
    starts late, and channels that never lock (noise, and digital silence throughout)."""
    from tools import synth
    n = int(SR * SECONDS)
    fq = synth.snap_fq(0.1, SR)
    rows = []
    rows.append(synth.rs41_capture(sr=SR, seconds=SECONDS, fq=fq, seed=11, noise_sigma=0.02))
    rows.append(synth.rs41_capture(sr=SR, seconds=SECONDS, fq=fq, seed=12, noise_sigma=0.08, bit_errors=9))
    rows.append(synth.rs41_capture(sr=SR, seconds=SECONDS, fq=fq, seed=13, noise_sigma=0.03, f_offset_hz=700.0, t_first=0.55))
    x = synth.rs41_capture(sr=SR, seconds=SECONDS, fq=fq, seed=14, noise_sigma=0.03, t_first=0.4)
    x[:2 * int(0.3 * SR)] = 0                                               # digital silence at the start (the mp = -1 / rc -5 path)
    rows.append(x)
    rows.append(synth.rs41_capture(sr=SR, seconds=SECONDS, fq=fq, seed=15, noise_sigma=0.03, t_first=2.1))
    rows.append(synth.rs41_capture(sr=SR, seconds=SECONDS, fq=fq, seed=16, noise_sigma=0.05, bit_errors=3, t_first=0.93))
    rng = np.random.default_rng(17)
    rows.append(np.clip(rng.normal(0, 800, 2 * n), -32768, 32767).astype(np.int16))     # noise: never locks
    rows.append(np.zeros(2 * n, np.int16))                                              # silence throughout
    rows = [r[:2 * n] for r in rows]
    return fq, np.stack(rows)


def _frames(eng):
    fr = eng.fetch_frames()
    return sorted((f["channel"], f["mv_pos"], f["mv"], f["len"], f["ecc"], f["nbytes"], f["frame"]) for f in fr)


CHUNKINGS = {
    "one_call": lambda n: [n],                                              # several frames in one long call
    "short_calls": lambda n: [2_000 * 2] * (n // 4_000),                   # calls much shorter than one window (4000 input = 2000 IF samples)
    "irregular": lambda n: [37_000, 61_500, 96_000, 10, 150_020, 23_990, 88_000, 41_000],   # frames and headers split across calls
    "seconds": lambda n: [SR] * (n // SR),
}


@pytest.mark.parametrize("chunking", sorted(CHUNKINGS))
def test_search_sync_matches_rounds(chunking):
    import torch
    from radiosonde_auto_rx_amd.engine import Engine
    from radiosonde_auto_rx_amd import shard
    fq, x = _captures()
    C, n = x.shape[0], x.shape[1] // 2
    pieces = [p for p in CHUNKINGS[chunking](n) if p > 0]
    max_chunk = max(pieces)
    engs, sums = [], []
    for rounds in (False, True):
        e = Engine([fq] * C, SR, ecc=2, max_chunk=max_chunk, max_frames=64)
        e.set_search_rounds(rounds)
        e.count_windows(True)
        s = shard.summary_buffer(C, torch.device("cuda", 0))
        e.set_summary(s.data_ptr(), 0)
        engs.append(e); sums.append(s)
    pos, n_frames, calls = 0, 0, 0
    for p in pieces:
        if pos + p > n:
            break
        chunk = np.ascontiguousarray(x[:, 2 * pos:2 * (pos + p)])
        for e in engs:
            e.process_host(chunk)
        fa, fb = _frames(engs[0]), _frames(engs[1])
        assert fa == fb, (chunking, calls, len(fa), len(fb))
        sa, sb = engs[0].sync_state(), engs[1].sync_state()
        assert np.array_equal(sa, sb), (chunking, calls, np.nonzero((sa != sb).any(1))[0], sa, sb)
        torch.cuda.synchronize()
        ra, rb = shard.decode_summaries(sums[0]), shard.decode_summaries(sums[1])
        assert ra.tobytes() == rb.tobytes(), (chunking, calls)
        n_frames += len(fa)
        pos += p
        calls += 1
    # end of stream: the frames in progress (old kernels on both)
    fa = sorted((f["channel"], f["mv_pos"], f["len"], f["ecc"], f["nbytes"], f["frame"]) for f in engs[0].fetch_frames(finish=True))
    fb = sorted((f["channel"], f["mv_pos"], f["len"], f["ecc"], f["nbytes"], f["frame"]) for f in engs[1].fetch_frames(finish=True))
    assert fa == fb
    ca, cb = engs[0].count_windows(False), engs[1].count_windows(False)
    for e in engs:
        e.close()
    assert n_frames >= 12, n_frames                                        # the sondes were received
    assert ca["round0"] == 0 and ca["rounds"] == 0 and cb["search_sync"] == 0, (ca, cb)
    assert 0 < ca["search_sync"] <= cb["round0"] + cb["rounds"], (ca, cb)
