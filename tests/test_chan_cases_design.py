"""The channelizer sweep's reference and cases (tests/chan_cases.py) held to the defining sum and to the launch's arithmetic — no GPU."""
import numpy as np
import pytest

import chan_cases as cc

ALL = cc.RUN + cc.REFUSED


@pytest.mark.parametrize("case", cc.RUN, ids=cc.case_id)
def test_reference_equals_the_sampled_direct_sum(case):
    M, D, P = case
    xi = cc.stream(M, D, P, "uniform")
    x = cc.to_complex(xi)
    nf = cc.n_frames(len(x), D)
    y, u_norm, a_norm = cc.expected(M, D, P, "uniform")
    assert y.shape == (M, nf) and u_norm.shape == a_norm.shape == (nf,)
    ms = [0, 15, 16, 17, nf - 1]
    ks = [0, 1, M // 2 - 1, M // 2, M - 3]
    want = cc.direct(x, cc.taps(M, P), M, D, ms, ks)
    assert np.abs(y[np.ix_(ks, ms)] - want).max() <= 1e-12
    # the branch sums can be no larger than their magnitude budget, and Parseval ties them to the outputs
    assert (u_norm <= a_norm * (1 + 1e-12)).all()
    assert np.allclose(np.linalg.norm(y, axis=0), np.sqrt(M) * u_norm, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("case", ALL, ids=cc.case_id)
def test_taps_sum_to_one_and_are_symmetric(case):
    M, D, P = case
    h = cc.taps(M, P)
    assert h.dtype == np.float32 and len(h) == M * P
    # every tap is rounded to float32 on its own: at most half a unit of its last place each
    assert abs(h.astype(np.float64).sum() - 1.0) <= 2.0 ** -24 * np.abs(h.astype(np.float64)).sum()
    assert np.abs(h - h[::-1]).max() <= 2.0 ** -24 * h.max()
    assert h.argmax() in (M * P // 2 - 1, M * P // 2)


def test_lds_formula_gives_the_listed_byte_counts():
    want = {(256, 256, 16): 64_512, (256, 200, 32): 77_536, (512, 400, 8): 105_920, (1024, 128, 4): 155_136, (1024, 800, 8): 211_840}
    for c, b in want.items():
        assert cc.lds_bytes(*c) == b, c
    for c in cc.RUN:
        assert cc.lds_bytes(*c) <= cc.LDS_LIMIT, c
    for c in cc.REFUSED:
        assert cc.lds_bytes(*c) > cc.LDS_LIMIT, c
        M, D, P = c
        assert 16 <= M <= 1024 and M & (M - 1) == 0 and 1 <= D <= M and 4 <= P <= 32          # inside the ranges create checked so far
    assert [c for c in cc.RUN if cc.lds_bytes(*c) > 64 * 1024] == [(256, 200, 32), (512, 400, 8), (1024, 128, 4)]
    assert [c for c in cc.RUN if c[0] > cc.CH_THREADS] == [(512, 400, 8), (1024, 128, 4)]


@pytest.mark.parametrize("case", cc.RUN, ids=cc.case_id)
def test_streams_are_what_the_sweep_says_they_are(case):
    M, D, P = case
    n = cc.stream_len(M, D, P)
    nf = cc.n_frames(n, D)
    assert nf > 3 * cc.CH_F and nf % cc.CH_F != 0 and cc.first_full_frame(M, D, P) < nf - 1
    a = cc.stream(M, D, P, "uniform")
    assert len(a) == 2 * n and a.min() == -32768 and a.max() == 32767
    assert {(-32768, 32767), (32767, -32768)} <= {(int(a[2 * i]), int(a[2 * i + 1])) for i in range(4)}
    # the impulse: every output is one tap times one phase, on both sides of the first workgroup edge
    b = cc.stream(M, D, P, "impulse")
    i0 = cc.impulse_index(M, D, P)
    assert np.count_nonzero(b) == 2 and i0 <= (cc.CH_F - 1) * D and i0 + M * P - 1 >= cc.CH_F * D
    y, _, _ = cc.expected(M, D, P, "impulse")
    h = cc.taps(M, P).astype(np.float64)
    for m in (cc.CH_F - 1, cc.CH_F):
        k = np.arange(M)
        want = h[m * D - i0] * (32767 - 32768j) / 32768.0 * np.exp(-2j * np.pi * ((k * i0) % M) / M)
        assert np.abs(y[:, m] - want).max() <= 1e-15
    # the tone: 0.9 on its channel once the filter is full, up to what rounding it to int16 moves; the image and DC channels in the stopband
    y, u_norm, a_norm = cc.expected(M, D, P, "tone")
    full = np.arange(cc.first_full_frame(M, D, P), nf)
    k0 = cc.tone_channel(M)
    tol = cc.bound(M, P, u_norm, a_norm)[full]
    assert np.abs(y[k0, full] - cc.TONE_AMP).max() <= cc.quant_allowance(M, P) + 2.0 ** -24
    level = cc.stopband_level(M, P)
    assert level < 1e-3                                                       # -59 dB below the tone or better: a real stopband
    for k in (M - k0, 0):
        assert (np.abs(y[k, full]) + tol <= level).all(), (k, np.abs(y[k, full]).max(), tol.max(), level)


@pytest.mark.parametrize("case", cc.RUN, ids=cc.case_id)
def test_cuts_cover_the_listed_calls_and_the_whole_stream(case):
    M, D, P = case
    T = M * P
    n = cc.cut_stream_len(M, D, P)
    seq = cc.cuts(M, D, P, n)
    assert sum(seq) == n and min(seq) >= 0
    k1 = min(D + 3, 260)
    assert seq[:k1] == [1] * k1 and seq[k1:k1 + 7] == [0, D - 1, D, D + 1, T - 2, T - 1, T]
    assert len(seq) == k1 + 9 and seq[-2] % 2 == 1 and seq[-1] > 0
    # single-sample calls run through the short-call history shift (n < T - 1), some of them complete no output sample (D > 1)
    assert 1 < T - 1
    pos, frames = 0, []
    for c in seq:
        frames.append(cc.n_frames(pos + c, D) - cc.n_frames(pos, D))
        pos += c
    assert sum(frames) == cc.n_frames(n, D)
    assert D == 1 or 0 in frames[1:k1]


# ------------------------------------------------------------------------------------------------------------ the bound bites, and is fair
def _model(case, xi, *, tap_shift=0, phase_from_block=False):
    """k_channelize in numpy float32, step for step: branch sums by fused multiply-add in tap order, the 2^-15 scale, the radix-2 decimation-in-time
    network with float32 twiddles, the phase factor from the same table.  tap_shift / phase_from_block build two wrong kernels."""
    M, D, P = case
    T = M * P
    h = cc.taps(M, P)
    hs = h[np.minimum(np.arange(T) + tap_shift, T - 1)]
    n = len(xi) // 2
    nf = cc.n_frames(n, D)
    xr = np.concatenate([np.zeros(T - 1), xi[0::2].astype(np.float64)])
    xq = np.concatenate([np.zeros(T - 1), xi[1::2].astype(np.float64)])
    m = np.arange(nf)
    r = np.arange(M)
    ur = np.zeros((nf, M), np.float32)
    ui = np.zeros((nf, M), np.float32)
    for p in range(P):
        idx = (T - 1) + m[:, None] * D - r[None, :] - p * M
        hp = hs[r + p * M].astype(np.float64)[None, :]
        ur = (hp * xr[idx] + ur.astype(np.float64)).astype(np.float32)         # a 24-bit tap times a 16-bit sample is exact in float64: one rounding
        ui = (hp * xq[idx] + ui.astype(np.float64)).astype(np.float32)
    s = np.float32(2.0 ** -15)
    log2m = M.bit_length() - 1
    rev = np.array([int(format(i, "0%db" % log2m)[::-1], 2) for i in range(M)])
    u = np.zeros((nf, M), np.complex64)
    u[:, rev] = (ur * s) + 1j * (ui * s)
    j = np.arange(M // 2)
    tw = (np.cos(2 * np.pi * j / M).astype(np.float32) + 1j * np.sin(2 * np.pi * j / M).astype(np.float32)).astype(np.complex64)
    for st in range(log2m):
        half = 1 << st
        pos, grp = j & (half - 1), j >> st
        i0 = (grp << (st + 1)) + pos
        i1 = i0 + half
        t = u[:, i1] * tw[pos << (log2m - 1 - st)][None, :]
        u[:, i0], u[:, i1] = u[:, i0] + t, u[:, i0] - t
    mm = (m // cc.CH_F * cc.CH_F if phase_from_block else m)
    idx = (r[None, :] * ((mm * D) % M)[:, None]) % M
    w = np.where(idx >= M // 2, -tw[idx & (M // 2 - 1)], tw[idx & (M // 2 - 1)])
    return (u * np.conj(w)).T


@pytest.mark.parametrize("case", cc.RUN, ids=cc.case_id)
def test_float32_model_sits_inside_the_bound_and_wrong_kernels_do_not(case):
    M, D, P = case
    xi = cc.stream(M, D, P, "uniform")
    y, u_norm, a_norm = cc.expected(M, D, P, "uniform")
    tol = cc.bound(M, P, u_norm, a_norm)
    ratio = (np.linalg.norm(_model(case, xi) - y, axis=0) / tol).max()
    print("%-16s float32 model: largest error / bound %.4f" % (cc.case_id(case), ratio))
    assert ratio <= 0.1                                   # the reference and the bound leave a correct float32 kernel a factor of ten
    # one tap index off by one
    assert (np.linalg.norm(_model(case, xi, tap_shift=1) - y, axis=0) / tol).min() > 1.0
    # the phase factor of the workgroup's first output sample for all sixteen: wrong wherever D is no multiple of M
    wrong = np.linalg.norm(_model(case, xi, phase_from_block=True) - y, axis=0) / tol
    if D % M:
        assert wrong[1::cc.CH_F].min() > 1.0 and wrong.max() > 100.0
