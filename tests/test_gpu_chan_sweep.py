"""Channelizer sweep: k_channelize (radiosonde_auto_rx_amd/csrc/sonde_chan.hip) against the float64 defining sum on EVERY output sample of EVERY
channel, over the shapes at which a different part of the kernel can go wrong, for every way the calls cut the stream, through both entries,
and the C receiver's row entries.  Cases, inputs and reference: tests/chan_cases.py (held to the direct sum by tests/test_chan_cases_design.py).

Tolerance, per output sample index m over all M channels (u_m: the float64 branch sums, A_m: their magnitude budget sum |h| |x|):

    ||y^_m - y_m||_2 <= 2^-24 sqrt(M) (8 log2(M) ||u_m||_2 + (P + 2) ||A_m||_2)

P fused multiply-adds per branch sum, +2 for the 2^-15 scale and the phase multiply, and the radix-2 float32 transform bound with the constant
tests/test_gpu_power.py uses.  The reference uses the kernel's float32 taps widened to float64, so tap rounding is no part of it.  The bound is not
to be widened to make a shape pass: a shape above it is a finding.  Measured ratios error / bound: profiles/chan_gpu_tolerances.txt.

The tone's channel is held to 0.9 within that bound plus what rounding the tone to int16 moves the float64 answer itself by (9.4e-6 at M = 16, where the
bound is 2.1e-6; no int16 tone reads 0.9 more closely); the reference supplies that figure and tests/test_chan_cases_design.py caps it at
2^-16 sqrt(2) sum|h|.  Against the reference the tone's channel is held to the bound alone, like every other.

Call cuts compare bits, not numbers: the arithmetic of an output sample depends neither on its place in a workgroup nor on the call that completes it.
The cut test draws its stream at chan_cases.cut_stream_len(): the listed calls alone are 4 D + 3 M P samples, more than M P + 48 D + 5 for most shapes.

Shapes whose LDS need is above what a workgroup may have are refused by sonde_chan_create; nothing here launches anything that is expected to fail."""
import re

import numpy as np
import pytest

import chan_cases as cc

pytestmark = pytest.mark.gpu
SR = 1_000_000
E_ARG, E_RANGE = -1, -4


def _code(fn, *args):
    """SONDE_E_* of a call that is expected to be refused (0 if it was not)"""
    from radiosonde_auto_rx_amd.engine import SondeError
    try:
        fn(*args)
    except SondeError as e:
        return int(re.search(r"\((-\d+)\)$", str(e)).group(1))
    return 0


def _run(case, xi, seq=None, *, device=False, refusals=False):
    """the stream xi through one channelizer in calls of seq samples (default: one call) -> (float32 [M][max_frames][2] as the device holds it behind a
    NaN fill, output samples per call).  device: process_device from a torch int16 tensor instead of process_host.  refusals: in front of every call
    one that is refused for its length and one that is refused for its out_stride."""
    import torch
    from radiosonde_auto_rx_amd.chan import Channelizer
    M, D, P = case
    n = len(xi) // 2
    seq = [n] if seq is None else seq
    max_chunk = n
    ch = Channelizer(SR, M, D, P, max_chunk=max_chunk)
    try:
        assert ch.taps == M * P and ch.max_frames == max_chunk // D + 2
        stride = ch.max_frames
        out = torch.full((M, stride, 2), float("nan"), dtype=torch.float32, device="cuda")
        wb = torch.from_numpy(np.concatenate([xi, np.zeros(2, np.int16)])).to("cuda") if device else None
        torch.cuda.synchronize()                 # the fill and the copy run on torch's stream, the channelizer on its own: order them
        too_long = np.zeros(2 * (max_chunk + 1), np.int16)
        pos, got, counts = 0, 0, []
        for take in seq:
            want = cc.n_frames(pos + take, D) - got
            dst = out.data_ptr() + 8 * got

            def call(n_s, dst=dst, stride=stride, pos=pos):
                if device:
                    return ch.process_device(wb.data_ptr() + 4 * pos, n_s, dst, stride)
                return ch.process_host(xi[2 * pos:2 * (pos + n_s)], dst, stride)
            if refusals:
                if device:
                    assert _code(ch.process_device, wb.data_ptr(), max_chunk + 1, dst, stride) == E_RANGE
                else:
                    assert _code(ch.process_host, too_long, dst, stride) == E_RANGE
                if want > 0:
                    assert _code(call, take, dst, want - 1) == E_RANGE
            k = call(take)
            assert k == want, (pos, take, k, want)
            counts.append(k)
            pos += take
            got += k
        assert pos == n
        ch.sync()
        return out.cpu().numpy(), counts
    finally:
        ch.close()


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _complex(raw, nf):
    return raw[:, :nf, 0].astype(np.float64) + 1j * raw[:, :nf, 1].astype(np.float64)


@pytest.mark.parametrize("case", cc.RUN, ids=cc.case_id)
def test_every_frame_every_channel_against_float64(case):
    M, D, P = case
    n = cc.stream_len(M, D, P)
    nf = cc.n_frames(n, D)
    ratios = {}
    for kind in cc.INPUTS:
        raw, counts = _run(case, cc.stream(M, D, P, kind))
        assert counts == [nf]
        assert np.isfinite(raw[:, :nf]).all() and np.isnan(raw[:, nf:]).all(), kind         # nothing written behind the count
        y, u_norm, a_norm = cc.expected(M, D, P, kind)
        tol = cc.bound(M, P, u_norm, a_norm)
        got = _complex(raw, nf)
        err = np.linalg.norm(got - y, axis=0)
        # where the bound is 0 (the impulse: output samples whose taps miss the lone sample) the output has to be exactly 0: any error there is infinite
        ratios[kind] = float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))))
        if kind == "tone":
            full = np.arange(cc.first_full_frame(M, D, P), nf)
            k0 = cc.tone_channel(M)
            own = np.abs(y[k0, full] - cc.TONE_AMP).max()         # what rounding the tone to int16 moves the float64 answer by (design test: <= 2^-16 sqrt2 sum|h|)
            tone_err = np.abs(got[k0, full] - cc.TONE_AMP)
            image = max(np.abs(got[M - k0, full]).max(), np.abs(got[0, full]).max())
            level = cc.stopband_level(M, P)
            print("%-16s tone: channel %d reads 0.9 within %.2e (bound %.2e + %.2e of the int16 tone)   channels %d and 0 at most %.2e (stopband %.2e)"
                  % (cc.case_id(case), k0, tone_err.max(), tol[full].min(), own, M - k0, image, level))
            assert (tone_err <= tol[full] + own).all(), (case, tone_err.max())
            assert image <= level, (case, image, level)
        if (err > tol).any():
            m = int(np.argmax(err - tol))
            print("%-16s %s: output sample %d of %d: error %.3e, bound %.3e" % (cc.case_id(case), kind, m, nf, err[m], tol[m]))
        assert (err <= tol).all(), (case, kind, int(np.count_nonzero(err > tol)), ratios[kind])
    print("%-16s LDS %6d B   %3d output samples x %4d channels   largest error / bound: uniform %.4f  impulse %.4f  tone %.4f"
          % (cc.case_id(case), cc.lds_bytes(M, D, P), nf, M, ratios["uniform"], ratios["impulse"], ratios["tone"]))
    assert max(ratios.values()) <= 1.0, (case, ratios)


@pytest.mark.parametrize("case", cc.RUN, ids=cc.case_id)
def test_call_cuts_and_both_entries_give_the_same_bits(case):
    M, D, P = case
    n = cc.cut_stream_len(M, D, P)
    xi = cc.stream(M, D, P, "uniform", n)
    seq = cc.cuts(M, D, P, n)
    whole, _ = _run(case, xi)
    nf = cc.n_frames(n, D)
    assert np.isfinite(whole[:, :nf]).all() and np.isnan(whole[:, nf:]).all()
    host, counts_h = _run(case, xi, seq)
    assert sum(counts_h) == nf
    assert _same_bits(host, whole), np.argwhere(host.view(np.uint32) != whole.view(np.uint32))[:4]
    dev, counts_d = _run(case, xi, seq, device=True)
    assert counts_d == counts_h
    assert _same_bits(dev, host), np.argwhere(dev.view(np.uint32) != host.view(np.uint32))[:4]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refused_calls_leave_the_state_alone(device):
    case = (128, 77, 6)
    M, D, P = case
    xi = cc.stream(M, D, P, "uniform")
    n = len(xi) // 2
    seq = [D + 1, 5, M * P - 2, n - (D + 1) - 5 - (M * P - 2)]           # short calls, a call that completes no output sample, long calls
    plain, counts = _run(case, xi, seq, device=device)
    assert 0 in counts
    refused, counts_r = _run(case, xi, seq, device=device, refusals=True)
    assert counts_r == counts and _same_bits(refused, plain)
    whole, _ = _run(case, xi)
    assert _same_bits(plain, whole)


@pytest.mark.parametrize("case", cc.REFUSED, ids=cc.case_id)
def test_shape_beyond_the_lds_is_refused_at_create(case, capfd):
    from radiosonde_auto_rx_amd.chan import Channelizer
    M, D, P = case
    assert _code(lambda: Channelizer(SR, M, D, P, max_chunk=4096)) == E_ARG
    assert "%d bytes of LDS" % cc.lds_bytes(M, D, P) in capfd.readouterr().err


def test_row_entries_of_the_c_receiver():
    """sonde_chan_output / sonde_chan_rows_alloc / sonde_chan_gather: the arrays are the library's, so they are read back with gather itself, into a torch
    tensor laid out as rows ([n][max_frames] complex64)"""
    import torch
    from radiosonde_auto_rx_amd.chan import Channelizer
    case = (64, 48, 8)
    M, D, P = case
    xi = cc.stream(M, D, P, "uniform")
    n = len(xi) // 2
    nf = cc.n_frames(n, D)
    whole, _ = _run(case, xi)
    ch = Channelizer(SR, M, D, P, max_chunk=n)
    try:
        own, stride = ch.output()
        assert own and stride == ch.max_frames and ch.output() == (own, stride)
        assert ch.process_host(xi, own, stride) == nf
        back = torch.full((M, stride, 2), float("nan"), dtype=torch.float32, device="cuda")
        rows_back = torch.full((4, stride, 2), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ch.gather(own, stride, list(range(M)), nf, back.data_ptr())
        chans = [5, -1, 63, 0]
        rows = ch.rows_alloc(4)
        assert rows and rows != own
        ch.gather(own, stride, chans, nf, rows)
        ch.gather(rows, stride, [0, 1, 2, 3], stride, rows_back.data_ptr())
        assert _code(ch.gather, own, stride, [5, M], nf, rows) == E_RANGE
        assert _code(ch.gather, own, stride, chans, stride + 1, rows) == E_ARG
        ch.sync()
        back, rows_back = back.cpu().numpy(), rows_back.cpu().numpy()
        assert _same_bits(back[:, :nf], whole[:, :nf])                    # the owned array holds what a caller's array holds
        assert np.isnan(back[:, nf:]).all()                               # gather copies n_frames samples of a row, no more
        for r, k in enumerate(chans):
            if k < 0:
                assert (rows_back[r].view(np.uint32) == 0).all()         # the row not in use stays as rows_alloc zeroed it
            else:
                assert _same_bits(rows_back[r, :nf], whole[k, :nf])
                assert (rows_back[r, nf:].view(np.uint32) == 0).all()
    finally:
        ch.close()


def test_a_smaller_channelizer_created_later_leaves_a_larger_one_running():
    """the dynamic-LDS attribute belongs to (kernel, device), not to a channelizer: one of 155 136 B still launches, with the same bits, after one of 77 536 B was created"""
    import torch
    from radiosonde_auto_rx_amd.chan import Channelizer
    big, small = (1024, 128, 4), (256, 200, 32)
    xi = cc.stream(*big, "uniform")
    n = len(xi) // 2
    alone, _ = _run(big, xi)
    a = Channelizer(SR, *big, max_chunk=n)
    b = Channelizer(SR, *small, max_chunk=n)
    try:
        out = torch.full((big[0], a.max_frames, 2), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert a.process_host(xi, out.data_ptr(), a.max_frames) == cc.n_frames(n, big[1])
        a.sync()
        assert _same_bits(out.cpu().numpy(), alone)
    finally:
        a.close()
        b.close()
