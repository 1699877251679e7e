"""IF chain sweep: every IF-filtered IQ, FM and tone-correlator sample of k_if_chain / k_if_chain_multi against the CPU oracle and against a float64
model of the chain, at every shape where the kernel takes another path (tests/if_chain_cases.py lists them and what each selects;
tests/test_if_chain_cases_design.py keeps model and table honest without a GPU).

Inputs are generated from seeds; nothing outside the repository is read (liboracle.so is built from oracle/*.c).  Per case 0.15 s of IF-rate IQ
(0.05 s at 384 kHz): at most 28 800 samples.

Bounds, on EVERY sample of every case, channel and way of cutting the stream into calls:
  against the oracle (the project's own, tests/test_gpu_parity.py) ... IF IQ 1e-6 RMS and 2e-5 max-abs, fm 1e-6 RMS, bufs 1e-5 RMS
  new: fm and bufs by max-abs against the oracle ..................... 2e-5, the bound the IQ streams have (one wrong sample at a tile, call or ring
                                                                        edge is 5e-4 or more; a flipped signed-zero sample is 0.8)
  new: against the float64 model, RMS and max-abs separately .......... GPU - model <= 3 x (oracle - model, same samples) + floor; the factor is the one
                                                                        test_gpu_parity.py and the decimator sweep apply to the reference's own floor
The floors are what the kernel's documented primitives add where the reference computes in double (FLOOR below, derivation beside it); all of them
are below 7e-7, a tenth of the smallest effect (7e-5) of the wrong kernels the design test and the list below stand for.

Measured on an MI355X, one call per case, seed 7 ("- f64": deviation from the float64 model, GPU / oracle; each cell RMS / max-abs).  DESIGN.md §2a has the same table.
  case                            stream GPU - oracle        GPU - f64           oracle - f64        ratio
  rs41                            IF IQ  2.79e-08 / 1.79e-07 3.18e-08 / 1.76e-07 3.13e-08 / 2.07e-07 1.02 / 0.85
                                  fm     2.18e-08 / 1.42e-07 2.39e-08 / 1.12e-07 2.31e-08 / 1.20e-07 1.03 / 0.93
                                  bufs   3.55e-07 / 1.18e-06 2.54e-08 / 9.60e-08 3.54e-07 / 1.18e-06 0.07 / 0.08
  rs41_50k_lpfm                   IF IQ  2.82e-08 / 2.09e-07 3.21e-08 / 1.65e-07 3.13e-08 / 1.86e-07 1.03 / 0.89
                                  fm     7.64e-09 / 3.35e-08 7.84e-09 / 4.08e-08 7.69e-09 / 5.98e-08 1.02 / 0.68
                                  bufs   4.40e-07 / 1.49e-06 2.67e-08 / 1.02e-07 4.39e-07 / 1.49e-06 0.06 / 0.07
  dfm                             IF IQ  2.49e-08 / 1.49e-07 2.77e-08 / 1.46e-07 2.77e-08 / 1.46e-07 1.00 / 1.00
                                  fm     2.11e-08 / 1.12e-07 2.17e-08 / 1.05e-07 2.09e-08 / 1.05e-07 1.04 / 1.00
                                  bufs   4.53e-07 / 1.22e-06 2.90e-08 / 1.21e-07 4.50e-07 / 1.28e-06 0.06 / 0.09
  m10                             IF IQ  2.19e-08 / 2.98e-07 2.28e-08 / 1.57e-07 2.38e-08 / 1.73e-07 0.96 / 0.91
                                  fm     2.08e-08 / 1.04e-07 1.99e-08 / 9.07e-08 1.87e-08 / 8.47e-08 1.06 / 1.07
                                  bufs   4.32e-07 / 1.15e-06 2.49e-08 / 1.01e-07 4.32e-07 / 1.11e-06 0.06 / 0.09
  edge_B                          IF IQ  2.82e-08 / 1.49e-07 3.17e-08 / 1.58e-07 3.11e-08 / 2.00e-07 1.02 / 0.79
                                  fm     2.17e-08 / 1.24e-07 2.37e-08 / 1.03e-07 2.30e-08 / 1.26e-07 1.03 / 0.82
                                  bufs   3.62e-07 / 9.69e-07 4.31e-08 / 1.91e-07 3.61e-07 / 9.83e-07 0.12 / 0.19
  edge_A                          IF IQ  2.82e-08 / 1.79e-07 3.19e-08 / 1.79e-07 3.15e-08 / 2.10e-07 1.01 / 0.85
                                  fm     2.13e-08 / 1.34e-07 2.33e-08 / 1.07e-07 2.33e-08 / 1.36e-07 1.00 / 0.79
                                  bufs   3.34e-07 / 7.75e-07 4.87e-08 / 1.83e-07 3.31e-07 / 8.13e-07 0.15 / 0.23
  edge_B3                         IF IQ  2.79e-08 / 1.79e-07 3.18e-08 / 1.57e-07 3.14e-08 / 2.09e-07 1.01 / 0.75
                                  fm     3.91e-09 / 1.86e-08 4.24e-09 / 7.59e-08 4.05e-09 / 7.59e-08 1.05 / 1.00
                                  bufs   1.87e-07 / 6.41e-07 4.55e-08 / 1.75e-07 1.82e-07 / 6.25e-07 0.25 / 0.28
  edge_A3                         IF IQ  2.81e-08 / 1.79e-07 3.22e-08 / 1.50e-07 3.16e-08 / 2.16e-07 1.02 / 0.70
                                  fm     3.72e-09 / 2.24e-08 4.17e-09 / 5.03e-08 3.95e-09 / 3.71e-08 1.06 / 1.36
                                  bufs   4.02e-07 / 1.49e-06 4.55e-08 / 1.77e-07 3.98e-07 / 1.44e-06 0.11 / 0.12
  wide96                          IF IQ  3.74e-08 / 2.38e-07 4.45e-08 / 2.56e-07 4.30e-08 / 3.03e-07 1.03 / 0.84
                                  fm     2.59e-09 / 2.98e-08 2.74e-09 / 7.01e-08 2.75e-09 / 6.60e-08 0.99 / 1.06
                                  bufs   4.86e-07 / 1.85e-06 4.74e-08 / 1.73e-07 4.87e-07 / 1.79e-06 0.10 / 0.10
  wide192                         IF IQ  5.02e-08 / 4.47e-07 6.22e-08 / 3.42e-07 6.10e-08 / 4.14e-07 1.02 / 0.83
                                  fm     2.22e-09 / 1.49e-08 2.13e-09 / 3.37e-08 2.14e-09 / 2.71e-08 0.99 / 1.25
                                  bufs   7.63e-07 / 1.95e-06 4.92e-08 / 1.89e-07 7.59e-07 / 1.93e-06 0.06 / 0.10
  iq0                             IF IQ  2.79e-08 / 1.79e-07 3.18e-08 / 1.76e-07 3.13e-08 / 2.07e-07 1.02 / 0.85
                                  fm     7.33e-09 / 4.47e-08 7.33e-09 / 5.05e-08 7.34e-09 / 4.08e-08 1.00 / 1.24
                                  bufs   7.33e-09 / 4.47e-08 7.33e-09 / 5.05e-08 7.34e-09 / 4.08e-08 1.00 / 1.24
  nolp                            IF IQ  0.00e+00 / 0.00e+00 0.00e+00 / 0.00e+00 0.00e+00 / 0.00e+00 0.00 / 0.00
                                  fm     8.52e-09 / 2.98e-08 9.30e-09 / 5.06e-08 5.96e-09 / 3.07e-08 1.56 / 1.65
                                  bufs   2.51e-07 / 7.60e-07 2.39e-08 / 8.76e-08 2.50e-07 / 7.44e-07 0.10 / 0.12
  zeros8                          IF IQ  0.00e+00 / 0.00e+00 -                   -                   -
                                  fm     2.40e-08 / 5.96e-08 -                   -                   -
                                  bufs   2.40e-08 / 5.96e-08 -                   -                   -
  big                             IF IQ  6.88e-08 / 4.77e-07 8.61e-08 / 4.61e-07 8.42e-08 / 5.56e-07 1.02 / 0.83
                                  fm     2.53e-09 / 1.21e-08 2.49e-09 / 2.91e-08 2.48e-09 / 3.05e-08 1.00 / 0.96
                                  bufs   6.29e-07 / 1.71e-06 4.97e-08 / 2.17e-07 6.27e-07 / 1.61e-06 0.08 / 0.14
  rs41 ring wrap                  IF IQ  2.77e-08 / 2.09e-07 3.13e-08 / 1.77e-07 3.10e-08 / 2.02e-07 1.01 / 0.88
                                  fm     2.16e-08 / 1.34e-07 2.33e-08 / 1.28e-07 2.31e-08 / 1.48e-07 1.01 / 0.86
                                  bufs   9.65e-07 / 2.50e-06 2.57e-08 / 1.10e-07 9.65e-07 / 2.48e-06 0.03 / 0.04
  rs41 ring wrap, 32768 +- 59     IF IQ  2.78e-08 / 1.04e-07 3.00e-08 / 1.06e-07 3.39e-08 / 1.29e-07 0.89 / 0.82
                                  fm     2.02e-08 / 6.71e-08 2.22e-08 / 6.61e-08 2.46e-08 / 8.15e-08 0.91 / 0.81
                                  bufs   9.76e-07 / 1.76e-06 2.57e-08 / 6.96e-08 9.79e-07 / 1.74e-06 0.03 / 0.04
  rs41 3 channels, ch 0           IF IQ  2.75e-08 / 1.79e-07 3.15e-08 / 1.54e-07 3.10e-08 / 1.85e-07 1.02 / 0.83
                                  fm     2.16e-08 / 1.45e-07 2.41e-08 / 1.26e-07 2.33e-08 / 1.37e-07 1.04 / 0.92
                                  bufs   3.04e-07 / 9.98e-07 2.54e-08 / 1.07e-07 3.03e-07 / 9.82e-07 0.08 / 0.11
  rs41 3 channels, ch 2           IF IQ  2.77e-08 / 1.79e-07 3.12e-08 / 1.53e-07 3.09e-08 / 2.29e-07 1.01 / 0.67
                                  fm     2.16e-08 / 1.19e-07 2.28e-08 / 1.19e-07 2.30e-08 / 1.34e-07 0.99 / 0.88
                                  bufs   3.42e-07 / 9.24e-07 2.68e-08 / 1.16e-07 3.42e-07 / 9.10e-07 0.08 / 0.13
  rs41 3 channels, ch 1 before    IF IQ  2.77e-08 / 1.79e-07 3.15e-08 / 1.57e-07 3.09e-08 / 1.87e-07 1.02 / 0.84
                                  fm     2.20e-08 / 1.15e-07 2.33e-08 / 1.08e-07 2.30e-08 / 1.03e-07 1.01 / 1.05
                                  bufs   2.18e-07 / 7.15e-07 2.60e-08 / 8.49e-08 2.15e-07 / 7.33e-07 0.12 / 0.12
  rs41 3 channels, ch 1 restarted IF IQ  2.77e-08 / 1.79e-07 3.10e-08 / 1.62e-07 3.11e-08 / 2.15e-07 1.00 / 0.75
                                  fm     2.22e-08 / 1.23e-07 2.38e-08 / 1.03e-07 2.38e-08 / 1.30e-07 1.00 / 0.80
                                  bufs   2.86e-07 / 1.04e-06 2.52e-08 / 8.61e-08 2.85e-07 / 1.04e-06 0.09 / 0.08
  2400k rs41                      IF IQ  4.35e-08 / 2.38e-07 3.11e-08 / 1.56e-07 3.09e-08 / 1.85e-07 1.00 / 0.84
                                  fm     2.55e-08 / 2.38e-07 2.35e-08 / 1.26e-07 2.35e-08 / 1.21e-07 1.00 / 1.04
                                  bufs   5.21e-07 / 1.45e-06 2.54e-08 / 1.21e-07 5.19e-07 / 1.39e-06 0.05 / 0.09
  2400k dfm                       IF IQ  4.80e-08 / 2.38e-07 2.76e-08 / 1.34e-07 2.79e-08 / 1.89e-07 0.99 / 0.71
                                  fm     2.69e-08 / 1.12e-07 2.20e-08 / 1.07e-07 2.11e-08 / 1.17e-07 1.04 / 0.91
                                  bufs   2.23e-07 / 5.96e-07 2.80e-08 / 1.21e-07 2.19e-07 / 5.98e-07 0.13 / 0.20
  2400k m10                       IF IQ  6.04e-08 / 3.28e-07 2.24e-08 / 1.19e-07 2.31e-08 / 1.30e-07 0.97 / 0.92
                                  fm     4.65e-08 / 2.98e-07 1.93e-08 / 9.28e-08 1.84e-08 / 9.41e-08 1.05 / 0.99
                                  bufs   3.07e-07 / 8.64e-07 2.26e-08 / 9.69e-08 3.04e-07 / 8.43e-07 0.07 / 0.11
  mixed ch 0 rs41                 bufs   5.21e-07 / 1.45e-06 2.54e-08 / 1.21e-07 5.19e-07 / 1.39e-06 0.05 / 0.09
  mixed ch 1 dfm                  bufs   2.23e-07 / 5.96e-07 2.80e-08 / 1.21e-07 2.19e-07 / 5.98e-07 0.13 / 0.20
  mixed ch 2 rs41                 bufs   4.74e-07 / 1.42e-06 2.59e-08 / 9.23e-08 4.73e-07 / 1.38e-06 0.05 / 0.07
  mixed ch 3 m10                  bufs   3.07e-07 / 8.64e-07 2.26e-08 / 9.69e-08 3.04e-07 / 8.43e-07 0.07 / 0.11
  mixed ch 4 dfm                  bufs   3.33e-07 / 8.94e-07 2.85e-08 / 1.17e-07 3.31e-07 / 8.64e-07 0.09 / 0.14
Wrong kernels tried aside (one run each, not committed) and what failed with them:
  odd tail tap of the IF FIR skipped ........ test_case of every case with an IF low-pass, every cut, ring, restart and refusal test, base-rate rs41, mixed
                                              (IF IQ 2.0e-5 RMS at 48 kHz ... 2.5e-6 at 384 kHz; dfm / m10, whose last tap is 1e-20: fm off by 0.8 at sample 0,
                                              the sign of a zero)
  tone run's full sum from j = nwin - 2 ..... every test but test_case[iq0] and [zeros8], which have no tone correlator
  if_chain_xlo without rounding to IF_NB .... no test of this file: the two entries it leaves unwritten are read only by sums that are formed and not stored, and
                                              leave the running sum again.  The layout rule moves: tests/test_if_chain_cases_design.py::
                                              test_row_selects_what_it_claims[edge_B3] and [edge_A3] fail against that library
  tone phase from m instead of m - ep ....... no bound: |F| does not see a common rotation (test_the_tone_phase_origin_does_not_enter_bufs of the design
                                              test).  test_restart_on_a_run_boundary_is_a_fresh_engine_to_the_bit is there for it
"""
import functools

import numpy as np
import pytest
import if_chain_cases as K

pytestmark = pytest.mark.gpu

# Floors of the float64 comparison: (RMS, max-abs) the kernel may add to 3 x the reference's own deviation.
#   IF IQ: 1e-8, the decimator sweep's (_check_exact): the kernel forms the same float32 fused multiply-adds as the reference's sum, in another order.
#   fm:    the reference evaluates atan2 in double and rounds once; the kernel calls atan2f (2 ulp at |angle| <= pi: 2 x 2.4e-7 rad) and scales it by
#          0.8 and 1 / pi in float32 (two roundings of a value below 0.8, 3e-8 each): 4.8e-7 x 0.8 / pi + 6e-8 = 1.8e-7.  Behind the FM low-pass the
#          error is a weighted mean with sum |w| <= 1.5: 2.7e-7.  RMS: a third of that (errors spread evenly inside +- the bound give bound / sqrt 3).
#   bufs:  the reference forms its phasors with cos / sin in double; the kernel reduces the phase to a float32 fraction of a turn (half an ulp below
#          1: 2^-25 turns = 1.9e-7 rad) and takes the hardware sine and cosine (2e-7 absolute each): a term z e^{i phi} is off by at most
#          |z| (sqrt 2 x 2e-7 + 1.9e-7) = 4.7e-7 |z|.  A window has nwin = (int)sps terms, both tone sums take the error, and the result is scaled by
#          1 / sps: 2 x (nwin / sps) x 0.55 x 4.7e-7 = 5.2e-7 at |z| <= 0.55 (0.35 signal, what the filter leaves of the interferer, 4 sigma of noise);
#          the two hardware square roots (1 ulp of |F| <= nwin |z|, over sps: 6e-8 each) bring it to 6.4e-7.  RMS: the phasor errors of a window add
#          like a random walk, sqrt nwin / sps <= 0.45 of the worst case, and the roots' rounding is 3.5e-8 each: below 1e-7.
#          The float32 additions of the window sums are not in the floor: the reference adds in float32 too (its recursive sums), they are in its own figure.
#   --iq0: bufs is the fm stream, with fm's floor.
FLOOR = dict(ifiq=(1e-8, 1e-8), fm=(1e-7, 2.7e-7), bufs=(1e-7, 6.4e-7))
ORACLE_BOUND = dict(ifiq=(1e-6, 2e-5), fm=(1e-6, 2e-5), bufs=(1e-5, 2e-5))
CUTS = [1, 3, 957, 959, 960, 961, 2, 1919, 4]                  # call starts off and on multiples of 4 (koff, scalar and float4 stores), tiles +- 1; then the rest
TAPS = ("ifiq", "fm", "bufs")


# ----------------------------------------------------------------------------------------------- references (computed once, shared, read-only)
def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _ref(cid, seed, n=None, first=0):
    """oracle streams and float64 model of samples [first, n) of signal(cid, seed, n), as a stream of their own"""
    from oracle import bind
    c = K.BY_ID[cid]
    x = K.signal(cid, seed, n)[2 * first:]
    o = bind.ora_streams(x, c["sr"], **K.oracle_kw(c))
    assert o["n"] == len(x) // 2
    ref = _frozen(dict(ifiq=o["iq"], fm=o["fm"], bufs=o["bufs"], consts=o["consts"]))
    mod = None if cid == "zeros8" else _frozen(K.model(c, K.samples_of(x, c["bits"])))
    return ref, mod


def _check(tag, got, ref, mod, sl=slice(None), floor_of=None):
    """every bound of the module docstring on the samples sl of one channel; prints every figure first.  mod None: oracle only"""
    g = {k: np.asarray(v)[sl] for k, v in got.items()}
    r = {k: ref[k][sl] for k in g}
    go = K.figures(g, r)
    line = "IFSWEEP %-30s" % tag
    gm = om = None
    if mod is not None:
        m = {k: mod[k][sl] for k in g}
        gm, om = K.figures(g, m), K.figures(r, m)
    for k in go:
        line += "  %s gpu-oracle %.2e/%.2e" % (k, *go[k])
        if gm:
            line += " gpu-f64 %.2e/%.2e oracle-f64 %.2e/%.2e ratio %.2f/%.2f" % (*gm[k], *om[k], gm[k][0] / max(om[k][0], 1e-30), gm[k][1] / max(om[k][1], 1e-30))
    print(line)
    for k in go:
        assert go[k][0] < ORACLE_BOUND[k][0] and go[k][1] < ORACLE_BOUND[k][1], (tag, k, "against the oracle", go[k])
    if gm:
        for k in gm:
            fl = FLOOR[(floor_of or {}).get(k, k)]
            assert gm[k][0] <= 3 * om[k][0] + fl[0], (tag, k, "RMS against the float64 model", gm[k], om[k])
            assert gm[k][1] <= 3 * om[k][1] + fl[1], (tag, k, "max-abs against the float64 model", gm[k], om[k])
    return go, gm, om


def _floor_of(c):
    return {"bufs": "fm"} if c["iq"] == 0 else None


# ----------------------------------------------------------------------------------------------- the engine
def _read(eng, ch, first, count, names=TAPS):
    from radiosonde_auto_rx_amd import engine as E
    tap = dict(dec=E.TAP_DECIM, ifiq=E.TAP_IFIQ, fm=E.TAP_FM, bufs=E.TAP_BUFS)
    return {k: eng.read_tap(ch, tap[k], first, count) for k in names}


def _run(cid, X, calls=None, **over):
    """an engine of the case's shape fed X ([2n] or [channels, 2n]) in the given call lengths (+ the rest) -> (info, [per channel {tap: array}])"""
    from radiosonde_auto_rx_amd import engine as E
    c = K.BY_ID[cid]
    X = np.asarray(X)
    n_ch = 1 if X.ndim == 1 else X.shape[0]
    n = X.shape[-1] // 2
    eng = E.Engine([0.0] * n_ch, c["sr"], max_chunk=n, **dict(K.engine_kw(c), **over))
    try:
        pos = 0
        for b in list(calls or []) + [n - sum(calls or [])]:
            assert b > 0
            eng.process_host(X[..., 2 * pos:2 * (pos + b)])
            pos += b
        assert pos == n <= eng.info["ring_len"]
        return dict(eng.info), [_read(eng, ch, 0, n) for ch in range(n_ch)]
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _one_call(cid):
    info, got = _run(cid, K.signal(cid, 7))
    return info, _frozen(got[0])


# ----------------------------------------------------------------------------------------------- every case, one call
@pytest.mark.parametrize("cid", [c["id"] for c in K.CASES])
def test_case(oracle, cid):
    """the table's shapes in one call each: the filters the table claims, the three streams against the oracle and (but zeros8) the float64 model.
    Case big launches with 72 624 bytes of dynamic LDS, announced when the engine was created."""
    c = K.BY_ID[cid]
    ref, mod = _ref(cid, 7)
    info, got = _one_call(cid)
    assert (info["lpiq_taps"] or 1, info["lpfm_taps"] or 1, info["if_sr"], info["decM"], int(info["sps"])) == (c["T1"], c["T2"], c["sr"], 1, c["nwin"])
    assert (info["lpiq_taps"], info["lpfm_taps"], info["L"], info["M"]) == tuple(ref["consts"][k] for k in ("lpiq_taps", "lpfm_taps", "L", "M"))
    _check(cid, got, ref, mod, floor_of=_floor_of(c))


@pytest.mark.parametrize("cid", ["rs41", "rs41_50k_lpfm", "edge_B", "edge_A", "wide96"])
def test_call_cuts_give_the_same_bits(oracle, cid):
    c = K.BY_ID[cid]
    ref, mod = _ref(cid, 7)
    _, one = _one_call(cid)
    _, got = _run(cid, K.signal(cid, 7), calls=CUTS)
    for k in TAPS:
        bad = np.flatnonzero((got[0][k] != one[k]).reshape(len(one[k]), -1).any(axis=1))
        assert bad.size == 0, (cid, k, "first differing IF samples", bad[:8], "of", bad.size)
    _check("%s cut" % cid, got[0], ref, mod, floor_of=_floor_of(c))


def test_ring_wrap(oracle):
    """40 000 samples through a ring of 32 768 in 2048-sample calls, each call's taps read right after it: the same bounds over the whole stream, and
    on the samples whose filter and window history straddle the wrap"""
    from radiosonde_auto_rx_amd import engine as E
    c = K.BY_ID["rs41"]
    n, step = 40_000, 2048
    x = K.signal("rs41", 21, n)
    ref, mod = _ref("rs41", 21, n)
    eng = E.Engine([0.0], c["sr"], max_chunk=step, **K.engine_kw(c))
    try:
        assert eng.info["ring_len"] == 32_768
        parts = []
        for pos in range(0, n, step):
            b = min(step, n - pos)
            eng.process_host(x[2 * pos:2 * (pos + b)])
            parts.append(_read(eng, 0, pos, b))
    finally:
        eng.close()
    got = {k: np.concatenate([p[k] for p in parts]) for k in TAPS}
    _check("rs41 ring wrap", got, ref, mod)
    w = c["T1"] + c["nwin"]
    _check("rs41 ring wrap, 32768 +- %d" % w, got, ref, mod, sl=slice(32_768 - w, 32_768 + w))


def test_three_channels_one_restarted(oracle):
    """three seeds in one engine; channel 1 is restarted before a call that begins at IF sample 2501 (no multiple of 4 or 960): from there it equals the
    model of the samples fed from there — phase origin and zero history at the restart — and its neighbours carry on inside the bounds"""
    from radiosonde_auto_rx_amd import engine as E
    c = K.BY_ID["rs41"]
    n, cut = 7200, 2501
    seeds = (31, 32, 33)
    X = np.stack([K.signal("rs41", s, n) for s in seeds]).copy()
    X[1, 2 * cut:] = K.signal("rs41", 34, n)[2 * cut:]          # channel 1's second stream
    eng = E.Engine([0.0] * 3, c["sr"], max_chunk=n, **K.engine_kw(c))
    try:
        eng.process_host(X[:, :2 * cut])
        before = _read(eng, 1, 0, cut)
        eng.restart_channel(1)
        eng.process_host(X[:, 2 * cut:])
        got = [_read(eng, ch, 0, n) for ch in range(3)]
    finally:
        eng.close()
    for ch in (0, 2):
        _check("rs41 3 channels, ch %d" % ch, got[ch], *_ref("rs41", seeds[ch], n))
    _check("rs41 3 channels, ch 1 before", before, *_ref("rs41", seeds[1], n), sl=slice(0, cut))
    after = {k: v[cut:] for k, v in got[1].items()}
    _check("rs41 3 channels, ch 1 restarted", after, *_ref("rs41", 34, n, cut))


def test_restart_on_a_run_boundary_is_a_fresh_engine_to_the_bit(oracle):
    """a restart at IF sample 2504 (a multiple of IF_RUN, so the tone runs lie as in a stream that starts there; no multiple of the tile): with the phase
    origin and the zero history at the restart every operation is the one a fresh engine performs on the same samples — the same bits in all three
    streams.  (The origin does not enter |F|, so the bounds alone cannot see a phase counted from the engine's start: the last bits can.)"""
    from radiosonde_auto_rx_amd import engine as E
    c = K.BY_ID["rs41"]
    n, cut = 7200, 2504
    X = np.stack([K.signal("rs41", 31, n), K.signal("rs41", 32, n)]).copy()
    X[1, 2 * cut:] = K.signal("rs41", 34, n)[2 * cut:]
    eng = E.Engine([0.0] * 2, c["sr"], max_chunk=n, **K.engine_kw(c))
    try:
        eng.process_host(X[:, :2 * cut])
        eng.restart_channel(1)
        eng.process_host(X[:, 2 * cut:])
        got = _read(eng, 1, cut, n - cut)
    finally:
        eng.close()
    _, fresh = _run("rs41", X[1, 2 * cut:])
    for k in TAPS:
        bad = np.flatnonzero((got[k] != fresh[0][k]).reshape(n - cut, -1).any(axis=1))
        assert bad.size == 0, (k, "first differing samples behind the restart", bad[:8], "of", bad.size)
    _check("rs41 restarted at 2504", got, *_ref("rs41", 34, n, cut))


# ----------------------------------------------------------------------------------------------- LDS need decided at create
def test_lds_need_above_the_device_limit_is_refused_at_create(oracle):
    """1.5 Msps IF with both low-passes needs 182 720 bytes of LDS per workgroup: sonde_engine_create_generic returns SONDE_E_ARG (an argument check,
    nothing is launched), and the process goes on: the next engine passes case rs41"""
    from radiosonde_auto_rx_amd import engine as E
    c = dict(K.BY_ID["rs41"], lp_fm=True)
    with pytest.raises(E.SondeError) as ei:
        E.Engine([0.0], K.REFUSED["sr"], max_chunk=4096, **K.engine_kw(c))
    assert "(-1)" in str(ei.value) and E.lib().sonde_strerror(-1).decode() in str(ei.value)
    _, got = _run("rs41", K.signal("rs41", 7))
    _check("rs41 after the refusal", got[0], *_ref("rs41", 7))


# ----------------------------------------------------------------------------------------------- base-rate and mixed engines
FQ = dict(rs41=(0.1234, -0.31), dfm=(0.27, -0.07), m10=(-0.2, 0.41))


@functools.lru_cache(maxsize=None)
def _base_ref(kind, seed, fq):
    """the oracle's streams behind its own decimator, and the model run on the oracle's decimated IQ"""
    from oracle import bind
    c = K.BASE[kind]
    x = K.signal_base(kind, seed, fq)
    kw = dict(fq=fq, baud=c["baud"], bt=c["bt"], h=c["h"], lpiq_bw=c["lpiq_bw"], lpfm_bw=c["lpfm_bw"])
    a = bind.ora_streams(x, K.BASE_SR, lp_iq=False, **kw)
    b = bind.ora_streams(x, K.BASE_SR, lp_iq=True, **kw)
    assert a["n"] == b["n"] == len(x) // 2 // c["D"] and b["consts"]["lpiq_taps"] == c["T1"] and b["consts"]["decM"] == c["D"]
    dec = a["iq"].astype(np.float64)
    return _frozen(dict(ifiq=b["iq"], fm=b["fm"], bufs=b["bufs"])), _frozen(K.model(c, dec[:, 0] + 1j * dec[:, 1]))


def _check_base(tag, kind, got, seed, fq, names=TAPS):
    """the chain behind the decimator: the GPU against the model of ITS decimated IQ, the oracle against the model of its own"""
    c = K.BASE[kind]
    ref, omod = _base_ref(kind, seed, fq)
    dec = got["dec"].astype(np.float64)
    gmod = K.model(c, dec[:, 0] + 1j * dec[:, 1])
    g = {k: got[k] for k in names}
    go, gm, om = K.figures(g, ref), K.figures(g, gmod), K.figures({k: ref[k] for k in names}, omod)
    print("IFSWEEP %-30s" % tag + "".join("  %s gpu-oracle %.2e/%.2e gpu-f64 %.2e/%.2e oracle-f64 %.2e/%.2e ratio %.2f/%.2f" %
                                          (k, *go[k], *gm[k], *om[k], gm[k][0] / max(om[k][0], 1e-30), gm[k][1] / max(om[k][1], 1e-30)) for k in go))
    for k in go:
        assert go[k][0] < ORACLE_BOUND[k][0] and go[k][1] < ORACLE_BOUND[k][1], (tag, k, "against the oracle", go[k])
        assert gm[k][0] <= 3 * om[k][0] + FLOOR[k][0], (tag, k, "RMS against the float64 model", gm[k], om[k])
        assert gm[k][1] <= 3 * om[k][1] + FLOOR[k][1], (tag, k, "max-abs against the float64 model", gm[k], om[k])


@pytest.mark.parametrize("kind", ["rs41", "dfm", "m10"])
def test_base_rate_engine(oracle, kind):
    """2.4 Msps -> 48 kHz, the presets of the three decoders, one call of 0.15 s"""
    from radiosonde_auto_rx_amd import engine as E
    c = K.BASE[kind]
    fq = E.snap_fq(FQ[kind][0], K.BASE_SR)
    x = K.signal_base(kind, 41, fq)
    eng = E.Engine([fq], K.BASE_SR, sonde=kind, keep_soft=True, max_chunk=len(x) // 2)
    try:
        assert (eng.info["decM"], eng.info["if_sr"], eng.info["lpiq_taps"], int(eng.info["sps"])) == (c["D"], c["sr"], c["T1"], c["nwin"])
        eng.process_host(x)
        got = _read(eng, 0, 0, len(x) // 2 // c["D"], ("dec",) + TAPS)
    finally:
        eng.close()
    _check_base("2400k %s" % kind, kind, got, 41, fq)


def test_mixed_engine_three_groups_in_one_launch(oracle):
    """k_if_chain_multi: RS41, DFM and M10 groups (2 + 2 + 1 channels: three tone windows and tap sets) in ONE launch.  A mixed engine keeps no soft
    streams, so the tone-correlator stream only: every channel's bufs against the model of its own decimated IQ"""
    from radiosonde_auto_rx_amd import engine as E
    kinds = ["rs41", "dfm", "rs41", "m10", "dfm"]
    pick = {"rs41": 0, "dfm": 0, "m10": 0}
    fqs, seeds = [], []
    for i, k in enumerate(kinds):
        fqs.append(E.snap_fq(FQ[k][pick[k]], K.BASE_SR))
        seeds.append(41 if pick[k] == 0 else 50 + i)             # (the first channel of a kind shares signal and references with test_base_rate_engine)
        pick[k] += 1
    X = np.stack([K.signal_base(k, s, f) for k, s, f in zip(kinds, seeds, fqs)])
    n_if = X.shape[1] // 2 // 50
    eng = E.MixedEngine(fqs, kinds, K.BASE_SR, max_chunk=X.shape[1] // 2)
    try:
        for ch, k in enumerate(kinds):
            assert int(eng.group_info(ch)[1]["sps"]) == K.BASE[k]["nwin"] and eng.group_info(ch)[1]["lpiq_taps"] == 49
        eng.process_host(X)
        got = [_read(eng, ch, 0, n_if, ("dec", "bufs")) for ch in range(len(kinds))]
    finally:
        eng.close()
    for ch, k in enumerate(kinds):
        _check_base("mixed ch %d %s" % (ch, k), k, got[ch], seeds[ch], fqs[ch], names=("bufs",))
