"""The IF chain sweep's model and table (tests/if_chain_cases.py) held to the literal sums, to the CPU oracle and to the library's layout rule — no GPU.

  model = literal sums ....... on about 300 probe outputs per case (first and last 16, +-8 around every multiple of 960 and of 1024) the vectorised model's
                               z, fm and bufs equal the term-by-term sums to 1e-12
  model = the reference ...... oracle.ora_streams minus the model below 1e-6 RMS on IF IQ, fm and bufs over EVERY sample of every case: the condition
                               the decimator sweep puts on its float64 sum.  The figures are printed (ORACLE-MODEL ...): they are the "reference alone"
                               column of tests/test_gpu_if_chain_sweep.py.  Measured at seed 7: IF IQ <= 8.4e-8 RMS / 5.6e-7 max (384 kHz), fm <= 2.3e-8 / 1.4e-7,
                               bufs <= 7.6e-7 / 1.9e-6 (the reference's recursive float sums drifting)
  table = the library ........ layout and LDS bytes of every row equal sonde_if_chain_lds_bytes() of the built library (a pure host function: the rule
                               the launches use) and the restatement in if_chain_cases.py; T1 / T2 / nwin equal the oracle's consts / (int)sps
  the comparison can fail .... the last IF tap zeroed, and one window term dropped at multiples of 960, move the model by more than 10 x the
                               oracle-minus-model figure of their case
Case zeros8 has no model (atan2 of signed zeros is the reference's float32 arithmetic, not a sum): table row only."""
import ctypes as C
import functools

import numpy as np
import pytest
import if_chain_cases as K

MODELLED = [c["id"] for c in K.CASES if c["id"] != "zeros8"]


@functools.lru_cache(maxsize=None)
def _oracle_and_model(cid):
    from oracle import bind
    c = K.BY_ID[cid]
    x = K.signal(cid, 7)
    ref = bind.ora_streams(x, c["sr"], **K.oracle_kw(c))
    assert ref["n"] == len(x) // 2
    mod = K.model(c, K.samples_of(x, c["bits"]))
    return dict(ifiq=ref["iq"], fm=ref["fm"], bufs=ref["bufs"], consts=ref["consts"]), mod


@pytest.mark.parametrize("cid", MODELLED)
def test_model_is_the_literal_sums(oracle, cid):
    c = K.BY_ID[cid]
    y = K.samples_of(K.signal(cid, 7), c["bits"])
    _, mod = _oracle_and_model(cid)
    ms = K.probes(len(y))
    assert 200 <= len(ms) <= 1100 and ms[0] == 0 and ms[-1] == len(y) - 1
    lit = K.literal(c, y, ms)
    fig = K.figures({k: mod[k][ms] for k in lit}, lit)
    print("LITERAL %-14s outputs %d  " % (cid, len(ms)) + "  ".join("%s max %.2e" % (k, fig[k][1]) for k in fig))
    for k in fig:
        assert fig[k][1] < 1e-12, (cid, k, fig[k])


@pytest.mark.parametrize("cid", MODELLED)
def test_model_is_the_chain_the_reference_computes(oracle, cid):
    ref, mod = _oracle_and_model(cid)
    fig = K.figures(ref, mod)
    print("ORACLE-MODEL %-14s " % cid + "  ".join("%s rms %.2e max %.2e" % (k, *fig[k]) for k in fig))
    for k in fig:
        assert fig[k][0] < 1e-6, (cid, k, fig[k])


def _lds_bytes():
    from radiosonde_auto_rx_amd import engine
    L = C.CDLL(engine.LIB_PATH)
    f = L.sonde_if_chain_lds_bytes
    f.restype = C.c_size_t
    f.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)]
    return f


@pytest.mark.parametrize("cid", [c["id"] for c in K.CASES])
def test_row_selects_what_it_claims(oracle, cid):
    c = K.BY_ID[cid]
    tone_on = int(c["iq"] != 0)
    ov = C.c_int(-1)
    lds = _lds_bytes()(c["T1"], c["T2"], c["nwin"], tone_on, 1, C.byref(ov))           # fm_on: the sweep's engines keep the FM stream (keep_soft)
    assert (lds, "AB"[ov.value]) == (c["lds"], c["layout"]) == K.lds_rule(c["T1"], c["T2"], c["nwin"], tone_on, 1)
    k = oracle.ora_streams(K.signal(cid, 7)[:64], c["sr"], **K.oracle_kw(c))["consts"]
    assert (k["lpiq_taps"] or 1, k["lpfm_taps"] or 1, k["if_sr"], k["decM"]) == (c["T1"], c["T2"], c["sr"], 1)
    w_iq, w_fm, sps, _ = K.design(c)
    assert (1 if w_iq is None else len(w_iq), 1 if w_fm is None else len(w_fm), int(sps)) == (c["T1"], c["T2"], c["nwin"])
    assert k["L"] == int(len(K.HEADER) * np.float32(sps) + 0.5) <= 2730 and k["M"] == 8192


def test_table_covers_the_edges():
    by = K.BY_ID
    nzx = lambda c: (c["T2"] - 1) + max(1, c["nwin"] - 1) + 3 + K.IF_TILE - ((c["T2"] - 1) & ~3)          # nz - xlo
    assert nzx(by["edge_B"]) == 1024 and nzx(by["edge_A"]) == 1025 and nzx(by["edge_B3"]) == 1024 and nzx(by["edge_A3"]) == 1025
    assert by["edge_B3"]["T2"] % 4 == 3 and by["edge_A3"]["T2"] % 4 == 3
    assert {c["T1"] % 4 for c in K.CASES if c["T1"] > 1} == {1, 3} and by["nolp"]["T1"] == 1
    assert {c["layout"] for c in K.CASES} == {"A", "B"} and any(c["lp_fm"] and c["iq"] and c["layout"] == "B" for c in K.CASES)
    assert by["big"]["lds"] > 64 * 1024 and K.lds_rule(1501, 3001, 312, 1, 1)[0] == K.REFUSED["lds"] > 160 * 1024
    assert max(int(round(c["sr"] * c["seconds"])) for c in K.CASES) == 28_800
    assert by["wide192"]["T1"] - 1 + by["wide192"]["T2"] - 1 + by["wide192"]["nwin"] + 2 > K.IF_TILE // 2


@pytest.mark.parametrize("cid", ["rs41", "rs41_50k_lpfm", "edge_B"])
def test_a_zeroed_last_if_tap_shows(oracle, cid):
    """(the 7400 Hz filter at 48 / 50 kHz ends in a tap of -7.4e-5; at 96 kHz and above, and with the 12 and 24 kHz filters whose sinc has a zero there, the
    last tap is 1e-20: a kernel that drops it cannot be told from one that does not, so these cases carry the check)"""
    c = K.BY_ID[cid]
    ref, mod = _oracle_and_model(cid)
    floor = K.figures(ref, mod)["ifiq"]
    mut = K.figures(K.model(c, K.samples_of(K.signal(cid, 7), c["bits"]), zero_last_tap=True), mod)["ifiq"]
    print("MUTANT last tap %-6s  ifiq rms %.2e max %.2e   oracle-model rms %.2e max %.2e" % (cid, *mut, *floor))
    assert mut[0] > 10 * floor[0] and mut[1] > 10 * floor[1]


@pytest.mark.parametrize("cid", [c["id"] for c in K.CASES if c["iq"] != 0])
def test_a_dropped_window_term_shows(oracle, cid):
    c = K.BY_ID[cid]
    ref, mod = _oracle_and_model(cid)
    floor = K.figures(ref, mod)["bufs"]
    mut = K.model(c, K.samples_of(K.signal(cid, 7), c["bits"]), drop_term_every=960)
    d = np.abs(mut["bufs"] - mod["bufs"])
    at = np.arange(960, len(d), 960)
    assert len(at) >= 7 and np.count_nonzero(d) == len(at)
    print("MUTANT window term %-14s at %d outputs: min %.2e rms %.2e max %.2e   oracle-model rms %.2e max %.2e" % (cid, len(at), d[at].min(), K.rms(d[at]), d[at].max(), *floor))
    assert K.rms(d[at]) > 10 * floor[0] and d[at].max() > 10 * floor[1]


@pytest.mark.parametrize("kind", list(K.BASE))
def test_base_rate_rows(oracle, kind):
    """the presets behind the 2.4 Msps decimator: the same claims, and the model run on the oracle's decimated IQ is the oracle's chain"""
    c = K.BASE[kind]
    ov = C.c_int(-1)
    lds = _lds_bytes()(c["T1"], c["T2"], c["nwin"], 1, 1, C.byref(ov))
    assert (lds, "AB"[ov.value]) == (c["lds"], c["layout"]) == K.lds_rule(c["T1"], c["T2"], c["nwin"], 1, 1)
    x = K.signal_base(kind, 41, 0.1)
    kw = dict(fq=0.1, baud=c["baud"], bt=c["bt"], h=c["h"], lpiq_bw=c["lpiq_bw"], lpfm_bw=c["lpfm_bw"])
    a, b = oracle.ora_streams(x, K.BASE_SR, lp_iq=False, **kw), oracle.ora_streams(x, K.BASE_SR, lp_iq=True, **kw)
    assert (b["consts"]["lpiq_taps"], b["consts"]["lpfm_taps"] or 1, b["consts"]["if_sr"], b["consts"]["decM"], int(K.design(c)[2])) == (c["T1"], c["T2"], c["sr"], c["D"], c["nwin"])
    dec = a["iq"].astype(np.float64)
    fig = K.figures(dict(ifiq=b["iq"], fm=b["fm"], bufs=b["bufs"]), K.model(c, dec[:, 0] + 1j * dec[:, 1]))
    print("ORACLE-MODEL %-14s " % c["id"] + "  ".join("%s rms %.2e max %.2e" % (k, *fig[k]) for k in fig))
    for k in fig:
        assert fig[k][0] < 1e-6, (kind, k, fig[k])


def test_the_tone_phase_origin_does_not_enter_bufs(oracle):
    """|F1| and |F2| are the same wherever the tone phase counts from: a kernel that took the phase from the engine's sample count instead of the channel's own
    (restarted channels) computes the same stream up to the last bit, so no tolerance can tell the two apart — what can is bit-equality with a fresh engine
    (tests/test_gpu_if_chain_sweep.py::test_restart_on_a_run_boundary_is_a_fresh_engine_to_the_bit)"""
    c = K.BY_ID["rs41"]
    y = K.samples_of(K.signal("rs41", 7), c["bits"])
    d = np.abs(K.model(c, y)["bufs"] - K.model(c, y, m_start=-2501)["bufs"]).max()
    print("PHASE ORIGIN rs41  bufs max %.2e" % d)
    assert d < 1e-12
