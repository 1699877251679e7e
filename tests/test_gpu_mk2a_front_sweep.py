"""MkIIa front-end sweep: every sample k_mk2a_mix and the produce() part of k_mk2a write — the IF samples of a call (ifbuf), zrot, zlp, fmr,
sraw (--IQ), bufs, fmbuf — read through the testing taps (sonde_mk2a_read_tap / _read_state) and compared with the reference's own
mk2a1680mod.c driven by oracle/ref_mk2a_harness.c (read from oracle/_ref/, nothing else of the reference) and with the float64 model of
tests/mk2a_front_cases.py, whose table says what each case selects.  tests/test_mk2a_front_cases.py keeps harness, model and table honest
without a GPU.  Captures: 0.45 s from seeds (at most 108 000 IF samples).

(a) against the -O2 harness, every sample: IF IQ (ifin, zlp) and FM (fm, fmbuf) 1e-6 RMS and 2e-5 max-abs, tone stream (sraw) and bufs 1e-5 RMS
    (DESIGN 2).  With --dc up to the first AFC step of either side (at least half a window); ifin, which no AFC reaches, over the whole capture.
(b) the schedule: windows at the same samples; locked, mv_pos, header found, frame bits and frame ends exact; mv within 2e-4; Df behind window k
    within 3 x |Df(-Ofast) - Df(-O2)| of the reference's two builds at that window + IF rate x 2^-24 / 1.6 Hz (one float32 ulp of the dc mean).
(c) against the float64 model run with the ENGINE's schedule (read through the state tap behind calls of one tile, 2048 IF samples), all
    samples, behind AFC steps too: GPU - model <= 3 x (harness - model under the harness's schedule) + FLOOR, RMS and max-abs separately.
(d) cuts: the streams, the final state record and the frames of calls cut at CUTS, one sample before / at / after the first window, the first
    IQ-dc block end and the first AFC step are the bits of the tile-by-tile run; one call of the whole capture leaves the same ring contents,
    state and frames; calls of ONE IF sample (the smallest max_chunk create accepts) likewise, over three turns of the history rings.
(e) three captures in one engine: the middle channel's streams and state are the bits of its single-channel run.

Measured on an MI355X: DESIGN.md 2a.2 holds the table these tests print (MK2ASWEEP lines)."""
import functools
import os

import numpy as np
import pytest

import mk2a_front_cases as K

pytestmark = pytest.mark.gpu

TILE = 2048                                                      # MK2A_TILE; the IF-rate history rings hold two of them
RING = 2 * TILE
TAP_OF = dict(ifin="if", zrot="zrot", zlp="zlp", fm="fmr", sraw="sraw", bufs="bufs", fmbuf="fmbuf")
REF_BOUND = dict(ifin=(1e-6, 2e-5), zlp=(1e-6, 2e-5), fm=(1e-6, 2e-5), fmbuf=(1e-6, 2e-5), sraw=(1e-5, None), bufs=(1e-5, None))
# Floors of the float64 comparison, (RMS, max-abs), on top of 3 x the reference's own deviation.  ifin, zlp, fm, bufs of --IQ: the FLOOR of
# tests/test_gpu_if_chain_sweep.py for the decimator / IF IQ, fm and bufs streams, derivation there (this kernel takes atan2, the phasors and the
# square roots in double like the reference, so those floors are generous here).  Derived beside them:
#   zrot:  the reference keeps no copy of the rotated sample, so its deviation is taken from ifin, the stream in front: zrot = z e^{-i phi} with
#          the phasor from a double sincos (1e-16) rounded ONCE to float32: half an ulp of a component below 0.5 (signal 0.45, noise 4 sigma 0.04)
#          = 2^-26 = 1.5e-8 max, 1.5e-8 / sqrt 3 = 0.9e-8 RMS, on top of ifin's floor 1e-8.
#   sraw:  bufs' floor (it is bufs in front of the IQFM low-pass, whose weights sum to 1 in absolute value within 1.5).
#   fmbuf, bufs of --iq: fm's floor, which already is the figure behind the FM low-pass.
FLOOR = dict(ifin=(1e-8, 1e-8), zrot=(1.9e-8, 2.5e-8), zlp=(1e-8, 1e-8), fm=(1e-7, 2.7e-7), fmbuf=(1e-7, 2.7e-7), sraw=(1e-7, 6.4e-7), bufs_iq=(1e-7, 6.4e-7),
             bufs=(1e-7, 2.7e-7))
CUTS = [1, 3, "decFM-1", "decFM", "decFM+1", 63, 64, 65, 2047, 2048, 2049]


@pytest.fixture(scope="module", autouse=True)
def _harness_present():
    from oracle import bind
    missing = [n for n in ("libref_mk2a.so", "libref_mk2a_O2.so") if not os.path.exists(os.path.join(bind.REFDIR, n))]
    if missing:
        pytest.fail("oracle/_ref/%s missing: build it where the reference lies (make -C oracle ref)" % ", ".join(missing))


# ----------------------------------------------------------------------------------------------- the engine
def _feed(cid, X, calls, *, collect=True, max_chunk=None, read_every=1):
    """an engine of the case fed X ([2n] or [channels, 2n] raw samples) in calls of the given lengths (base-rate samples) ->
    per channel dict(streams {name: array, NaN where not read}, states [(IF samples fed, state)], frames, final state)"""
    from radiosonde_auto_rx_amd.mk2a import Mk2aEngine
    c = K.BY_ID[cid]
    X = np.asarray(X)
    X = X[None, :] if X.ndim == 1 else X
    n_ch, n = X.shape[0], X.shape[1] // 2
    assert sum(calls) == n
    eng = Mk2aEngine([c.get("fq", 0.0)] * n_ch, K.sr_of(c), max_chunk=max_chunk or max(calls), **K.engine_kw(c))
    try:
        D, d = eng.dec_m, eng.info["dec_fm"]
        names = [s for s in TAP_OF if s != "sraw" or c["opt"]["opt_iq"] == 5]
        n_if, n_out = n // D, n // D // d
        out = [dict(streams={s: np.full(n_out if s in ("bufs", "fmbuf") else n_if, np.nan, np.float32 if s in ("fm", "sraw", "bufs", "fmbuf") else np.complex64)
                             for s in names}, states=[], frames=[]) for _ in range(n_ch)]
        pos = u_read = 0
        for i, b in enumerate(calls):
            assert b > 0 and b % D == 0
            eng.process_host(X[:, 2 * pos:2 * (pos + b)])
            pos += b
            u1 = pos // D
            for f in eng.fetch_frames():
                out[f["channel"]]["frames"].append(f)
            if not collect or ((i + 1) % read_every and i + 1 < len(calls)):
                continue
            for ch in range(n_ch):
                o = out[ch]
                u0 = max(u_read, u1 - RING)
                for s in names:
                    if s in ("bufs", "fmbuf"):
                        a, e = -(-u0 // d), u1 // d
                    elif s == "ifin":
                        a, e = max(u0, u1 - b // D), u1
                    else:
                        a, e = u0, u1
                    if e > a:
                        o["streams"][s][a:e] = eng.read_tap(ch, TAP_OF[s], a, e - a)
                o["states"].append((u1, eng.read_state(ch)))
            u_read = u1
        final = [eng.read_state(ch) for ch in range(n_ch)]
        eng.finish()
        for f in eng.fetch_frames():
            out[f["channel"]]["frames"].append(f)
        for ch in range(n_ch):
            out[ch]["final"] = final[ch]
            out[ch]["info"] = dict(eng.info)
        return out
    finally:
        eng.close()


def _tiles(n, step):
    return [step] * (n // step) + ([n % step] if n % step else [])


@functools.lru_cache(maxsize=None)
def _tile_run(cid, seed=None):
    """the case in calls of one tile: every stream sample, the state behind every call"""
    c = K.BY_ID[cid]
    x = K.capture(cid, seed)
    D = K.reference(cid, seed=seed)["consts"]["decM"]
    r = _feed(cid, x, _tiles(len(x) // 2, TILE * D))[0]
    for v in r["streams"].values():
        v.setflags(write=False)
    return r


def _nominal(c, st):
    return int(st["locked"]) if c["opt"]["dc"] else 1


def _engine_windows(c, states, K4, frames):
    """the windows of a run from the state behind each call.  While searching (mode 0) the next window is evaluated when the output sample
    count reaches n_start + K - 4; a call of one tile makes fewer output samples than that, so at most one window falls in a call, and the
    state behind the call still holds what it set (mv, mv_pos, dc, dDf, Df, locked) even where its frame lies so far back in the window that it
    also ended in this call.  A header was accepted where a frame carries the window's mv_pos."""
    wins, prev = [], dict(n_start=0, mode=0)
    heads = {int(f["mv_pos"]) for f in frames}
    for u, st in states:
        nw = prev["n_start"] + K4
        if prev["mode"] == 0 and st["out_samples"] >= nw:
            wins.append(dict(sample=int(nw), mv=st["mv"], mv_pos=int(st["mv_pos"]), Df=st["df"], nominal=_nominal(c, st), found=int(int(st["mv_pos"]) in heads),
                             dc=st["dc"], dDf=st["ddf"]))
        prev = st
    return wins


def _engine_schedule(c, wins, d):
    s = [(0, 0.0, 0 if c["opt"]["dc"] else 1)]
    for w in wins:
        if (w["Df"], w["nominal"]) != s[-1][1:]:
            s.append((w["sample"] * d, w["Df"], w["nominal"]))
    return s


def _floor(c, s):
    return FLOOR["bufs_iq" if s == "bufs" and c["opt"]["opt_iq"] == 5 else s]


def _same_bits(tag, a, b, sl=slice(None)):
    for s in a:
        x, y = a[s][sl], b[s][sl]
        both = ~(np.isnan(x) | np.isnan(y))
        assert both.any() or len(x) == 0, (tag, s, "nothing to compare")
        bad = np.flatnonzero((x.view(np.uint32 if x.dtype == np.float32 else np.uint64) != y.view(np.uint32 if y.dtype == np.float32 else np.uint64)) & both)
        assert bad.size == 0, (tag, s, "first differing samples", bad[:8], "of", bad.size)


# ----------------------------------------------------------------------------------------------- (a) (b) (c): every case, tile by tile
@pytest.mark.parametrize("cid", [c["id"] for c in K.CASES])
def test_case(cid):
    c = K.BY_ID[cid]
    ref, reff = K.reference(cid), K.reference(cid, "libref_mk2a.so")
    k = ref["consts"]
    d, sr = k["decFM"], k["if_sr"]
    run = _tile_run(cid)
    info = run["info"]
    assert (info["if_rate"], info["dec_m"], info["dec_fm"], info["L"], info["K"], info["taps_dec"] if k["decM"] > 1 else 0, info["taps_iq"] if k["lp"] & 1 else 0) == \
           (sr, k["decM"], d, k["L"], k["K"], k["dectaps"] if k["decM"] > 1 else 0, k["iq_taps"])
    g = run["streams"]
    assert all(not np.isnan(v).any() for v in g.values()) and len(g["zlp"]) == ref["n_if"] and len(g["bufs"]) == ref["n_out"]
    # the harness holds every sample of every stream the case has (the tone stream inside frames too): nothing is left out of a figure below
    assert all(len(ref[s]) == len(g[s]) and not np.isnan(ref[s]).any() for s in g if s != "zrot")
    wins = _engine_windows(c, run["states"], k["K"] - 4, run["frames"])
    gs, rs = _engine_schedule(c, wins, d), K.schedule_of(ref)

    # (a) against the reference harness
    span = min([s[0] for s in gs[1:2]] + [s[0] for s in rs[1:2]] + [ref["n_if"]]) if c["opt"]["dc"] else ref["n_if"]
    assert span >= (k["K"] - 4) * d // 2
    line = "MK2ASWEEP %-10s" % cid
    fig_ref = {}
    for s in g:
        if s == "zrot":
            continue
        sl = slice(None) if s == "ifin" else slice(0, span // d if s in ("bufs", "fmbuf") else span)
        fig_ref[s] = K.figure(g[s], ref[s], sl)
        ne = int(np.count_nonzero(g[s][sl] != ref[s][sl]))
        line += "  %s gpu-ref %.2e/%.2e ne %d of %d" % (s, *fig_ref[s], ne, len(ref[s][sl]))
    print(line)
    for s, f in fig_ref.items():
        assert f[0] < REF_BOUND[s][0] and (REF_BOUND[s][1] is None or f[1] < REF_BOUND[s][1]), (cid, s, "against the reference", f)

    # (b) the schedule
    print("MK2ASWEEP %-10s windows gpu %s" % (cid, [(w["sample"], round(w["mv"], 4), w["mv_pos"], w["Df"], w["nominal"], w["found"]) for w in wins]))
    print("MK2ASWEEP %-10s windows ref %s" % (cid, [(int(w["sample"]), round(w["mv"], 4), int(w["mv_pos"]), w["Df"], int(w["nominal"]), int(w["found"])) for w in ref["win"]]))
    assert [w["sample"] for w in wins] == [int(w["sample"]) for w in ref["win"]]
    ulp = sr * 2.0 ** -24 / 1.6
    inv = 0
    for w, r2, rf in zip(wins, ref["win"], reff["win"]):
        tol = 3 * abs(rf["Df"] - r2["Df"]) + ulp
        assert abs(w["Df"] - r2["Df"]) <= tol, ("Df behind the window at", w["sample"], w["Df"], r2["Df"], rf["Df"], tol)
        assert abs(w["mv"] - r2["mv"]) <= 2e-4 and w["mv_pos"] == int(r2["mv_pos"]), (w, r2)
        if c["opt"]["dc"]:
            assert w["nominal"] == int(r2["nominal"]), (w, r2)
        found = int(r2["found"])
        if found and r2["mv"] * (0.5 - inv) < 0:                # main drops a header of the wrong polarity and flips the option (:2383-2386)
            found, inv = 0, inv ^ 1
        assert w["found"] == found, (w, r2)
    assert len(run["frames"]) == len(ref["frames"])
    for f, r2, rf in zip(run["frames"], ref["frames"], reff["frames"]):
        assert np.array_equal(f["bits"], r2["bits"]) and f["mv_pos"] == int(r2["mv_pos"]) and f["sample"] == int(r2["sample"]) and f["inv"] == int(r2["inv"])
        assert abs(f["mv"] - r2["mv"]) <= 2e-4 and abs(f["df"] - r2["Df"]) <= 3 * abs(rf["Df"] - r2["Df"]) + ulp, (f["mv"], f["df"], r2["mv"], r2["Df"])
    st = run["final"]
    assert (st["if_samples"], st["out_samples"], st["base"]) == (ref["n_if"], ref["n_out"], ref["n_if"] * k["decM"])
    assert (st["avg_x"], st["avg_y"], st["maxcnt"]) == (np.float32(ref["dcev"][-1][1]), np.float32(ref["dcev"][-1][2]), int(ref["dcev"][-1][3]))

    # (c) against the float64 model, all samples
    if not c.get("model", True):
        return
    z = K.front_of(cid)
    mg = dict(K.model(z, ref, gs, ref["n_if"]), ifin=z)
    mr = dict(K.model(z, ref, rs, ref["n_if"]), ifin=z)
    line = "MK2ASWEEP %-10s" % cid
    figs = {}
    for s in g:
        gm = K.figure(g[s], mg[s])
        om = K.figure(ref["ifin" if s == "zrot" else s], mr["ifin" if s == "zrot" else s])
        figs[s] = (gm, om)
        line += "  %s gpu-f64 %.2e/%.2e ref-f64 %.2e/%.2e ratio %.2f/%.2f" % (s, *gm, *om, gm[0] / max(om[0], 1e-30), gm[1] / max(om[1], 1e-30))
    print(line)
    for s, (gm, om) in figs.items():
        fl = _floor(c, s)
        assert gm[0] <= 3 * om[0] + fl[0], (cid, s, "RMS against the float64 model", gm, om)
        assert gm[1] <= 3 * om[1] + fl[1], (cid, s, "max-abs against the float64 model", gm, om)


# ----------------------------------------------------------------------------------------------- (d) cuts
def _cut_calls(cid):
    """call lengths in base-rate samples: CUTS, then one IF sample before / at / after the first window, the first IQ-dc block end and the
    first AFC step, then the rest; stretches longer than a tile go tile by tile so that every sample can still be read from the rings"""
    ref = K.reference(cid)
    k = ref["consts"]
    D, d = k["decM"], k["decFM"]
    lens = [{"decFM-1": d - 1, "decFM": d, "decFM+1": d + 1}.get(v, v) for v in CUTS]
    pos, marks = 0, []
    for v in lens:
        if v > 0:
            pos += v
            marks.append(pos)
    targets = [(k["K"] - 4) * d, k["maxcnt0"] // D] + [s[0] for s in K.schedule_of(ref)[1:2]]
    for t in sorted(set(targets)):
        marks += [t - 1, t, t + 1]
    marks = sorted({m for m in marks if 0 < m < ref["n_if"]}) + [ref["n_if"]]
    calls, pos = [], 0
    for m in marks:
        while m - pos > RING:
            calls.append(TILE * D)
            pos += TILE
        calls.append((m - pos) * D)
        pos = m
    return calls, marks


def _same_state(tag, a, b):
    diff = {f: (a[f], b[f]) for f in a if np.asarray(a[f]).tobytes() != np.asarray(b[f]).tobytes()}
    assert not diff, (tag, diff)


def _same_frames(tag, a, b):
    assert len(a) == len(b), (tag, len(a), len(b))
    for f, h in zip(a, b):
        assert np.array_equal(f["bits"], h["bits"]) and (f["mv"], f["df"], f["mv_pos"], f["sample"], f["inv"]) == (h["mv"], h["df"], h["mv_pos"], h["sample"], h["inv"]), tag


@pytest.mark.parametrize("cid", [c["id"] for c in K.CASES])
def test_call_cuts_give_the_same_bits(cid):
    ref = K.reference(cid)
    one = _tile_run(cid)
    x = K.capture(cid)
    calls, marks = _cut_calls(cid)
    assert min(calls) == ref["consts"]["decM"] and len(calls) > 40
    cut = _feed(cid, x, calls)[0]
    _same_bits("%s cut" % cid, cut["streams"], one["streams"])
    _same_state("%s cut" % cid, cut["final"], one["final"])
    _same_frames("%s cut" % cid, cut["frames"], one["frames"])
    whole = _feed(cid, x, [len(x) // 2])[0]                      # one call: what the rings still hold at its end
    n_if = ref["n_if"]
    tail = {s: slice(len(v) - (RING // ref["consts"]["decFM"] if s in ("bufs", "fmbuf") else RING), len(v)) for s, v in one["streams"].items()}
    for s in one["streams"]:
        _same_bits("%s one call" % cid, {s: whole["streams"][s]}, {s: one["streams"][s]}, tail[s])
    _same_state("%s one call" % cid, whole["final"], one["final"])
    _same_frames("%s one call" % cid, whole["frames"], one["frames"])
    print("MK2ASWEEP %-10s %d calls cut at IF samples %s ...: the bits of %d tile calls and of one call of %d" % (cid, len(calls), marks[:14], len(one["states"]), n_if))


@pytest.mark.parametrize("cid", ["auto240", "r960"])
def test_calls_of_one_if_sample(cid):
    """max_chunk = decM, the smallest create accepts: 12 288 calls of one IF sample, three turns of the IF-rate rings (and 48 / 15 of the
    base-rate ring's 256 decM + taps window), taps read every 2048 calls"""
    D = K.reference(cid)["consts"]["decM"]
    n = 3 * RING
    one = _tile_run(cid)
    got = _feed(cid, K.capture(cid)[:2 * n * D], [D] * n, max_chunk=D, read_every=TILE)[0]
    d = K.reference(cid)["consts"]["decFM"]
    g = {s: v for s, v in got["streams"].items() if s != "ifin"}                 # (the call's own IF buffer holds one sample here)
    _same_bits("%s 1-sample calls" % cid, g, {s: one["streams"][s][:n // d if s in ("bufs", "fmbuf") else n] for s in g})
    u, st = [(u, s) for u, s in one["states"] if u == n][0]
    _same_state("%s 1-sample calls" % cid, got["final"], st)


# ----------------------------------------------------------------------------------------------- (e) three channels
def test_three_captures_in_one_engine():
    cid = "auto240"
    seeds = (11, None, 12)                                       # the middle channel is the case's own capture
    X = np.stack([K.capture(cid, s) for s in seeds])
    got = _feed(cid, X, _tiles(X.shape[1] // 2, TILE))
    one = _tile_run(cid)
    _same_bits("middle channel", got[1]["streams"], one["streams"])
    _same_state("middle channel", got[1]["final"], one["final"])
    _same_frames("middle channel", got[1]["frames"], one["frames"])
    for ch, s in ((0, 11), (2, 12)):                             # and the neighbours are their own captures, not copies
        ref = K.reference(cid, seed=s)
        assert [f["mv_pos"] for f in got[ch]["frames"]] == [int(f["mv_pos"]) for f in ref["frames"]] and len(ref["frames"]) >= 1
        f = K.figure(got[ch]["streams"]["ifin"], ref["ifin"])
        assert f[0] < 1e-6 and f[1] < 2e-5, (ch, f)
    assert not np.array_equal(got[0]["streams"]["ifin"], got[1]["streams"]["ifin"])
