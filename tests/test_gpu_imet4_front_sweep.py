"""iMet-4 front-end sweep: every sample k_imet4_decim and the front end of k_imet4_afsk write — the IF samples of a call (ifbuf, "ifin"), zring
("zrot": the sample entering the IF low-pass), fmring ("fm": the sample entering the FM low-pass), xring ("x": the front-end sample the
sliding DFT takes) — and the state record (Df, dc, locked, pre_pos, xsum, the DFT sums, the IQ-dc fields), read through the testing taps
(sonde_imet4_read_tap / _read_state) and compared with the reference's own imet4iq.c run by oracle/ref_imet4_harness.c (read from
oracle/_ref/, nothing else of the reference) and with the float64 model of tests/imet4_front_cases.py, whose table says what each case
selects.  tests/test_imet4_front_cases.py keeps harness, model and table honest without a GPU.  Captures: 1.15 s from seeds.

(a) against the -O2 harness, every sample: IF IQ (ifin, zrot) and FM (fm, x) 1e-6 RMS and 2e-5 max-abs.  With --dc up to the first
    AFC update behind the header (more than half the capture; the update at sample 0 has to give the reference's Df to the bit); ifin, which
    no AFC reaches, over the whole capture.
(b) the schedule: the state changes Df / dc / locked at the reference's update samples and nowhere else (each update sample is a call of its
    own); Df behind update k within 3 x |Df(-Ofast) - Df(-O2)| of the reference's two builds + IF rate x 2^-24 / 1.6 Hz (one float32 ulp
    of the dc mean); tap set, pre_pos behind every call, frame bits, frame ends and the IQ-dc means exact.
(c) against the float64 model run with the ENGINE's schedule (state tap behind calls of at most one tile, 64 samples), all samples, behind
    AFC updates too: GPU - model <= 3 x (harness - model under the harness's schedule) + FLOOR, RMS and max-abs separately; likewise xsum
    and the two DFT sums behind every call against the windowed sums.
(d) cuts: the streams, the final state record and the frames of calls cut at CUTS, one sample before / at / after the header's sample, the
    first IQ-dc block end and the AFC update behind the header are the bits of the tile-by-tile run; one call of the whole capture leaves the
    same state, frames and ring contents; calls of ONE IF sample (the smallest max_chunk create accepts) likewise, past the header.
(e) three captures in one engine: the middle channel's streams and state are the bits of its single-channel run.

Measured on an MI355X: DESIGN.md 2a.2 holds the table these tests print (IMET4SWEEP lines)."""
import functools
import os

import numpy as np
import pytest

import imet4_front_cases as I

pytestmark = pytest.mark.gpu

TILE = 64
TAP_OF = dict(ifin="if", zrot="zring", fm="fmring", x="xring")
REF_BOUND = dict(ifin=(1e-6, 2e-5), zrot=(1e-6, 2e-5), fm=(1e-6, 2e-5), x=(1e-6, 2e-5))
# Floors of the float64 comparison, (RMS, max-abs), on top of 3 x the reference's own deviation.  ifin, zrot, fm / x: those of the same streams in
# tests/test_gpu_mk2a_front_sweep.py (from tests/test_gpu_if_chain_sweep.py, derivation there; this kernel too takes the rotation's sincos and
# atan2 in double and rounds once).  Derived beside them:
#   xsum:  a float32 running sum below 128 in magnitude: one ulp, 2^-17.
#   F:     a double running sum of terms below 1 over floor(bitlen) <= 80 samples, magnitude below 64: a few ulps of 2^-47; 1e-12.
FLOOR = dict(ifin=(1e-8, 1e-8), zrot=(1.9e-8, 2.5e-8), fm=(1e-7, 2.7e-7), x=(1e-7, 2.7e-7), xsum=(2.0 ** -17, 2.0 ** -17), F=(1e-12, 1e-12))
CUTS = [1, 3, 1, 2, 63, 64, 65, 2047, 2048, 2049]               # (decFM is 1 in this engine: decFM - 1 drops out, decFM and decFM + 1 are 1 and 2)
STATE_F = ("df", "dc", "locked")


@pytest.fixture(scope="module", autouse=True)
def _harness_present():
    from oracle import bind
    missing = [n for n in ("libref_imet4.so", "libref_imet4_O2.so") if not os.path.exists(os.path.join(bind.REFDIR, n))]
    if missing:
        pytest.fail("oracle/_ref/%s missing: build it where the reference lies (make -C oracle ref)" % ", ".join(missing))


# ----------------------------------------------------------------------------------------------- the engine
def _names(cid):
    r = I.reference(cid)
    k = r["consts"]
    return [s for s, on in (("ifin", k["decM"] > 1), ("zrot", bool(k["iq_taps"])), ("fm", bool(k["fm_taps"])), ("x", True)) if on]


def _feed(cid, X, calls, *, max_chunk=None, collect=True):
    """an engine of the case fed X ([samples] or [channels, samples] raw) in calls of the given lengths (IF samples) ->
    per channel dict(streams {name: array, NaN where not read}, states [(IF samples fed, state)], frames, final state)"""
    from radiosonde_auto_rx_amd.imet4 import Imet4Engine
    c = I.BY_ID[cid]
    iq = not c.get("wav")
    w = 2 if iq else 1
    X = np.asarray(X)
    X = X[None, :] if X.ndim == 1 else X
    n_ch = X.shape[0]
    D = I.reference(cid)["consts"]["decM"]
    assert sum(calls) * D * w <= X.shape[1]
    eng = Imet4Engine([c.get("fq", 0.0)] * n_ch, I.sr_of(c), max_chunk=max_chunk or max(calls) * D, **I.engine_kw(c))
    try:
        assert eng.dec_m == D
        keep = eng.tap_ring - 64
        names = _names(cid)
        n = sum(calls)
        out = [dict(streams={s: np.full(n, np.nan, np.float32 if s in ("fm", "x") else np.complex64) for s in names}, states=[], frames=[]) for _ in range(n_ch)]
        u0 = 0
        for b in calls:
            assert b > 0
            eng.process_host(X[:, u0 * D * w:(u0 + b) * D * w])
            u1 = u0 + b
            for f in eng.fetch_frames():
                out[f["channel"]]["frames"].append(f)
            for ch in range(n_ch):
                o = out[ch]
                if collect:
                    a = max(u0, u1 - keep)
                    for s in names:
                        o["streams"][s][a:u1] = eng.read_tap(ch, TAP_OF[s], a, u1 - a)
                o["states"].append((u1, eng.read_state(ch)))
            u0 = u1
        for ch in range(n_ch):
            out[ch]["final"] = out[ch]["states"][-1][1]
            out[ch]["ring"] = eng.tap_ring
        return out
    finally:
        eng.close()


def _tile_calls(cid, n=None, seed=None):
    """calls of at most one tile, cut further so that every AFC update sample of the reference is a call of its own"""
    ref = I.reference(cid, seed=seed)
    n = ref["n"] if n is None else n
    marks = set(range(TILE, n, TILE)) | {n}
    for p in I.updates_of(ref):
        marks |= {m for m in (p, p + 1) if 0 < m < n}
    marks = sorted(marks)
    return [b - a for a, b in zip([0] + marks[:-1], marks)]


@functools.lru_cache(maxsize=None)
def _tile_run(cid):
    r = _feed(cid, I.capture(cid), _tile_calls(cid))[0]
    for v in r["streams"].values():
        v.setflags(write=False)
    return r


def _nominal(ref, st):
    return bool(st["locked"]) if (ref["dc"] and ref["consts"]["iq_taps"]) else True


def _engine_schedule(ref, states):
    """per sample what was in effect for it, from the state behind each call (changes happen at the last sample of a call, (b) holds that)"""
    n = ref["n"]
    df, dc, nom = np.zeros(n), np.zeros(n), np.zeros(n, bool)
    nom[:] = _nominal(ref, dict(locked=0))
    for u, st in states:
        df[u:], dc[u:], nom[u:] = st["df"], st["dc"], _nominal(ref, st)
    return dict(df=df, dc=dc, nominal=nom)


def _same_bits(tag, a, b, sl=slice(None)):
    for s in a:
        x, y = a[s][sl], b[s][sl]
        both = ~(np.isnan(x) | np.isnan(y))
        assert both.any() or len(x) == 0, (tag, s, "nothing to compare")
        t = np.uint32 if x.dtype == np.float32 else np.uint64
        bad = np.flatnonzero((x.view(t) != y.view(t)) & both)
        assert bad.size == 0, (tag, s, "first differing samples", bad[:8], "of", bad.size)


def _same_state(tag, a, b):
    diff = {f: (a[f], b[f]) for f in a if np.asarray(a[f]).tobytes() != np.asarray(b[f]).tobytes()}
    assert not diff, (tag, diff)


def _same_frames(tag, a, b):
    assert len(a) == len(b), (tag, len(a), len(b))
    for f, h in zip(a, b):
        assert np.array_equal(f["bits"], h["bits"]) and f["sample"] == h["sample"], tag


# ----------------------------------------------------------------------------------------------- (a) (b) (c): every case, tile by tile
@pytest.mark.parametrize("cid", [c["id"] for c in I.CASES])
def test_case(cid):
    ref, reff = I.reference(cid), I.reference(cid, "libref_imet4.so")
    k = ref["consts"]
    n, sr = ref["n"], k["if_sr"]
    run = _tile_run(cid)
    g = run["streams"]
    # every sample of every stream the case has, on both sides
    assert all(len(v) == n and not np.isnan(v).any() for v in g.values()) and all(ref[s] is not None and len(ref[s]) == n for s in g)
    upd, hdr = I.updates_of(ref), I.headers_of(ref)
    states = run["states"]

    # (b) the schedule
    prev, changed = dict(df=0.0, dc=0.0, locked=0), []
    for u, st in states:
        if any(st[f] != prev[f] for f in STATE_F):
            changed.append(u - 1)
        prev = st
        assert st["sample"] == u and (u == n or st["pre_pos"] == int(ref["pre_pos"][u])), ("pre_pos behind the call ending at", u, st["pre_pos"])
    print("IMET4SWEEP %-10s updates ref %s gpu changes at %s header %s pre_pos %d" % (cid, upd, changed, hdr, states[-1][1]["pre_pos"]))
    assert set(changed) <= set(upd) and set(I.changes_of(ref)) <= set(changed) | {n - 1}
    by_u = dict(states)
    ulp = sr * 2.0 ** -24 / 1.6
    for j, p in enumerate(upd):
        if p + 1 >= n:
            continue
        st = by_u[p + 1]
        tol = 3 * abs(reff["df"][p + 1] - ref["df"][p + 1]) + ulp
        print("IMET4SWEEP %-10s update at %d: Df gpu %.9f ref %.9f (-Ofast %.9f) tol %.2e  dc gpu %.9g ref %.9g" % (cid, p, st["df"], ref["df"][p + 1], reff["df"][p + 1], tol, st["dc"], ref["dc_of"][p + 1]))
        assert abs(st["df"] - ref["df"][p + 1]) <= tol
        assert _nominal(ref, st) == bool(ref["nominal"][p + 1])
        if j == 0 and p == 0:
            assert st["df"] == ref["df"][1] and st["dc"] == ref["dc_of"][1]         # one sample went into it: nothing to disagree about
    st = run["final"]
    assert st["pre_pos"] == int(ref["pre_pos"][-1]) + 0 and st["locked"] == k["locked_end"]
    assert len(run["frames"]) == len(ref["frames"]) >= 1
    for f, r2 in zip(run["frames"], ref["frames"]):
        assert np.array_equal(f["bits"], r2["bits"]) and f["sample"] + 1 == r2["sample"]
    if ref["iq"]:
        assert (st["avg_x"], st["avg_y"], st["maxcnt"]) == (np.float32(ref["dcev"][-1][1]), np.float32(ref["dcev"][-1][2]), int(ref["dcev"][-1][3]))

    # (a) against the reference harness
    span = n
    if ref["dc"]:
        behind = [p for p in upd if p > hdr[0]]
        span = behind[0] + 1
        assert span > n // 2
    line = "IMET4SWEEP %-10s" % cid
    fig_ref = {}
    for s in g:
        sl = slice(None) if s == "ifin" else slice(0, span)
        fig_ref[s] = I.figure(g[s], ref[s], sl)
        line += "  %s gpu-ref %.2e/%.2e ne %d of %d" % (s, *fig_ref[s], int(np.count_nonzero(g[s][sl] != ref[s][sl])), len(ref[s][sl]))
    ends = np.array([u - 1 for u, _ in states])
    ends = ends[ends < span]
    sx = np.array([by_u[u + 1]["xsum"] for u in ends], np.float32)
    sF = np.array([[by_u[u + 1][f] for f in ("f1_re", "f1_im", "f2_re", "f2_im")] for u in ends])
    line += "  xsum ne %d of %d  F ne %d of %d" % (int(np.count_nonzero(sx != ref["xsum"][ends])) if ref["dc"] else 0, len(ends), int(np.count_nonzero((sF != ref["F"][ends]).any(axis=1))), len(ends))
    print(line)
    for s, f in fig_ref.items():
        assert f[0] < REF_BOUND[s][0] and f[1] < REF_BOUND[s][1], (cid, s, "against the reference", f)

    # (c) against the float64 model, all samples, the model under the engine's own schedule
    y = I.front(cid, ref)
    mg = dict(I.model(y, ref, _engine_schedule(ref, states)), ifin=y[:n])
    mr = dict(I.model(y, ref, I.schedule_of(ref)), ifin=y[:n])
    figs = {}
    for s in g:
        figs[s] = (I.figure(g[s], mg[s]), I.figure(ref[s], mr[s]))
    ends = np.array([u - 1 for u, _ in states])
    gx, g1, g2 = I.sums_at(mg["x"], ref, ends)
    rx, r1, r2 = I.sums_at(mr["x"], ref, ends)
    sx = np.array([by_u[u + 1]["xsum"] for u in ends], np.float64)
    sF = np.array([[by_u[u + 1][f] for f in ("f1_re", "f1_im", "f2_re", "f2_im")] for u in ends])
    if ref["dc"]:
        figs["xsum"] = (I.figure(sx, gx), I.figure(ref["xsum"][ends].astype(np.float64), rx))
    figs["F"] = (I.figure(np.concatenate([sF[:, 0] + 1j * sF[:, 1], sF[:, 2] + 1j * sF[:, 3]]), np.concatenate([g1, g2])),
                 I.figure(np.concatenate([ref["F"][ends, 0] + 1j * ref["F"][ends, 1], ref["F"][ends, 2] + 1j * ref["F"][ends, 3]]), np.concatenate([r1, r2])))
    line = "IMET4SWEEP %-10s" % cid
    for s, (gm, om) in figs.items():
        line += "  %s gpu-f64 %.2e/%.2e ref-f64 %.2e/%.2e ratio %.2f/%.2f" % (s, *gm, *om, gm[0] / max(om[0], 1e-30), gm[1] / max(om[1], 1e-30))
    print(line)
    for s, (gm, om) in figs.items():
        assert gm[0] <= 3 * om[0] + FLOOR[s][0], (cid, s, "RMS against the float64 model", gm, om)
        assert gm[1] <= 3 * om[1] + FLOOR[s][1], (cid, s, "max-abs against the float64 model", gm, om)


# ----------------------------------------------------------------------------------------------- (d) cuts
def _cut_calls(cid):
    """call lengths in IF samples: the short CUTS, then (tile by tile in between, so that every sample can still be read from the rings) one
    sample before / at / after the first IQ-dc block end and the header's sample, then the long CUTS as single calls, then one sample before /
    at / after the AFC update behind the header, then the rest"""
    ref = I.reference(cid)
    k = ref["consts"]
    n = ref["n"]
    marks, pos = [], 0
    for v in [c for c in CUTS if c <= TILE + 1]:
        pos += v
        marks.append(pos)
    hdr = I.headers_of(ref)[0]
    targets = ([k["maxcnt0"] // k["decM"]] if ref["iq"] else []) + [hdr, hdr + 1]
    for t in targets:
        marks += [t - 1, t, t + 1]
    assert min(targets) - 1 > pos
    pos, long_from = max(marks), set()
    for v in [c for c in CUTS if c > TILE + 1]:
        long_from.add(pos)
        pos += v
        marks.append(pos)
    late = [p + d for p in I.updates_of(ref) if p > hdr for d in (0, 1)]
    assert not late or min(late) - 1 > pos
    for t in late:
        marks += [t - 1, t, t + 1]
    marks = sorted({m for m in marks if 0 < m < n}) + [n]
    calls, pos = [], 0
    for m in marks:
        while m - pos > TILE and pos not in long_from:
            calls.append(TILE)
            pos += TILE
        calls.append(m - pos)
        pos = m
    return calls, marks


@pytest.mark.parametrize("cid", [c["id"] for c in I.CASES])
def test_call_cuts_give_the_same_bits(cid):
    ref = I.reference(cid)
    one = _tile_run(cid)
    x = I.capture(cid)
    calls, marks = _cut_calls(cid)
    assert min(calls) == 1 and max(calls) == 2049 and sum(calls) == ref["n"]
    cut = _feed(cid, x, calls)[0]
    _same_bits("%s cut" % cid, cut["streams"], one["streams"])
    _same_state("%s cut" % cid, cut["final"], one["final"])
    _same_frames("%s cut" % cid, cut["frames"], one["frames"])
    whole = _feed(cid, x, [ref["n"]])[0]                          # one call: what the rings still hold at its end
    tail = slice(ref["n"] - (one["ring"] - 64), ref["n"])
    names = [s for s in one["streams"] if s != "ifin"]
    _same_bits("%s one call" % cid, {s: whole["streams"][s] for s in names}, {s: one["streams"][s] for s in names}, tail)
    _same_state("%s one call" % cid, whole["final"], one["final"])
    _same_frames("%s one call" % cid, whole["frames"], one["frames"])
    print("IMET4SWEEP %-10s %d calls cut at IF samples %s ...: the bits of %d tile calls and of one call of %d (ring %d)" % (cid, len(calls), marks[:12], len(one["states"]), ref["n"], one["ring"]))


@pytest.mark.parametrize("cid", ["imet48", "r2400"])
def test_calls_of_one_if_sample(cid):
    """max_chunk = decM, the smallest create accepts: calls of one IF sample from the start to two tiles past the header, a dozen turns of the
    history rings"""
    ref = I.reference(cid)
    D = ref["consts"]["decM"]
    one = _tile_run(cid)
    n = (I.headers_of(ref)[0] // TILE + 3) * TILE
    st = dict(one["states"])[n]
    got = _feed(cid, I.capture(cid), [1] * n, max_chunk=D)[0]
    assert n > 10 * got["ring"]
    _same_bits("%s 1-sample calls" % cid, got["streams"], {s: v[:n] for s, v in one["streams"].items()})
    _same_state("%s 1-sample calls" % cid, got["final"], st)
    assert got["final"]["pre_pos"] == int(ref["pre_pos"][n]) > 0


# ----------------------------------------------------------------------------------------------- (e) three channels
def test_three_captures_in_one_engine():
    cid = "imet48"
    seeds = (11, None, 12)                                       # the middle channel is the case's own capture
    X = np.stack([I.capture(cid, s) for s in seeds])
    got = _feed(cid, X, _tile_calls(cid))
    one = _tile_run(cid)
    _same_bits("middle channel", got[1]["streams"], one["streams"])
    _same_state("middle channel", got[1]["final"], one["final"])
    _same_frames("middle channel", got[1]["frames"], one["frames"])
    for ch, s in ((0, 11), (2, 12)):                             # and the neighbours are their own captures, not copies
        ref = I.reference(cid, seed=s)
        assert [f["sample"] + 1 for f in got[ch]["frames"]] == [f["sample"] for f in ref["frames"]] and len(ref["frames"]) >= 1
        f = I.figure(got[ch]["streams"]["zrot"][:2000], ref["zrot"][:2000])
        assert f[0] < 1e-6 and f[1] < 2e-5, (ch, f)
    assert not np.array_equal(got[0]["streams"]["zrot"], got[1]["streams"]["zrot"])
