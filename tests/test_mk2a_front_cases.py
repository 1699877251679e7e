"""CPU side of the MkIIa front-end sweep (tests/mk2a_front_cases.py, tests/test_gpu_mk2a_front_sweep.py), from the compiled reference and
the float64 model alone — no GPU:
  - the harness (oracle/ref_mk2a_harness.c, which runs the reference's own main() under instrumentation) records the frames, mv and Df
    the compiled CLI prints under -r -vv, on every sweep capture;
  - model() equals the term-by-term sums (1e-12) and sits within the bounds of DESIGN 2 of the reference's -O2 build;
  - every row of the case table selects what it claims.
The compiled reference is read from oracle/_ref/ (make -C oracle ref)."""
import re

import numpy as np
import pytest

import mk2a_front_cases as K

IDS = [c["id"] for c in K.CASES]
MODEL_IDS = [c["id"] for c in K.CASES if c.get("model", True)]
# IF IQ and FM streams 1e-6 RMS (IQ 2e-5 max-abs), tone-correlator stream and bufs 1e-5 RMS
BOUND = dict(ifin=(1e-6, 2e-5), zlp=(1e-6, 2e-5), fm=(1e-6, 2e-5), fmbuf=(1e-6, 2e-5), sraw=(1e-5, 2e-5), bufs=(1e-5, 2e-5))


@pytest.fixture(scope="module")
def refdir():
    from oracle import bind, ref_front
    import os
    missing = [n for n in ("libref_mk2a.so", "libref_mk2a_O2.so", "mk2a1680mod") if not os.path.exists(os.path.join(bind.REFDIR, n))]
    if missing:
        pytest.fail("oracle/_ref lacks %s: run `make -C oracle ref` where the reference lies" % ", ".join(missing))
    return ref_front


@pytest.mark.parametrize("cid", IDS)
def test_harness_frames_are_the_cli_s(refdir, cid):
    """-r prints every frame's bytes (bits2bytes, trailing CA trimmed by the CRC rule), -vv `<s=%+.2f Df=%+.1fkHz>` in front of every 54 subframe"""
    from oracle import bind
    c = K.BY_ID[cid]
    r = K.reference(cid, "libref_mk2a.so")                       # the CLI's flags
    out, err, rc = bind.ref_run("mk2a1680mod", ["-r", "-vv"] + K.cli_argv(c), K.capture(cid))
    assert rc == 0 and "IF: %d" % r["consts"]["if_sr"] in err and "dec: %d" % r["consts"]["decM"] in err
    raw = []                                                     # (bytes, the <s= Df=> text behind it or None)
    for line in out.split("\n"):
        if re.fullmatch(r"([0-9a-f]{2} )+", line):
            raw.append([bytes.fromhex(line.replace(" ", "")), None])
        m = re.match(r"<s=([+-]\d+\.\d\d)( Df=([+-]\d+\.\d)kHz)?>", line)
        if m:
            raw[-1][1] = (m.group(1), m.group(3))
    assert len(raw) == len(r["frames"]) >= 1, (len(raw), len(r["frames"]))
    seen = 0
    for (b, txt), f in zip(raw, r["frames"]):
        assert bytes(f["bytes"][:len(b)]) == b and len(b) <= int(f["nbits"]) // 10
        if txt:
            seen += 1
            assert txt[0] == "%+.2f" % f["mv"], (txt, f["mv"])
            if c["opt"]["dc"]:
                assert txt[1] == "%+.1f" % (f["Df"] / 1e3), (txt, f["Df"])
    assert seen >= 1


@pytest.mark.parametrize("cid", MODEL_IDS)
def test_model_equals_the_term_by_term_sums(refdir, cid):
    r = K.reference(cid)
    sched = K.schedule_of(r)
    d = r["consts"]["decFM"]
    z = K.front_of(cid)
    m = K.model(z, r, sched, r["n_if"])
    last = sched[-1][0]
    pi = sorted({0, 1, 2, 37, r["consts"]["maxcnt0"] // r["consts"]["decM"] + 3, last - 1, last, last + 5, r["n_if"] - 1} - {-1})
    po = sorted({0, 9, (last + d) // d, r["n_out"] - 1})
    lit = K.literal(K.capture(cid), K.bits_of(K.BY_ID[cid]), r, sched, pi, po)
    assert np.abs(lit["ifin"] - z[pi]).max() < 1e-12
    for s in ("zrot", "zlp", "fm", "sraw"):
        if m[s] is not None:
            assert np.abs(lit[s] - m[s][pi]).max() < 1e-12, s
    for s in ("bufs", "fmbuf"):
        assert np.abs(lit[s] - m[s][po]).max() < 1e-12, s


@pytest.mark.parametrize("cid", MODEL_IDS)
def test_model_against_the_o2_reference(refdir, cid):
    r = K.reference(cid)
    z = K.front_of(cid)
    m = dict(K.model(z, r, K.schedule_of(r), r["n_if"]), ifin=z)
    line = "MK2AMODEL %-11s" % cid
    for s in ("ifin", "zlp", "fm", "sraw", "bufs", "fmbuf"):
        if r[s] is None:
            continue
        f = K.figure(r[s], m[s])
        line += "  %s %.2e/%.2e" % (s, *f)
        assert f[0] < BOUND[s][0] and f[1] < BOUND[s][1], (cid, s, f)
    print(line)
    for s in ("ifin", "zlp", "fm", "sraw", "bufs", "fmbuf"):      # every sample of every stream was recorded, the tone stream inside frames too
        assert r[s] is None or (len(r[s]) == (r["n_out"] if s in ("bufs", "fmbuf") else r["n_if"]) and not np.isnan(r[s]).any()), s


@pytest.mark.parametrize("cid", IDS)
def test_row_selects_what_it_claims(refdir, cid):
    c = K.BY_ID[cid]
    r, rf = K.reference(cid), K.reference(cid, "libref_mk2a.so")
    k = r["consts"]
    want = dict(auto240=(1, 4), auto240_u8=(1, 4), r960=(5, 4), r960min=(6, 4), r2400=(12, 4), IQ240=(1, 4), lpfm240=(1, 1), decfm2=(1, 2), zeros8=(1, 4))[cid]
    assert (k["decM"], k["decFM"]) == want
    assert len(r["win"]) >= 3 and sum(int(w["found"]) for w in r["win"]) >= 1 and len(r["frames"]) >= 1
    assert any(int(f["sample"]) < r["n_out"] for f in r["frames"])                   # a complete frame: ended by sync or the length limit, not by the end of the capture
    assert [int(w["sample"]) for w in r["win"]] == [int(w["sample"]) for w in rf["win"]]
    sched = K.schedule_of(r)
    if c["opt"]["dc"]:
        assert len({s[1] for s in sched}) >= 3, sched                               # Df = 0 and at least two AFC steps
        assert sched[0][2] == 0 and any(s[2] == 1 for s in sched)                   # acquisition -> nominal tap set (for --IQ without --lpIQ: unlock -> lock)
        assert sched[1][0] < r["n_if"] // 2
    else:
        assert sched == [(0, 0.0, 1)]
    ends = [b + m for b, m in K.iqdc_blocks(len(K.capture(cid)) // 2, k["maxcnt0"], k["maxlim"])]
    assert len(ends) >= 2 and len(r["dcev"]) == len(ends)                           # IQ-dc block ends inside the capture, and the reference saw as many means
    x = K.samples_of(K.capture(cid), K.bits_of(c))
    _, means = K.iqdc_mean(x, k["maxcnt0"], k["maxlim"])
    for (end, a), ev in zip(means, r["dcev"]):
        assert (np.float32(a.real), np.float32(a.imag)) == (np.float32(ev[1]), np.float32(ev[2])), (end, a, ev)
    if cid == "IQ240":
        assert r["win"][0]["mv2"] != 0.0 and k["iqfm_taps"] > 1 and k["fm_taps"] > 1 and len(r["tone"]) >= 3 and r["sraw"] is not None
    if cid == "zeros8":
        assert (K.capture(cid)[:2 * c["silence"]] == 128).all() and (r["zlp"][:c["silence"] - 40] == 0).all()
    if cid == "auto240_u8":
        assert K.capture(cid).dtype == np.uint8
