"""CPU side of the iMet-4 front-end sweep (tests/imet4_front_cases.py, tests/test_gpu_imet4_front_sweep.py), from the compiled reference and
the float64 model alone — no GPU:
  - the harness (oracle/ref_imet4_harness.c, which runs the reference's own main() under instrumentation) records the frames the compiled CLI
    prints under -r (bytes) and --rawbits (bits), on every sweep capture;
  - model() equals the term-by-term sums (1e-12) and sits within the bounds of DESIGN 2 of the reference's -O2 build; the windowed sums equal
    the reference's running xsum and sliding DFT sums;
  - every row of the case table selects what it claims.
The compiled reference is read from oracle/_ref/ (make -C oracle ref)."""
import os
import re
import subprocess

import numpy as np
import pytest

import imet4_front_cases as I

IDS = [c["id"] for c in I.CASES]
# IF IQ and FM streams 1e-6 RMS, 2e-5 max-abs
BOUND = dict(ifin=(1e-6, 2e-5), zrot=(1e-6, 2e-5), zlp=(1e-6, 2e-5), fm=(1e-6, 2e-5), x=(1e-6, 2e-5))


@pytest.fixture(scope="module")
def refdir():
    from oracle import bind
    missing = [n for n in ("libref_imet4.so", "libref_imet4_O2.so", "imet4iq") if not os.path.exists(os.path.join(bind.REFDIR, n))]
    if missing:
        pytest.fail("oracle/_ref lacks %s: run `make -C oracle ref` where the reference lies" % ", ".join(missing))
    return bind.REFDIR


def _cli(refdir, cid, flag, tmp_path):
    argv, data, wav = I.cli_input(cid)
    if wav is not None:
        p = str(tmp_path / "in.wav")
        with open(p, "wb") as f:
            f.write(wav)
        argv = argv + [p]
    r = subprocess.run([os.path.join(refdir, "imet4iq"), flag] + argv, input=data, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-300:]
    return r.stdout.decode("latin-1")


@pytest.mark.parametrize("cid", IDS)
def test_harness_frames_are_the_cli_s(refdir, cid, tmp_path):
    r = I.reference(cid, "libref_imet4.so")                      # the CLI's flags
    rows = [bytes.fromhex(l.replace(" ", "")) for l in _cli(refdir, cid, "-r", tmp_path).split("\n") if re.fullmatch(r"([0-9A-F]{2} )+", l)]
    bits = [np.array([int(ch) for ch in l.replace(" ", "")], np.uint8) for l in _cli(refdir, cid, "--rawbits", tmp_path).split("\n") if re.fullmatch(r"[01 ]{100,}", l)]
    assert len(rows) == len(bits) == len(r["frames"]) >= 1, (len(rows), len(bits), len(r["frames"]))
    for b, d, f in zip(rows, bits, r["frames"]):
        assert len(b) >= 30 and bytes(f["bytes"][:len(b)]) == b
        assert len(d) == 10 * len(b) and np.array_equal(f["bits"][:len(d)], d)


@pytest.mark.parametrize("cid", IDS)
def test_model_equals_the_term_by_term_sums(refdir, cid):
    r = I.reference(cid)
    sched = I.schedule_of(r)
    y = I.front(cid, r)
    m = dict(I.model(y, r, sched), ifin=y)
    upd, hdr = I.updates_of(r), I.headers_of(r)
    probes = sorted({0, 1, 2, 37, r["consts"]["maxcnt0"] // r["consts"]["decM"] + 3, hdr[0], hdr[0] + 1, r["n"] - 1} | {p + d for p in upd for d in (0, 1, 5)})
    probes = [p for p in probes if 0 <= p < r["n"]]
    lit = I.literal(cid, r, sched, probes)
    for s in ("ifin", "zrot", "zlp", "fm", "x"):
        if m[s] is not None:
            assert np.abs(lit[s] - np.asarray(m[s])[probes]).max() < 1e-12, s


@pytest.mark.parametrize("cid", IDS)
def test_model_against_the_o2_reference(refdir, cid):
    r = I.reference(cid)
    y = I.front(cid, r)
    m = dict(I.model(y, r, I.schedule_of(r)), ifin=y[:r["n"]])
    line = "IMET4MODEL %-10s" % cid
    for s in ("ifin", "zrot", "zlp", "fm", "x"):
        if r[s] is None:
            continue
        assert len(r[s]) == r["n"]
        f = I.figure(r[s], m[s])
        line += "  %s %.2e/%.2e" % (s, *f)
        assert f[0] < BOUND[s][0] and f[1] < BOUND[s][1], (cid, s, f)
    # the running sums at every 997th sample and around the AFC updates: the float32 xsum recursion within 1e-3 of the windowed sum of the
    # reference's own x (|xsum| < 128: 55 200 roundings of at most 2^-18 each add up to at most 0.2, as a random walk to 5e-4), the double
    # DFT recursion within 1e-9
    probes = sorted(set(range(0, r["n"], 997)) | {p for u in I.updates_of(r) for p in (u - 1, u) if p >= 0})
    xs, F1, F2 = I.sums_at(r["x"].astype(np.float64), r, probes)
    ex, e1, e2 = np.abs(xs - r["xsum"][probes]).max(), np.abs(F1 - (r["F"][probes, 0] + 1j * r["F"][probes, 1])).max(), np.abs(F2 - (r["F"][probes, 2] + 1j * r["F"][probes, 3])).max()
    print(line + "  xsum %.2e F1 %.2e F2 %.2e" % (ex, e1, e2))
    if r["dc"]:
        assert ex < 1e-3
    assert e1 < 1e-9 and e2 < 1e-9


@pytest.mark.parametrize("cid", IDS)
def test_row_selects_what_it_claims(refdir, cid):
    c = I.BY_ID[cid]
    r, rf = I.reference(cid), I.reference(cid, "libref_imet4.so")
    k = r["consts"]
    want = dict(imet48=(48000, 1), imet1_96=(96000, 1), imet48_u8=(48000, 1), r2400=(48000, 50), wav48=(48000, 1), wav48_dc=(48000, 1))[cid]
    assert (k["if_sr"], k["decM"]) == want and r["n"] == rf["n"] == int(round(I.SECONDS * I.sr_of(c))) // k["decM"]
    hdr, upd = I.headers_of(r), I.updates_of(r)
    assert len(hdr) == 1 and len(r["frames"]) == 1 and r["frames"][0]["sample"] < r["n"]          # one header, one complete frame
    assert hdr == I.headers_of(rf) and np.array_equal(r["pre_pos"], rf["pre_pos"])
    assert hdr[0] % 64 != 63                                      # the header falls inside a 64-sample tile: the tile is cut short and redone
    assert int(r["pre_pos"][-1]) > 0
    if c["opt"].get("dc"):
        assert len(upd) >= 2 and upd[0] == 0 and upd[-1] > hdr[0] and upd == I.updates_of(rf)     # an update behind the header, under its phase
        assert (upd[-1] + int(r["pre_pos"][-1])) % k["if_sr"] == 0 and upd[-1] % k["if_sr"] != 0
        assert set(I.changes_of(r)) <= set(upd) and upd[-1] in I.changes_of(r)
        assert r["df"][-1] != 0 and abs(r["df"][-1] - rf["df"][-1]) < 1.0
        if r["iq"]:
            assert r["nominal"][0] == 0 and r["nominal"][1:].all()                                # acquisition -> nominal tap set at the first update
            assert upd[-1] % 64 != 63                             # the update point ends a tile early
    else:
        assert upd == [] and not r["df"].any()
    if r["iq"]:
        n_base = len(I.capture(cid)) // 2
        ends = [b + m for b, m in I.K.iqdc_blocks(n_base, k["maxcnt0"], k["maxlim"])]
        assert len(ends) >= 2 and len(r["dcev"]) == len(ends)                                     # IQ-dc block ends inside the capture
        _, means = I.K.iqdc_mean(I.K.samples_of(I.capture(cid), I.bits_of(c)), k["maxcnt0"], k["maxlim"])
        for (end, a), ev in zip(means, r["dcev"]):
            assert (np.float32(a.real), np.float32(a.imag)) == (np.float32(ev[1]), np.float32(ev[2])), (end, a, ev)
    if cid == "wav48_dc":
        assert k["fm_taps"] > 1 and np.abs(r["dc_of"]).max() > 0.01                               # v - dc 0.4 with a dc that matters
    if cid == "imet48_u8":
        assert I.capture(cid).dtype == np.uint8
