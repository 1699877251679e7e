"""The decimator sweep's table (tests/decim_sweep_cases.py) against the reference's design arithmetic — no GPU.

Every row names the kernel variant it is there for; which variant an engine picks follows from D, T, Q = ceil(T / D) and
lut_len % D alone (sonde_engine.cpp / sonde_launch_mix_decimate).  The numbers come from the compiled reference's `consts`
(oracle/_ref, init_buffers of demod_mod.c) where it is present and from the CPU oracle's otherwise; the oracle's stream entry
has no --min switch, so without the compiled reference the --min rows are checked against the same arithmetic written out
here (demod_mod.c:1222-1249)."""
import numpy as np
import pytest
from decim_sweep_cases import SWEEP, LONG, REFUSED, case_id, wide_ds


def _design_min(sr, opt_min):
    if_sr = 32000 if opt_min else 48000
    D = 1
    if if_sr > sr:
        if_sr = sr
    if if_sr < sr:
        while sr % if_sr:
            if_sr += 1
        D = sr // if_sr
    t_bw = np.float32(if_sr - (12e3 if opt_min else 20e3))
    if t_bw < 0:
        t_bw = np.float32(10e3)
    t_bw = np.float32(t_bw / np.float32(sr))
    taps = int(4.0 / float(t_bw))
    taps += 1 - taps % 2
    d = next(k for k in range(16, 0, -1) if sr % k == 0)
    return dict(if_sr=if_sr, decM=D, dectaps=taps, lut_len=sr // d)


def _consts(oracle, c):
    x = np.zeros(2 * 4 * c["D"], np.int16)
    if oracle.have_ref():
        return oracle.ref_streams(x, c["sr"], fq=c["fq"], lp_iq=False, libname="libref_demod_O2.so", opt_min=c["opt_min"])["consts"]
    if c["opt_min"]:
        return _design_min(c["sr"], True)
    return oracle.ora_streams(x, c["sr"], fq=c["fq"], lp_iq=False)["consts"]


@pytest.mark.parametrize("c", SWEEP + [LONG, REFUSED], ids=case_id)
def test_row_selects_what_it_claims(oracle, c):
    k = _consts(oracle, c)
    assert (k["if_sr"], k["decM"], k["dectaps"], k["lut_len"]) == (c["if_sr"], c["D"], c["T"], c["lut_len"])
    if not c["opt_min"]:                                       # the restatement above is the oracle's / the reference's arithmetic
        m = _design_min(c["sr"], False)
        assert (m["if_sr"], m["decM"], m["dectaps"], m["lut_len"]) == (c["if_sr"], c["D"], c["T"], c["lut_len"])
    D, T = c["D"], c["T"]
    Q = -(-T // D)
    name = c["kernel"]
    if name.startswith("k_mix_decimate50"):
        assert D == 50 and Q == 7 and c["lut_len"] % D == 0
        if "pad" in name:
            assert Q * D - T == int(name.split("pad")[1])
    elif name.startswith("wide"):
        assert D > 64 and 5 <= Q <= 8 and wide_ds(D) == int(name.split("DS")[1])
    elif name.startswith("generic"):
        assert D <= 64 and Q <= 8 and not (D == 50 and Q == 7)
        if "Q 6" in name:
            assert Q == 6 and c["lut_len"] % D != 0
        if "D 64" in name:
            assert D == 64 and 4 * (64 * D + 4) * 4 == 65600
    else:
        assert D > 64 and wide_ds(D) == 0                      # the refused rate: no piece length divides a prime D


def test_sweep_covers_every_variant_and_the_fq_edges():
    kinds = {c["kernel"].split(",")[0].split(" Q")[0].split(":")[0] for c in SWEEP}
    assert {"generic", "k_mix_decimate50", "wide"} <= kinds
    assert sorted(c["sr"] for c in SWEEP if not c["opt_min"]) == [130_000, 250_000, 1_024_000, 1_800_000, 2_048_000, 2_400_000, 2_500_000,
                                                                  2_560_000, 3_072_000, 3_200_000, 3_600_000, 6_000_000]
    assert sorted(c["sr"] for c in SWEEP if c["opt_min"]) == [1_600_000, 2_048_000, 2_400_000]
    fqs = [c["fq"] for c in SWEEP]
    assert 0.0 in fqs and any(0.48 <= abs(f) < 0.5 for f in fqs) and len(set(fqs)) == len(fqs)
