"""sonde_wxr_design against the stderr lines of the goldens (iq_dec's "IF:" / "dec:", weathex301d's "samples/bit:"), and the generator pinned by
the reference decoding it: every golden of a clean case holds exactly the frames tools.synth.wxr_frames put into the capture."""
import re

import pytest

from tests import wxr_cases as cases


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_design_equals_the_references_stderr(name):
    from radiosonde_auto_rx_amd import wxr
    case, g = cases.CASES[name], cases.load(name)
    form = case["gen"].get("form", "cs16")
    if form == "soft":
        assert all(e == b"" for e in g["stderr"])                 # --softin reads no header and prints nothing
        return
    pn9 = bool(case["gen"].get("pn9"))
    if case["front"] is not None:
        sr, bits = int(case["front"][-2]), int(case["front"][-1])
        d = wxr.design(sr, bits=bits, pn9=pn9, if_bw_khz=64)
        assert g["front_stderr"] == b"IF: %d\ndec: %d\n" % (d["if_rate"], d["dec_m"])
        assert d["taps_fm"] == (4 * d["if_rate"] // 2000) | 1
        wav_bits, nch, rate = 32, 1, d["if_rate"]
    else:
        wav_bits, nch, rate = {"wav16": (16, 1), "wav8": (8, 1), "wav32": (32, 1), "wav2ch": (16, 2)}[form] + (96000,)
        d = wxr.design(rate, input=wxr.IN_FM, bits=wav_bits, pn9=pn9)
        assert d["if_rate"] == rate and d["dec_m"] == 1 and d["taps_fm"] == 0
    want = b"sample_rate: %d\nbits       : %d\nchannels   : %d\nsamples/bit: %.2f\n" % (rate, wav_bits, nch, d["sps"])
    for err in g["stderr"]:
        assert err == want, (name, err, want)


def test_design_numbers():
    from radiosonde_auto_rx_amd import wxr
    assert wxr.design(96000) == dict(if_rate=96000, dec_m=1, taps_dec=0, taps_fm=193, sps=20.0)
    d = wxr.design(2400000)
    assert (d["if_rate"], d["dec_m"], d["sps"]) == (75000, 32, 15.625)
    assert abs(wxr.design(96000, pn9=True)["sps"] - 19.2) < 1e-6
    assert wxr.design(900001, input=wxr.IN_FM, bits=16)["if_rate"] == 900000


@pytest.mark.parametrize("name", cases.CLEAN)
def test_clean_goldens_hold_the_generators_frames(name):
    case, g = cases.CASES[name], cases.load(name)
    want = [" ".join("%02X" % b for b in f) for f in cases.frames_in(case)]
    raw = [i for i, a in enumerate(g["argv"]) if "-r" in a]
    if raw:
        lines = [l for l in g["stdout"][raw[0]].decode().split("\n") if "[OK]" in l]
        got = [re.sub(r"^<[ 0-9.]*> ", "", l)[:69 * 3 - 1] for l in lines]
        assert got == want, name
    js = [i for i, a in enumerate(g["argv"]) if "--json" in a]
    if js:                                                      # one JSON line per id-1 / id-2 pair
        import json
        objs = [json.loads(l) for l in g["stdout"][js[0]].decode().split("\n") if l.startswith("{")]
        assert [o["frame"] for o in objs] == [100 + k for k in range(len(want) // 2)] and all(o["id"] == "WXR-20230117" for o in objs)
        assert abs(objs[1]["lat"] - 52.20922) < 1e-5 and abs(objs[1]["lon"] - 14.12014) < 1e-5 and abs(objs[1]["alt"] - 1239.5) < 1e-3
        assert objs[1]["datetime"] == "12:34:41Z"
