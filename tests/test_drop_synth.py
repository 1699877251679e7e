"""The dropsonde generator (tools/synth.py drop_*) and the design numbers of the engine (host code, no GPU)."""
import numpy as np

from tests import drop_cases as cases
from tools import synth


def test_generator_is_pinned_by_its_seed():
    a = synth.drop_capture(seed=3, n_frames=2)
    assert a.dtype == np.int16 and len(a) == 2 * (2 * 12000 + (2 * 2400 + 40) * 10) and np.array_equal(a, synth.drop_capture(seed=3, n_frames=2))
    assert not np.array_equal(a, synth.drop_capture(seed=4, n_frames=2))
    f = synth.drop_frame(41, 100)
    assert f[:2] == b"\xFC\x1D" and f[118:] == b"\x1A\xCF" and len(f) == 120 and f == synth.drop_frames(1, 41)[0]


def test_rawbits_are_manchester_coded_8n1_and_start_with_the_header_the_decoder_searches():
    raw = synth.drop_rawbits([synth.drop_frame(94, 0)])
    assert len(raw) == 2400 and np.all(raw[0::2] != raw[1::2])
    hdr = "10101001010101010101" "10011001010110101001"
    assert "".join(map(str, raw[:40])) == hdr
    bits = raw[1::2].reshape(120, 10)
    assert np.all(bits[:, 0] == 0) and np.all(bits[:, 9] == 1)
    assert bytes(np.packbits(bits[:, 1:9], axis=1, bitorder="little").reshape(-1)) == synth.drop_frame(94, 0)


def test_design_gives_the_references_stderr_numbers():
    from radiosonde_auto_rx_amd import drop
    for name in ("clean41", "wav8", "wide41_2400k", "br94"):
        g = cases.load(name)
        front = g["front"]
        sr = int(front[-2]) if front else 48000
        for argv, err in zip(g["argv"], g["stderr"]):
            br = float(argv[argv.index("--br") + 1]) if "--br" in argv else 0.0
            d = drop.design(sr, baud=br)
            assert d["if_rate"] == 48000 and d["dec_m"] == sr // 48000
            lines = err.decode().split("\n")
            assert "samples/bit: %.2f" % drop.design(48000, input=drop.IN_FM)["sps"] in lines
            if br:
                assert "corr: %.4f" % d["sps"] in lines
    assert drop.design(48000, input=drop.IN_FM, baud=4798.8)["sps"] == np.float32(48000) / np.float32(4798.8)
    assert drop.design(48000, baud=5000.0)["sps"] == 10.0
    assert g["front_stderr"] is not None


def test_every_case_has_its_golden_and_the_clean_ones_give_every_frame():
    for name, case in cases.CASES.items():
        g = cases.load(name)
        assert g["argv"] == case["argv"] and g["front"] == case["front"] and g["params"] == cases.json.loads(cases.json.dumps(case["gen"])), name
        assert g["rc"] == [case.get("rc", 0)] * len(case["argv"])
    for name, i in cases.CLEAN.items():
        g = cases.load(name)
        soft = cases.CASES[name]["gen"].get("form") == "soft"
        assert g["stdout"][i].count(b'"type"') >= cases.N_FRAMES - (1 if soft else 0), name
    # the branches the flips cases are there for: text without JSON, no text at all, RD41 frames typed RD94
    g = cases.load("flips41")
    r = g["stdout"][1].decode().split("\n")                                      # -R
    assert sum("# chk: 00001" in l or "# chk: 0000010" in l for l in r) >= 2 and any(l.endswith("# chk: 11111") for l in r)
    assert cases.load("wav32")["stdout"] == [b""]
