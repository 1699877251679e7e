"""The WxR-301D printer (sonde_wxr_print_frame, host code): on the frames of the goldens' own -R lines it prints what the reference printed for
the same capture as text, -r and JSON, byte for byte, both variants; wrong check, unpaired id-2 frame and zero position give no JSON."""
import numpy as np
import pytest

from tests import wxr_cases as cases
from tools import synth


def _bits_of(stdout: bytes):
    return [np.array([int(c) for c in l], np.uint8) for l in stdout.decode("latin-1").split("\n") if len(l) == 552]


def _bits(frame: bytes):
    return np.unpackbits(np.frombuffer(frame, np.uint8))


def _printer(**kw):
    from radiosonde_auto_rx_amd.wxr import WxrPrinter
    return WxrPrinter(version="oracle", **kw)


@pytest.mark.parametrize("name,pn9", [("clean", False), ("clean_pn9", True)])
def test_printer_on_the_goldens_frames(name, pn9):
    g = cases.load(name)
    pn = ["--pn9"] if pn9 else []
    frames = _bits_of(g["stdout"][g["argv"].index(["-R"] + pn)])
    assert len(frames) == 16
    # these captures are clean: the -b runs frame the same bits as the runs without -b, so one set of -R lines serves all argument lists
    for argv, kw in ((["-b", "--json"] + pn, dict(json=True)), (["-b", "-r", "-v"] + pn, dict(raw=1, vbs=True)), (["-R"] + pn, dict(raw=2)),
                     (["-b", "--json"] + pn + ["--jsn_cfq", "403000000"], dict(json=True, jsn_freq_khz=403000)), (["--json"] + pn, dict(json=True))):
        ref = g["stdout"][g["argv"].index(argv)]
        p = _printer(pn9=pn9, **kw)
        text = "".join(p.frame(f) for f in frames) + "\n"
        assert text.encode("latin-1") == ref, (name, argv)
    v = [a for a in g["argv"] if "-v" in a and "-r" not in a][0]
    p = _printer(pn9=pn9, vbs=True, json="--json" in v)
    assert ("".join(p.frame(f) for f in frames) + "\n").encode("latin-1") == g["stdout"][g["argv"].index(v)]


@pytest.mark.parametrize("pn9", [False, True])
def test_json_needs_check_pairing_and_position(pn9):
    def run(frames, **kw):
        p = _printer(pn9=pn9, json=True, **kw)
        return "".join(p.frame(_bits(f)) for f in frames)

    f1, f2 = synth.wxr_frame(777, 5, 1, pn9), synth.wxr_frame(777, 5, 2, pn9)
    t = run([f1, f2])
    assert t.count("[OK]") == 1 and t.count('"type": "WXR301"') == 1 and '"id": "WXR-777"' in t and '"frame": 5' in t
    assert ('"subtype": "WXR_PN9"' in t) == pn9 and t.endswith(" }\n\n")
    t = run([f1, synth.wxr_frame(777, 5, 2, pn9, corrupt=True)])                   # wrong check
    assert "[NO]" in t and "{" not in t
    assert "{" not in run([f2])                                                    # no id-1 frame before
    assert "{" not in run([synth.wxr_frame(777, 4, 1, pn9), f2])                   # id-1 frame of another counter
    assert "{" not in run([synth.wxr_frame(778, 5, 1, pn9), f2])                   # ... of another serial
    assert "{" not in run([synth.wxr_frame(777, 5, 1, pn9, corrupt=True), f2])     # ... with a wrong check
    t = run([f1, synth.wxr_frame(777, 5, 2, pn9, lat=0.0, lon=0.0, alt_m=0.0)])   # zero position
    assert t.count("[OK]") == 1 and "{" not in t
    assert '"freq": 403000' in run([f1, f2], jsn_freq_khz=403000)
    assert run([f1], vbs=True).startswith(" (777)  [    5]   [OK] # [")


def test_unset_bits_print_as_nul_and_count_as_zero():
    p = _printer(raw=2)
    b = np.full(552, 2, np.uint8)
    b[:40] = _bits(bytes.fromhex("AAAAAA2DD4"))
    t = p.frame(b)
    assert len(t) == 553 and t[40:552] == "\0" * 512 and t[-1] == "\n"
    assert _printer(raw=1).frame(b).startswith("AA AA AA 2D D4 00 00 ")


def test_xor8sum_known_answers():
    from radiosonde_auto_rx_amd.wxr import xor8sum
    assert xor8sum(b"") == 0
    assert xor8sum(b"\x01\x02\x03") == 0x0006
    assert xor8sum(b"\xFF\xFF") == 0x00FE
    assert xor8sum(bytes(range(53))) == ((0 ^ 52) << 8 | (sum(range(53)) & 0xFF)) and synth.wxr_xor8sum(bytes(range(53))) == xor8sum(bytes(range(53)))
    assert xor8sum(b"\x80\x81") == 0x0101
