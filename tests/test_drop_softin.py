"""rd94rd41drop --softin / --softinv (host code, no GPU): the goldens hold the sign of every soft bit that the reference's fsk_demod wrote
for a capture and the reference decoder's stdout on them; the decoder looks at the sign only (bit = s >= 0 after the inversions), so the
framer fed with +-1 floats — in pieces of several sizes — and the printer must give that stdout byte for byte."""
import numpy as np
import pytest

from tests import drop_cases as cases
from tests.test_drop_fields import _printer

SOFT = sorted(n for n, c in cases.CASES.items() if c["gen"].get("form") == "soft")


def _soft(sign):
    """floats with the golden's signs; a zero stays +0.0, which is >= 0 and, negated, still >= 0, as in the reference"""
    return sign.astype(np.float32)


@pytest.mark.parametrize("name", SOFT)
@pytest.mark.parametrize("piece", [1 << 20, 4096, 2401, 63])
def test_framer_on_the_reference_modems_signs(name, piece):
    from radiosonde_auto_rx_amd.drop import DropSoftin
    g = cases.load(name)
    s = _soft(g["soft_sign"])
    assert len(s) > 8 * 2400
    for argv, ref in zip(g["argv"], g["stdout"]):
        si, p, text = DropSoftin(invert=("--softinv" in argv) != ("-i" in argv)), _printer(argv), ""
        for k in range(0, len(s), piece):
            for f in si.push(s[k:k + piece]):
                assert f["complete"] and f["nraw"] == 2400
                text += p.frame(f["bytes"])
        assert text.encode() == ref, (name, argv, text[-500:], ref[-500:])


def test_soft_goldens_meet_the_conditions_on_clean_cases():
    for name in SOFT:
        g = cases.load(name)
        n = [o.count(b'"type"') for o in g["stdout"]]
        if name in cases.CLEAN:
            assert n[cases.CLEAN[name]] >= cases.N_FRAMES - 1, (name, n)
    g = cases.load("soft41")
    assert g["stdout"][3] == b""                                             # --softin without -i on a capture that needs --softinv: nothing


def test_zero_soft_bits_count_as_one_in_both_polarities():
    from radiosonde_auto_rx_amd.drop import DropSoftin
    from tools import synth
    raw = synth.drop_rawbits([b"\x1A\xCF"] + synth.drop_frames(2, 41)).astype(np.float32)        # bit 1 -> 1.0, bit 0 -> 0.0: all >= 0
    assert DropSoftin().push(raw) == [] and DropSoftin(invert=True).push(raw) == []
    soft = 2 * raw - 1
    fr = DropSoftin().push(soft)
    assert [f["err41"] for f in fr] == [0, 0] and fr[0]["sample"] == 40 + 40 and fr[1]["sample"] == 40 + 2400 + 40
    assert [f["err41"] for f in DropSoftin(invert=True).push(-soft)] == [0, 0]
