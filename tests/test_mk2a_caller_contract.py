"""auto_rx's own handling of the decoder's stdout (auto_rx/autorx/decode.py: lines are read one by one, everything that does not start with
"{" is dropped, the rest goes through json.loads and must carry the fields the MK2LMS branch reads) applied to the JSON lines of the goldens,
which host/bin/mk2a1680mod reproduces byte for byte (tests/test_gpu_mk2a.py), and to the printer's own lines."""
import json

from tests import mk2a_cases as cases
from tools import synth

FIELDS = ("type", "frame", "id", "datetime", "lat", "lon", "alt", "vel_h", "heading", "vel_v", "subtype", "ref_datetime", "ref_position", "version")


def _handle(stdout: bytes):
    """decode.py's reader loop: a line is telemetry when it is not empty and starts with '{'"""
    out = []
    for line in stdout.decode("ascii").split("\n"):
        if line is None or line == "":
            continue
        if line[0] != "{":
            continue
        out.append(json.loads(line))
    return out


def test_json_lines_of_the_goldens_pass_the_callers_reader():
    seen = 0
    for name in sorted(cases.CASES):
        g = cases.load(name)
        for argv, out in zip(g["argv"], g["stdout"]):
            assert out.endswith(b"\n")
            for js in _handle(out):
                seen += 1
                for f in FIELDS:
                    assert f in js, (name, f)
                assert js["type"] == "LMS" and js["subtype"] == "MK2A" and js["id"].startswith("LMS6-") and js["version"] == "oracle"
                assert len(js["datetime"]) == len("12:34:01.250Z") and js["datetime"].endswith("Z")
                assert ("freq" in js) == ("--jsn_cfq" in argv)
    assert seen > 60


def test_printer_lines_pass_the_callers_reader():
    from radiosonde_auto_rx_amd.mk2a import Mk2aPrinter
    p = Mk2aPrinter(json=True, jsn_freq_khz=1680240, version="1.2.3")
    text = ""
    for k in range(3):
        f, m = synth.mk2a_subframes(k)
        for x in (f, m):
            text += p.frame(synth.mk2a_bits(x + b"\xCA" * 4)[:1760])
    js = _handle(text.encode())
    assert [j["frame"] for j in js] == [101, 102] and js[0]["freq"] == 1680240 and js[0]["version"] == "1.2.3"
    assert js[0]["id"] == "LMS6-12345678" and abs(js[0]["lat"] - 41.2345) < 1e-4
