"""auto_rx's own handling of the decoder's stdout (auto_rx/autorx/decode.py: lines are read one by one, everything that does not start with
"{" is dropped, the rest goes through json.loads and must carry the fields the WXR301 / WXRPN9 branches read) applied to the JSON lines of
the goldens, which host/bin/weathex301d reproduces byte for byte (tests/test_gpu_wxr.py, tests/test_wxr_softin.py), and to the printer's own."""
import json

import numpy as np

from tests import wxr_cases as cases
from tools import synth

FIELDS = ("type", "frame", "id", "datetime", "lat", "lon", "alt", "ref_datetime", "ref_position", "version")


def _handle(stdout: bytes):
    """decode.py's reader loop: a line is telemetry when it is not empty and starts with '{'"""
    out = []
    for line in stdout.decode("latin-1").split("\n"):
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
                assert js["type"] == "WXR301" and js["id"].startswith("WXR-") and js["version"] == "oracle"
                assert js["ref_datetime"] == "UTC" and js["ref_position"] == "MSL"
                assert len(js["datetime"]) == len("12:34:01Z") and js["datetime"].endswith("Z")
                assert (js.get("subtype") == "WXR_PN9") == ("--pn9" in argv) and ("subtype" in js) == ("--pn9" in argv)
                assert ("freq" in js) == ("--jsn_cfq" in argv)
                if "--jsn_cfq" in argv:
                    assert js["freq"] == (int(argv[argv.index("--jsn_cfq") + 1]) + 500) // 1000
    assert seen > 150


def test_printer_lines_pass_the_callers_reader():
    from radiosonde_auto_rx_amd.wxr import WxrPrinter
    for pn9 in (False, True):
        p = WxrPrinter(json=True, pn9=pn9, jsn_freq_khz=403240, version="1.2.3")
        text = "".join(p.frame(np.unpackbits(np.frombuffer(f, np.uint8))) for f in synth.wxr_frames(6, pn9))
        js = _handle(text.encode())
        assert [j["frame"] for j in js] == [100, 101, 102] and js[0]["freq"] == 403240 and js[0]["version"] == "1.2.3"
        assert js[0]["id"] == "WXR-20230117" and abs(js[0]["lat"] - 52.20912) < 1e-5 and (js[0].get("subtype") == "WXR_PN9") == pn9
        for f in FIELDS:
            assert f in js[0]
