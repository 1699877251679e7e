"""auto_rx's own handling of the decoder's stdout (auto_rx/autorx/decode.py: lines are read one by one, everything that does not start with
"{" is dropped, the rest goes through json.loads; the RD94RD41 branch takes the sonde type from the "type" field and the frequency from
"freq" when it is there) applied to the JSON lines of the goldens, which host/bin/rd94rd41drop reproduces byte for byte
(tests/test_gpu_drop.py), and to the printer's own."""
import json
import re

from tests import drop_cases as cases
from tools import synth

FIELDS = ("type", "frame", "id", "datetime", "lat", "lon", "alt", "vel_h", "heading", "vel_v", "sats", "temp", "humidity", "pressure",
          "ref_datetime", "ref_position", "version")


def _handle(stdout: bytes):
    """decode.py's reader loop: a line is telemetry when it is not empty and starts with '{'"""
    out = []
    for line in stdout.decode("utf-8").split("\n"):
        if line is None or line == "":
            continue
        if line[0] != "{":
            continue
        out.append(json.loads(line))
    return out


def _check(js, argv):
    for f in FIELDS:
        assert f in js, f
    assert js["type"] in ("RD94", "RD41") and re.fullmatch(r"\d{9}", js["id"])
    if js["type"] == "RD94":
        assert re.fullmatch(r"\d{4}-\d\d-\d\dT\d\d:\d\d:\d\d\.\d{3}Z", js["datetime"]) and js["ref_datetime"] == js["ref_position"] == "GPS"
    else:
        assert re.fullmatch(r"\d\d:\d\d:\d\d\.\d\dZ", js["datetime"]) and js["ref_datetime"] == "UTC" and js["ref_position"] == "MSL"
    assert ("freq" in js) == ("--jsn_cfq" in argv)
    if "--jsn_cfq" in argv:
        assert js["freq"] == (int(argv[argv.index("--jsn_cfq") + 1]) + 500) // 1000


def test_json_lines_of_the_goldens_pass_the_callers_reader():
    seen = {"RD94": 0, "RD41": 0}
    for name in sorted(cases.CASES):
        g = cases.load(name)
        for argv, out in zip(g["argv"], g["stdout"]):
            assert out == b"" or out.endswith(b"\n")
            for js in _handle(out):
                _check(js, argv)
                assert js["version"] == "oracle"
                seen[js["type"]] += 1
    assert min(seen.values()) > 100, seen


def test_printer_lines_pass_the_callers_reader():
    from radiosonde_auto_rx_amd.drop import DropPrinter
    for kind in (41, 94):
        p = DropPrinter(json=True, jsn_freq_khz=403240, version="1.2.3")
        text = "".join(p.frame(f) for f in synth.drop_frames(4, kind, corrupt={2: [1]}))
        js = _handle(text.encode())
        assert [j["frame"] for j in js] == [100, 101, 103] and js[0]["freq"] == 403240 and js[0]["version"] == "1.2.3"
        assert js[0]["type"] == "RD%d" % kind and js[0]["id"] == "162345678" and abs(js[0]["lat"] - 47.60821) < 1e-5 and abs(js[0]["alt"] - 9326.5) < 0.01
        for j in js:
            _check(j, ["--jsn_cfq", "403240000"])
