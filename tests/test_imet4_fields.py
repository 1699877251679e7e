"""The iMet-4 / iMet-1-RS printer (include/sonde_imet4.h, host code): the reference's own --rawbits frames of a capture, printed here, against
the reference's stdout for the same capture with --json, --jsn_cfq, -r and no option — eGPS (its CRC read at the GPS offset), ozone and
generic XDATA ("aux"), a wrong CRC ([NO], no JSON line).  Goldens: tools/make_golden_imet4.py."""
import numpy as np
import pytest

from tests import imet4_cases as cases


def _frames(rawbits_stdout: bytes):
    """--rawbits lines -> 1000-bit frames (the line ends where the byte frame ends; ones behind it end it the same way)"""
    out = []
    for line in rawbits_stdout.decode().split("\n"):
        s = line.replace(" ", "")
        if not s:
            continue
        b = np.ones(1000, np.uint8)
        b[:len(s)] = np.frombuffer(s.encode(), np.uint8) - ord("0")
        out.append(b)
    return out


def _print(frames, **opts):
    from radiosonde_auto_rx_amd.imet4 import Imet4Printer
    opts.setdefault("version", "oracle")
    p = Imet4Printer(**opts)
    return ("".join(p.frame(f) for f in frames) + "\n").encode("latin-1")


def _opts(argv):
    o = {"json": "--json" in argv, "raw": "-r" in argv, "rawbits": "--rawbits" in argv}
    if "--jsn_cfq" in argv:
        cfq = int(argv[argv.index("--jsn_cfq") + 1])
        fq = float(argv[argv.index("--iq") + 1]) if "--iq" in argv else 0.0
        o["jsn_freq_khz"] = int((cfq + fq * int(argv[argv.index("-") + 1]) + 500) / 1e3)
    return o


def test_printer_equals_reference_on_its_own_frames():
    g = cases.load("48k_off1500")
    frames = _frames(g["stdout"][g["argv"].index(cases.IMET + ["--rawbits"])])
    assert len(frames) == 7
    for argv, ref in zip(g["argv"], g["stdout"]):
        assert _print(frames, **_opts(argv)) == ref, argv


def test_golden_covers_the_packet_kinds():
    ref = cases.load("48k_off1500")["stdout"][0]
    assert b"vH:" in ref and b"[NO]" in ref and b"Icell:" in ref and b"(N=0x04)" in ref and b'"aux": "0107007B09605A70#19023344"' in ref
    assert ref.count(b'"type": "IMET"') == 5
    assert b'"freq": 402500' in cases.load("48k_off1500")["stdout"][1]


def test_crc16_known_answer():
    from radiosonde_auto_rx_amd.imet4 import crc16
    from tools.synth import imet4_crc16
    assert crc16(b"123456789") == imet4_crc16(b"123456789") == 0xE5CC      # CRC-16/AUG-CCITT check value
    assert crc16(b"") == 0x1D0F
    pkt = bytes.fromhex("0102") + bytes(range(14))
    assert crc16(pkt) == imet4_crc16(pkt)


def test_printer_rejects_bad_arguments():
    from radiosonde_auto_rx_amd.engine import SondeError
    from radiosonde_auto_rx_amd.imet4 import Imet4Printer
    with pytest.raises(SondeError):
        Imet4Printer().frame(np.zeros(1300, np.uint8))
