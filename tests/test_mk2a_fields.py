"""The LMS6-1680 / MkIIa printer (include/sonde_mk2a.h, host code): the reference's own -r frames of a capture, turned back into frame bits and
printed here, against the reference's stdout for the same capture — both subframes, wrong CRCs ([NO], no JSON line), CRC bytes ending in 0xCA
(the retry at three lengths), --jsn_cfq, no JSON before the full ID, and frames the reference did not see: one cut before pos_GPSalt + 4 and a
repeated frame number.  Goldens: tools/make_golden_mk2a.py."""
import numpy as np
import pytest

from tests import mk2a_cases as cases
from tools import synth

CA4 = bytes([0xCA] * 4)


def _fb(data: bytes):
    """frame bits of a subframe as the slicer ends them: at CA CA CA CA behind it, or at 1760 bits (the 54 subframe: 174 bytes and two of fill)"""
    return synth.mk2a_bits(bytes(data) + CA4)[:1760]


def _frames(raw_stdout: bytes):
    """the hex lines of a -r output -> frame bits as the slicer hands them over: the bytes in 8N1 and the CA CA CA CA that ended the frame"""
    out = []
    for line in raw_stdout.decode().split("\n"):
        if not line.startswith("24 52 "):
            continue
        hexpart = line.split("  [")[0]
        out.append(_fb(bytes.fromhex(hexpart.replace(" ", ""))))
    return out


def _print(frames, **opts):
    from radiosonde_auto_rx_amd.mk2a import Mk2aPrinter
    opts.setdefault("version", "oracle")
    p = Mk2aPrinter(**opts)
    return ("".join(p.frame(f, 0.97, 1234.0) for f in frames) + "\n").encode("latin-1")


def _opts(argv):
    o = {"json": "--json" in argv, "raw": "-r" in argv, "crc": "--crc" in argv, "vbs": 1 if "-v" in argv else 0, "show_df": "--dc" in argv}
    if "--jsn_cfq" in argv:
        cfq = int(argv[argv.index("--jsn_cfq") + 1])
        fq = float(argv[argv.index("--iq") + 1])
        o["jsn_freq_khz"] = int((cfq + fq * int(argv[argv.index("-") + 1]) + 500) / 1e3)
    return o


@pytest.mark.parametrize("name", ["240k_off0", "240k_noisy", "240k_crcca"])
def test_printer_equals_reference_on_its_own_frames(name):
    g = cases.load(name)
    raw = g["stdout"][g["argv"].index(cases.MK2A + ["-r"])]
    frames = _frames(raw)
    assert len(frames) >= 12
    for argv, ref in zip(g["argv"], g["stdout"]):
        if "-vv" in argv:
            continue                                  # s= / Df= come from the demodulator (tests/test_gpu_mk2a.py)
        assert _print(frames, **_opts(argv)) == ref, argv


def test_goldens_cover_the_frame_kinds():
    raw = cases.load("240k_off0")["stdout"][1].decode()
    assert "24 52 54 " in raw and "24 52 4d " in raw and " (0x614E) [  100]" in raw and " (12345678) [  101]" in raw
    first = raw.index('"type": "LMS"')
    assert raw.index("[  100]") < first and '"frame": 100' not in raw          # no full ID yet: no JSON line
    assert '"freq": 1680000' in cases.load("240k_off0")["stdout"][2].decode()
    noisy = cases.load("240k_noisy")["stdout"][1].decode()
    assert " [NO]" in noisy and noisy.count('"type": "LMS"') < noisy.count("vH:")
    ca = cases.load("240k_crcca")["stdout"][0].decode()
    assert sum(1 for l in ca.split("\n") if l.startswith("24 52 54") and l.endswith("ca  [OK]")) == 2


def test_crc_ending_in_fill_is_found_at_the_longer_lengths():
    f, _ = synth.mk2a_subframes(3, crc_ca=True)
    assert f[-1] == 0xCA and synth.mk2a_crc16(f[:-2]) == (f[-2] << 8 | f[-1])
    out = _print([_fb(f)], raw=True, crc=True).decode()
    assert out.split("\n")[0] == " ".join("%02x" % b for b in f) + "  [OK]"
    # both CRC bytes 0xCA cannot be told from fill by the first two tries either: a frame whose CRC is 0xCACA
    body = bytearray(f[:-2])
    v = 0
    while synth.mk2a_crc16(body) != 0xCACA:
        v += 1
        body[100], body[101], body[102] = v & 0x7F, (v >> 7) & 0x7F, (v >> 14) & 0x7F
    out = _print([_fb(bytes(body) + b"\xCA\xCA")], raw=True, crc=True).decode()
    assert out.split("\n")[0] == " ".join("%02x" % b for b in bytes(body) + b"\xCA\xCA") + "  [OK]"


def test_frame_cut_before_the_altitude_prints_no_telemetry():
    f, m = synth.mk2a_subframes(4)
    bits = synth.mk2a_bits(f)
    short = _print([bits[:300]], raw=True, crc=True, json=True).decode()       # 30 bytes: len / 10 > pos_GPSalt + 4 = 30 fails
    assert short == " ".join("%02x" % b for b in f[:30]) + "  [NO]\n\n"
    assert "vH:" in _print([bits[:310]], raw=True, crc=True, json=True).decode()


def test_repeated_frame_number_prints_one_json_line():
    f, m = synth.mk2a_subframes(7)
    frames = [_fb(x) for x in (m, f, f)]
    out = _print(frames, json=True).decode()
    assert out.count("[  107]") == 2 and out.count('"frame": 107') == 1 and '"id": "LMS6-12345678"' in out


def test_crc16_known_answer():
    from radiosonde_auto_rx_amd.mk2a import crc16
    assert crc16(b"123456789") == synth.mk2a_crc16(b"123456789") == 0x31C3        # CRC-16/XMODEM check value
    assert crc16(b"") == 0


def test_printer_rejects_bad_arguments():
    from radiosonde_auto_rx_amd.engine import SondeError
    from radiosonde_auto_rx_amd.mk2a import Mk2aPrinter
    with pytest.raises(SondeError):
        Mk2aPrinter().frame(np.zeros(1761, np.uint8))
    with pytest.raises(SondeError):
        Mk2aPrinter().frame(np.zeros(19, np.uint8))
