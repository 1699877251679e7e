"""iMet-4 / iMet-1-RS on the GPU (k_imet4_afsk behind include/sonde_imet4.h): host/bin/imet4iq stdout byte-identical to the reference's
imet4iq on the same captures (goldens of tools/make_golden_imet4.py: the auto_rx IMET form at +1.5 / -2.6 kHz, --imet1 at 96 kHz, an
off-centre carrier, 8-bit IQ, a noisy capture with wrong CRCs, -r / --rawbits, a stream cut inside a frame, 2.4 Msps (decM 50), FM-audio WAV
at 48 and 96 kHz with and without --dc / --lpFM); a 48-channel batch through the C ABI; three chunkings of one stream; the one-stream receiver
(wideband.py) on a 2.4 Msps capture with an iMet-4 and an RS41."""
import os
import subprocess

import numpy as np
import pytest

from tests import imet4_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "host", "bin", "imet4iq")
ENV = dict(os.environ, SONDE_JSN_VERSION="oracle")


def _cli(argv, data=None, wav=None, tmp_path=None):
    if wav is not None:
        p = str(tmp_path / "in.wav")
        with open(p, "wb") as f:
            f.write(wav)
        argv = [p if a == "{wav}" else a for a in argv]
    r = subprocess.run([BIN] + argv, input=data, capture_output=True, timeout=120, env=ENV)
    assert r.returncode == 0, (argv, r.stderr[-400:])
    return r.stdout


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_cli_equals_reference(name, tmp_path):
    g = cases.load(name)
    data, wav = cases.capture(cases.CASES[name])
    for argv, ref in zip(g["argv"], g["stdout"]):
        assert argv in cases.CASES[name]["argv"]
        out = _cli(argv, data, wav, tmp_path)
        assert out == ref, (name, argv, out[-600:], ref[-600:])


def test_cli_refuses_what_is_not_built():
    for argv in (["--decFM", "--iq", "0.0", "-", "48000", "16"], ["--iq", "0.0", "-", "48000", "32"], ["--noLUT", "--iq", "0.0", "-", "48000", "16"]):
        r = subprocess.run([BIN] + argv, input=b"\0" * 4000, capture_output=True, timeout=60, env=ENV)
        assert r.returncode == 255 and r.stdout == b"", argv


def _engine_text(eng, printers, n_ch, x, chunk):
    """x: (n_ch, 2 n) int16 -> per channel the printed text, processing `chunk` samples per call"""
    text = [""] * n_ch
    n = x.shape[1] // 2
    for p in range(0, n, chunk):
        eng.process_host(np.ascontiguousarray(x[:, 2 * p:2 * min(n, p + chunk)]))
        for f in eng.fetch_frames():
            text[f["channel"]] += printers[f["channel"]].frame(f["bits"])
    return [t + "\n" for t in text]


def test_batch_48_channels_equal_single_channel_and_reference():
    from radiosonde_auto_rx_amd.imet4 import Imet4Engine, Imet4Printer
    names = ["48k_off1500", "48k_offm2600", "48k_noisy", "48k_cut"]            # four 16-bit streams at fq 0, twelve channels each
    n = int(4.62 * 48000)
    xs, refs = [], []
    for k in range(48):
        nm = names[k % 4]
        data, _ = cases.capture(cases.CASES[nm])
        xs.append(np.frombuffer(data, "<i2")[:2 * n])
        g = cases.load(nm)
        refs.append(g["stdout"][g["argv"].index(cases.IMET + ["--json"])].decode("latin-1"))
    x = np.stack(xs)
    eng = Imet4Engine([0.0] * 48, 48000, max_chunk=12000)
    out = _engine_text(eng, [Imet4Printer(json=True, version="oracle") for _ in range(48)], 48, x, 12000)
    eng.close()
    for k in range(4):
        one = _cli(cases.IMET + ["--json"], x[k].astype("<i2").tobytes()).decode("latin-1")
        assert one.count("\n\n") >= 3
        assert ref_prefix(one, refs[k])
        for c in range(k, 48, 4):
            assert out[c] == one, c


def ref_prefix(text, ref):
    """the frames of a cut stream are the first frames of the whole one (the chain is causal)"""
    return ref.startswith(text[:-1])


def test_chunkings_give_identical_lines():
    from radiosonde_auto_rx_amd.imet4 import Imet4Engine, Imet4Printer
    data, _ = cases.capture(cases.CASES["48k_off1500"])
    x = np.frombuffer(data, "<i2")[None, :]
    res = []
    for chunk in (4800, 48000, 12345):
        eng = Imet4Engine([0.0], 48000, max_chunk=chunk)
        res.append(_engine_text(eng, [Imet4Printer(json=True, version="oracle")], 1, x, chunk)[0])
        eng.close()
    g = cases.load("48k_off1500")
    assert res[0] == res[1] == res[2] == g["stdout"][0].decode("latin-1")


def test_wideband_receiver_decodes_imet4_like_imet4iq():
    """wideband.py on 2.4 Msps with an iMet-4 at +300 kHz and an RS41 at -400 kHz, told nothing: the scanner reports IMET4, an iMet channel
    starts at 48 kHz IF, and its JSON objects are the reference imet4iq's on that capture from the first frame after the start on."""
    import json
    from radiosonde_auto_rx_amd.wideband import WidebandReceiver
    g = cases.load("wide_2400k")
    data, _ = cases.capture(cases.CASES["wide_2400k"])
    ref = [json.loads(l) for l in g["stdout"][0].decode().split("\n") if l.startswith("{")]
    rx = WidebandReceiver(2_400_000, cfreq_hz=403_000_000, raster_hz=10_000, version="oracle")
    out = rx.push(np.frombuffer(data, np.int16), finish=True)
    types = sorted(s["type"] for s in rx.sondes)
    rs41_frames = sum(s["frames"] for s in rx.sondes if s["type"] == "RS41")
    rx.close()
    assert types == ["IMET4", "RS41"], rx.log
    imet = [j for j in out if j["type"] == "IMET"]
    assert len(imet) >= 3 and len(ref) >= 6, (len(imet), len(ref))
    assert imet == ref[len(ref) - len(imet):]
    assert rs41_frames >= 3                  # the RS41 next to it is decoded too (no JSON: its frames carry no calibration data)
