"""Weathex WxR-301D on the GPU (the iq_dec front end + k_wxr_slice behind include/sonde_wxr.h).  Everything is compared as text, byte for byte,
with the reference's weathex301d on the same captures (goldens of tools/make_golden_wxr.py):
 - `host/bin/iq_dec <auto_rx's options> | host/bin/weathex301d <argv>` as two processes, stdout and the decoder's stderr;
 - the engine's IQ form (front end and slicer in one engine, the FM samples never leave the device) through a small driver;
 - WAV input of 8 / 16 / 32 bits and 2 channels straight into weathex301d: no float front end in between, the slicer alone;
 - a 48-channel batch through the C ABI, four chunkings of one stream with and without -b;
 - the one-stream receiver (wideband.py) told a WXR301 / WXRPN9 channel on a 2.4 Msps capture;
 - `host/bin/fsk_demod | host/bin/weathex301d --softin -i`;
 - what the reference answers with exit 255."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import wxr_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "host", "bin", "weathex301d")
IQDEC = os.path.join(ROOT, "host", "bin", "iq_dec")
FSK = os.path.join(ROOT, "host", "bin", "fsk_demod")
ENV = dict(os.environ, SONDE_JSN_VERSION="oracle")

IQ = sorted(n for n, c in cases.CASES.items() if c["front"] is not None and c["gen"].get("form") != "soft")
WAV = sorted(n for n, c in cases.CASES.items() if c["front"] is None)
SOFT = sorted(n for n, c in cases.CASES.items() if c["gen"].get("form") == "soft")


def _pipe(front, argv, data):
    """two processes, as auto_rx runs them; returns the decoder's (stdout, stderr)"""
    if front is None:
        r = subprocess.run([BIN] + argv, input=data, capture_output=True, timeout=180, env=ENV)
    else:
        p1 = subprocess.Popen(front, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=ENV)
        p2 = subprocess.Popen([BIN] + argv, stdin=p1.stdout, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=ENV)
        p1.stdout.close()
        p1.stdin.write(data)
        p1.stdin.close()
        out, err = p2.communicate(timeout=180)
        e1 = p1.stderr.read()
        assert p1.wait(timeout=60) == 0, e1[-400:]
        r = subprocess.CompletedProcess(argv, p2.returncode, out, err)
    assert r.returncode == 0, (argv, r.stderr[-400:])
    return r.stdout, r.stderr


def _printer(argv):
    from radiosonde_auto_rx_amd.wxr import WxrPrinter
    cfq = int(argv[argv.index("--jsn_cfq") + 1]) if "--jsn_cfq" in argv else -1
    return WxrPrinter(raw=2 if "-R" in argv else 1 if "-r" in argv else 0, vbs="-v" in argv, json="--json" in argv, pn9="--pn9" in argv,
                      jsn_freq_khz=(cfq + 500) // 1000 if cfq >= 300000000 else 0, version="oracle")


def _text(pr, f, argv, rate):
    """what weathex301d writes for one frame record"""
    t = "<%8.3f> " % (f["sample"] / rate) if "-t" in argv else ""
    return t + (pr.frame(f["bits"]) if f["complete"] or "-b" in argv else "")


def _engine_text(eng, printers, argv, n_ch, x, chunk, per=2):
    """x: (n_ch, per * n) samples -> per channel the text of the command line `argv`, processing `chunk` samples per call"""
    text = [""] * n_ch
    n = x.shape[1] // per
    step = max(eng.dec_m, chunk - chunk % eng.dec_m)
    n -= n % eng.dec_m
    for p in list(range(0, n, step)) + [None]:
        if p is None:
            eng.finish()
        else:
            eng.process_host(np.ascontiguousarray(x[:, per * p:per * min(n, p + step)]))
        for f in eng.fetch_frames():
            text[f["channel"]] += _text(printers[f["channel"]], f, argv, float(eng.if_rate))
    return [t + "\n" for t in text]


def _iq_engine(argv, sr, bits, fqs, chunk):
    from radiosonde_auto_rx_amd.wxr import WxrEngine
    return WxrEngine(fqs, sr, bits=bits, pn9="--pn9" in argv, invert="-i" in argv, opt_b="-b" in argv, if_bw_khz=64, max_chunk=chunk)


@pytest.mark.parametrize("name", IQ)
def test_iq_pipeline_and_engine_equal_reference(name):
    case, g = cases.CASES[name], cases.load(name)
    data = cases.capture(case)
    assert g["argv"] == case["argv"] and g["front"] == case["front"]
    sr, bits, fq = int(case["front"][-2]), int(case["front"][-1]), float(case["front"][case["front"].index("--iq") + 1])
    x = np.frombuffer(data, "<i2" if bits == 16 else np.uint8)[None, :]
    for argv, ref, ref_err in zip(g["argv"], g["stdout"], g["stderr"]):
        out, err = _pipe([IQDEC] + case["front"], argv, data)
        print(name, argv, "lines", out.count(b"\n"), ref.count(b"\n"), "equal", out == ref)
        assert out == ref, (name, argv, out[-900:], ref[-900:])
        assert err == ref_err, (name, argv, err, ref_err)
        eng = _iq_engine(argv, sr, bits, [fq], sr // 4)
        one = _engine_text(eng, [_printer(argv)], argv, 1, x, sr // 4)[0]
        eng.close()
        assert one.encode("latin-1") == ref, (name, argv, "engine", one[-900:], ref[-900:])


@pytest.mark.parametrize("name", WAV)
def test_wav_input_equals_reference(name):
    case, g = cases.CASES[name], cases.load(name)
    data = cases.capture(case)
    for argv, ref, ref_err in zip(g["argv"], g["stdout"], g["stderr"]):
        out, err = _pipe(None, argv, data)
        print(name, argv, "lines", out.count(b"\n"), ref.count(b"\n"), "equal", out == ref)
        assert out == ref, (name, argv, out[-900:], ref[-900:])
        assert err == ref_err, (name, argv, err, ref_err)


def test_wav_file_argument(tmp_path):
    g = cases.load("wav16")
    p = str(tmp_path / "fm.wav")
    with open(p, "wb") as f:
        f.write(cases.capture(cases.CASES["wav16"]))
    r = subprocess.run([BIN] + g["argv"][0] + [p], capture_output=True, timeout=180, env=ENV)
    assert r.returncode == 0 and r.stdout == g["stdout"][0]


@pytest.mark.parametrize("name", SOFT)
def test_modem_pipeline_equals_reference(name):
    """fsk_demod with auto_rx's WXR options in front of --softin: 2-FSK at 20 samples per symbol, as the modem takes every other sonde"""
    case, g = cases.CASES[name], cases.load(name)
    data = cases.capture(case)
    for argv, ref in zip(g["argv"], g["stdout"]):
        out, _ = _pipe([FSK] + case["front"], argv, data)
        print(name, argv, "lines", out.count(b"\n"), ref.count(b"\n"), "equal", out == ref)
        assert out == ref, (name, argv, out[-900:], ref[-900:])


def test_cli_exit_codes(tmp_path):
    """what the reference answers with `return -1`, and -h"""
    from tools import synth
    wav24 = synth.wav_bytes(np.zeros(4000, np.int16), 96000)
    wav24 = wav24[:34] + (24).to_bytes(2, "little") + wav24[36:]
    for argv, data in ((["-b", "--json"], b"\0" * 4000), (["-b"], wav24), ([str(tmp_path / "missing.wav")], b""), (["--json", "--jsn_cfq"], b"")):
        r = subprocess.run([BIN] + argv, input=data, capture_output=True, timeout=60, env=ENV)
        assert r.returncode == 255 and r.stdout == b"", argv
    r = subprocess.run([BIN, "-h"], input=b"", capture_output=True, timeout=60, env=ENV)
    assert r.returncode == 0 and r.stdout == b"" and b"[options] audio.wav" in r.stderr


def test_batch_48_channels_equal_single_channel_and_reference():
    names = cases.BATCH                                                         # the 96 kHz 16-bit captures, round-robin
    xs = [np.frombuffer(cases.capture(cases.CASES[nm]), "<i2") for nm in names]
    for argv in (["-b", "--json"], ["-r", "-t"]):
        for pn9 in (False, True):
            av = argv + (["--pn9"] if pn9 else [])
            idx = [k for k, nm in enumerate(names) if bool(cases.CASES[nm]["gen"].get("pn9")) == pn9]
            n = max(len(xs[i]) for i in idx)                                   # zero IQ behind the shorter ones: FM 0, one long run, no bits
            x = np.stack([np.concatenate([xs[i], np.zeros(n - len(xs[i]), np.int16)]) for i in (idx[c % len(idx)] for c in range(48))])
            eng = _iq_engine(av, 96000, 16, [0.0] * 48, 24000)
            out = _engine_text(eng, [_printer(av) for _ in range(48)], av, 48, x, 24000)
            eng.close()
            for k, i in enumerate(idx):
                nm = names[i]
                one, _ = _pipe([IQDEC] + cases.iq_dec_args(), av, x[k].astype("<i2").tobytes())
                g = cases.load(nm)
                if av in g["argv"] and len(xs[i]) == n:
                    assert one == g["stdout"][g["argv"].index(av)], (nm, av)
                for c in range(k, 48, len(idx)):
                    assert out[c].encode("latin-1") == one, (c, nm, av)
    g = cases.load("clean")
    assert g["stdout"][0].count(b"[OK]") == 8


@pytest.mark.parametrize("argv", [["-b", "-r", "-t"], ["-r", "-t"]])
def test_chunkings_give_identical_frames(argv):
    x = np.frombuffer(cases.capture(cases.CASES["cut"]), "<i2")[None, :]
    res = []
    for chunk in (24000, 96000, 12345, 3001):                                   # 3001 < 552 * 20 samples of a frame, 12345 odd
        eng = _iq_engine(argv, 96000, 16, [0.0], chunk)
        res.append(_engine_text(eng, [_printer(argv)], argv, 1, x, chunk)[0])
        eng.close()
    one, _ = _pipe([IQDEC] + cases.iq_dec_args(), argv, x[0].astype("<i2").tobytes())
    assert res[0].encode("latin-1") == one and one.count(b"[OK]") >= 10
    for r in res[1:]:
        assert r == res[0]


def test_fm_form_chunkings_on_float_samples():
    """the slicer alone (FM form; float32, and the 16-bit capture with runs of 0 bits) in pieces down to 7 samples a call against the
    one-call CLI run on the same WAV"""
    from radiosonde_auto_rx_amd.wxr import WxrEngine
    for name, dt, chunks in (("wav32", "<f4", (24000, 4099, 7)), ("zero_runs", "<i2", (4099, 7))):
        data = cases.capture(cases.CASES[name])
        g = cases.load(name)
        s = np.frombuffer(data[44:], dt)[None, :]
        bits = s.dtype.itemsize * 8
        for argv, ref in zip(g["argv"], g["stdout"]):
            for chunk in chunks:
                if chunk == 7:
                    s1 = s[:, :40000]
                    eng = WxrEngine.fm(1, 96000, bits=bits, opt_b="-b" in argv, max_chunk=24000)
                    want = _engine_text(eng, [_printer(argv)], argv, 1, s1, 24000, per=1)[0]
                    eng.close()
                else:
                    s1, want = s, ref.decode("latin-1")
                eng = WxrEngine.fm(1, 96000, bits=bits, opt_b="-b" in argv, max_chunk=chunk)
                got = _engine_text(eng, [_printer(argv)], argv, 1, s1, chunk, per=1)[0]
                eng.close()
                assert got == want, (name, argv, chunk)


@pytest.mark.parametrize("typ,name", [("WXR301", "wide_2400k"), ("WXRPN9", "wide_2400k_pn9")])
def test_wideband_receiver_decodes_a_told_channel(typ, name):
    """wideband.py on 2.4 Msps with a WxR-301D at +240 kHz, the channel announced at its fq (the scanner's 48 kHz IF does not see a 64 kHz
    wide signal reliably): the receiver's JSON objects are those of `iq_dec --iq 0.1 ... | weathex301d -b --json --jsn_cfq ...`."""
    from radiosonde_auto_rx_amd.wideband import WidebandReceiver
    g = cases.load(name)
    data = cases.capture(cases.CASES[name])
    ref = [json.loads(l) for l in g["stdout"][0].decode().split("\n") if l.startswith("{")]
    assert len(ref) >= 5 and ref[0]["freq"] == 403240
    rx = WidebandReceiver(2_400_000, cfreq_hz=403_000_000, raster_hz=100_000, version="oracle")
    rx.add_channel(typ, 0.1)
    out = rx.push(np.frombuffer(data, np.int16), finish=True)
    types = [s["type"] for s in rx.sondes if s["type"] == typ]
    rx.close()
    assert types == [typ], rx.log
    assert [j for j in out if j["type"] == "WXR301"] == ref
