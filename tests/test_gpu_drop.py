"""RD94 / RD41 dropsondes on the GPU (the iq_dec front end + k_drop_slice behind include/sonde_drop.h).  Everything is compared as text, byte
for byte, with the reference's rd94rd41drop on the same captures (goldens of tools/make_golden_drop.py):
 - `host/bin/iq_dec --FM --lpFM --wav --bo 16 ... | host/bin/rd94rd41drop <argv>` as two processes, stdout and the decoder's stderr;
 - the engine's IQ form (front end and slicer in one engine, the FM samples never leave the device) through the Python mirror;
 - WAV input of 8 / 16 bits and 2 channels straight into rd94rd41drop: no float front end in between, the slicer alone;
 - the device's check masks of every fetched frame against the host code on the device's bytes; the device's bytes against the host
   framer on the same raw bits on a synthetic stream (elsewhere the bytes are covered through the printed text);
 - a 48-channel batch through the C ABI, several chunkings of one stream with and without -b, the FM form down to 7 samples a call;
 - `host/bin/fsk_demod | host/bin/rd94rd41drop --json --softinv`, --rawhex, and what the reference answers with exit 255."""
import os
import subprocess

import numpy as np
import pytest

from tests import drop_cases as cases
from tests.test_drop_fields import _printer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "host", "bin", "rd94rd41drop")
IQDEC = os.path.join(ROOT, "host", "bin", "iq_dec")
FSK = os.path.join(ROOT, "host", "bin", "fsk_demod")
ENV = dict(os.environ, SONDE_JSN_VERSION="oracle")

IQ = sorted(n for n, c in cases.CASES.items() if c["front"] is not None and c["gen"].get("form") != "soft")
WAV = sorted(n for n, c in cases.CASES.items() if c["front"] is None)
SOFT = sorted(n for n, c in cases.CASES.items() if c["gen"].get("form") == "soft")


def _pipe(front, argv, data, rc=0):
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
    assert r.returncode == rc, (argv, r.returncode, r.stderr[-400:])
    return r.stdout, r.stderr


def _check_record(f):
    """the device's frame completion against the host's: check masks from the bytes"""
    from radiosonde_auto_rx_amd import drop
    assert (f["err94"], f["err41"]) == drop.errs(f["bytes"]), f
    assert f["nraw"] == 2400 if f["complete"] else 40 <= f["nraw"] < 2400


def _engine_text(eng, printers, n_ch, x, chunk, per=2, records=None):
    """x: (n_ch, per * n) samples -> per channel the decoder's text, processing `chunk` samples per call"""
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
            _check_record(f)
            if records is not None:
                records.append(f)
            text[f["channel"]] += printers[f["channel"]].frame(f["bytes"])
    return text


def _br(argv):
    return float(argv[argv.index("--br") + 1]) if "--br" in argv else 0.0


def _iq_engine(argv, sr, bits, fqs, chunk):
    from radiosonde_auto_rx_amd.drop import DropEngine
    return DropEngine(fqs, sr, bits=bits, invert="-i" in argv, opt_b="-b" in argv, baud=_br(argv), max_chunk=chunk)


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
        one = _engine_text(eng, [_printer(argv)], 1, x, sr // 4)[0]
        eng.close()
        assert one.encode() == ref, (name, argv, "engine", one[-900:], ref[-900:])


@pytest.mark.parametrize("name", WAV)
def test_wav_and_rawhex_input_equal_reference(name):
    case, g = cases.CASES[name], cases.load(name)
    data = cases.capture(case)
    for argv, ref, ref_err in zip(g["argv"], g["stdout"], g["stderr"]):
        out, err = _pipe(None, argv, data, rc=case.get("rc", 0))
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
    """auto_rx's production pipe: fsk_demod --cs16 -b -20000 -u 20000 -s --stats=N 2 48000 4800 - - | rd94rd41drop --json --softinv"""
    case, g = cases.CASES[name], cases.load(name)
    data = cases.capture(case)
    for argv, ref in zip(g["argv"], g["stdout"]):
        out, _ = _pipe([FSK] + case["front"], argv, data)
        print(name, argv, "lines", out.count(b"\n"), ref.count(b"\n"), "equal", out == ref)
        assert out == ref, (name, argv, out[-900:], ref[-900:])


def test_cli_exit_codes(tmp_path):
    """what the reference answers with `return -1`, and -h"""
    from tools import synth
    wav32 = cases.capture(cases.CASES["wav32"])
    for argv, data in ((["-b", "--json"], b"\0" * 4000), (["-b"], wav32), ([str(tmp_path / "missing.wav")], b""), (["--json", "--jsn_cfq"], b""),
                       (["-b", "--br"], synth.wav_bytes(np.zeros(4000, np.int16), 48000))):
        r = subprocess.run([BIN] + argv, input=data, capture_output=True, timeout=60, env=ENV)
        assert r.returncode == 255 and r.stdout == b"", argv
    r = subprocess.run([BIN, "-h"], input=b"", capture_output=True, timeout=60, env=ENV)
    assert r.returncode == 0 and r.stdout == b"" and b"[options] <file>" in r.stderr


def test_batch_52_channels_equal_reference():
    names = cases.BATCH                                                         # the 48 kHz 16-bit captures, round-robin
    xs = [np.frombuffer(cases.capture(cases.CASES[nm]), "<i2") for nm in names]
    n = max(len(v) for v in xs)                                                 # zero IQ behind the shorter ones: FM 0, one long run, no bits
    n_ch = 4 * len(names)
    x = np.stack([np.concatenate([xs[c % len(xs)], np.zeros(n - len(xs[c % len(xs)]), np.int16)]) for c in range(n_ch)])
    assert n_ch >= 48
    for argv in (["-b", "--json"], ["-r"]):
        eng = _iq_engine(argv, 48000, 16, [0.0] * n_ch, 12000)
        recs = []
        out = _engine_text(eng, [_printer(argv) for _ in range(n_ch)], n_ch, x, 12000, records=recs)
        eng.close()
        assert len(recs) > 4 * 40
        for k, nm in enumerate(names):
            g = cases.load(nm)
            one, _ = _pipe([IQDEC] + cases.iq_dec_args(), argv, x[k].astype("<i2").tobytes())
            if argv in g["argv"] and len(xs[k]) == n:
                assert one == g["stdout"][g["argv"].index(argv)], (nm, argv)
            for c in range(k, n_ch, len(names)):
                assert out[c].encode() == one, (c, nm, argv)


@pytest.mark.parametrize("argv", [["-b", "-r"], ["-r"], ["-b", "--br", "4798.8", "-r"]])
def test_chunkings_give_identical_frames(argv):
    x = np.frombuffer(cases.capture(cases.CASES["cut41"]), "<i2")[None, :]
    res = []
    for chunk in (12000, 48000, 12345, 3001):                                   # a -b frame is 23 600 samples: every chunking cuts it
        eng = _iq_engine(argv, 48000, 16, [0.0], chunk)
        res.append(_engine_text(eng, [_printer(argv)], 1, x, chunk)[0])
        eng.close()
    one, _ = _pipe([IQDEC] + cases.iq_dec_args(), argv, x[0].astype("<i2").tobytes())
    assert res[0].encode() == one and one.count(b"\n") >= 3
    g = cases.load("cut41")
    if argv in g["argv"]:
        assert one == g["stdout"][g["argv"].index(argv)]
    for r in res[1:]:
        assert r == res[0]


def test_fm_form_chunkings_on_integer_samples():
    """the slicer alone (FM form, 16 and 8 bits) in pieces down to 7 samples a call against the reference's text on the same WAV"""
    from radiosonde_auto_rx_amd.drop import DropEngine
    for name, dt, chunks in (("wav16", "<i2", (12000, 4099, 7)), ("wav8", np.uint8, (12000, 4099, 7)), ("zero_runs", "<i2", (4099, 7))):
        data = cases.capture(cases.CASES[name])
        g = cases.load(name)
        s = np.frombuffer(data[44:], dt)[None, :]
        for argv, ref in zip(g["argv"], g["stdout"]):
            for chunk in chunks:
                s1, want = s, ref.decode()
                if chunk == 7:                                                   # a quarter of the stream is enough at 7 samples a call
                    s1 = s[:, :60000]
                    eng = DropEngine.fm(1, 48000, bits=s.dtype.itemsize * 8, opt_b="-b" in argv, max_chunk=12000)
                    want = _engine_text(eng, [_printer(argv)], 1, s1, 12000, per=1)[0]
                    eng.close()
                    assert want != ""
                eng = DropEngine.fm(1, 48000, bits=s.dtype.itemsize * 8, opt_b="-b" in argv, max_chunk=chunk)
                got = _engine_text(eng, [_printer(argv)], 1, s1, chunk, per=1)[0]
                eng.close()
                assert got == want, (name, argv, chunk)


def test_device_bytes_equal_host_framer_on_the_same_raw_bits():
    """FM form on a synthetic square wave made from known raw bits: the device's bytes are the generator's frames, and equal what the host
    code makes of the same raw bits (sonde_drop_frame_from_rawbits); a frame cut by the end of the input is completed with '0' bits"""
    from radiosonde_auto_rx_amd import drop
    from tools import synth
    frames = synth.drop_frames(3, 94, corrupt={1: [2]})
    raw = synth.drop_rawbits([b"\x1A\xCF"] + frames)
    s = np.repeat(np.where(raw > 0, 9000, -9000).astype(np.int16), 10)[None, :-8000]
    for opt_b in (True, False):
        eng = drop.DropEngine.fm(1, 48000, bits=16, opt_b=opt_b, max_chunk=5000)
        recs = []
        _engine_text(eng, [_printer(["-r"])], 1, s, 5000, per=1, records=recs)
        eng.close()
        assert [r["bytes"] for r in recs[:2]] == frames[:2] and [r["err94"] for r in recs[:2]] == [0, 4]
        for r, k in zip(recs, range(3)):
            host = drop.frame_from_rawbits(raw[40 + 2400 * k:40 + 2400 * (k + 1)].astype(np.uint8), r["nraw"])
            assert (host["bytes"], host["err94"], host["err41"]) == (r["bytes"], r["err94"], r["err41"])
        assert len(recs) == (3 if opt_b else 2)
        if opt_b:
            assert not recs[2]["complete"] and recs[2]["nraw"] == 2400 - 800 and recs[2]["bytes"][:79] == frames[2][:79]


WIDE = [("wide41_2400k", "RD41", False), ("wide94_2400k", "RD94", True)]


def _golden_json(name):
    import json
    g = cases.load(name)
    ref = [json.loads(l) for l in g["stdout"][0].decode().split("\n") if l.startswith("{")]
    assert len(ref) == cases.N_FRAMES and ref[0]["freq"] == 403240
    return ref


@pytest.mark.parametrize("name,typ,inv", WIDE)
def test_wideband_receiver_decodes_a_told_channel(name, typ, inv):
    """wideband.py on 2.4 Msps with a dropsonde at +240 kHz, the channel announced at its fq: the receiver's JSON objects are those of
    `iq_dec --iq 0.1 ... --bo 16 | rd94rd41drop -b --json [-i] --jsn_cfq ...`, all of them"""
    from radiosonde_auto_rx_amd.wideband import WidebandReceiver
    ref = _golden_json(name)
    data = cases.capture(cases.CASES[name])
    rx = WidebandReceiver(2_400_000, cfreq_hz=403_000_000, raster_hz=100_000, version="oracle")
    rx.add_channel("RD94RD41", 0.1, invert=inv)
    out = rx.push(np.frombuffer(data, np.int16), finish=True)
    types = [s["type"] for s in rx.sondes if abs(s["fq"] - 0.1) < 1e-6]
    rx.close()
    assert types == [typ], rx.log
    assert [j for j in out if j["type"] == typ] == ref


@pytest.mark.parametrize("name,typ,inv", WIDE)
def test_wideband_receiver_finds_the_dropsonde_itself(name, typ, inv):
    """left to its scanner: one `detected` event for the frequency (RD94RD41, a negative score starting the decoder with -i), the sonde ends
    up typed by its frames, and the JSON objects are a suffix of the golden's.  Missing at the front may be the frames whose header lies
    before the end of the chunk in which the detection was logged, and no more: frame i's header starts lead_s + 40 / 4800 + 0.5 i seconds
    into the capture (the two sync bytes in front, two frames a second)."""
    from radiosonde_auto_rx_amd.wideband import WidebandReceiver
    ref = _golden_json(name)
    x = np.frombuffer(cases.capture(cases.CASES[name]), np.int16)
    sr = 2_400_000
    rx = WidebandReceiver(sr, cfreq_hz=403_000_000, raster_hz=120_000, version="oracle")      # +240 kHz is a raster point
    out, t_det = [], None
    for s0 in range(0, len(x) // 2, rx.chunk):
        last = s0 + rx.chunk >= len(x) // 2
        out += rx.push(x[2 * s0:2 * (s0 + rx.chunk)], finish=last)
        if t_det is None and any(e["event"] == "detected" for e in rx.log):
            t_det = (s0 + rx.chunk) / sr
    det = [e for e in rx.log if e["event"] == "detected" and abs(e["fq"] - 0.1) * sr < 20_000]
    types = [s["type"] for s in rx.sondes if abs(s["fq"] - 0.1) * sr < 20_000]
    log = list(rx.log)
    rx.close()
    assert len(det) == 1 and det[0]["type"] == "RD94RD41" and t_det is not None, log
    assert types == [typ], log
    lead_s = cases.CASES[name]["gen"].get("lead_s", 0.25)
    may_miss = sum(1 for i in range(cases.N_FRAMES) if lead_s + 40 / 4800.0 + 0.5 * i < t_det)
    got = [j for j in out if j["type"] == typ]
    print(name, "detected at the end of", t_det, "s; frames", len(got), "of", len(ref), "may miss", may_miss)
    assert len(got) >= len(ref) - may_miss and len(got) >= 1
    assert got == ref[len(ref) - len(got):]
