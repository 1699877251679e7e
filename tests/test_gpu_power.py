"""The spectrum survey on the GPU (radiosonde_auto_rx_amd/csrc/sonde_power.hip through include/sonde_power.h and power.py): spectra against
the float64 goldens (tools/make_golden_power.py), tone placement, call cuts, stream isolation, auto_rx's peaks from the GPU spectrum, the
rtl_power command line, and the receiver's survey mode.

Tolerances of every spectrum comparison:
  norm-wise  ||P^ - P||_2 <= 8 log2(nfft) 2^-24 ||P||_2   the radix-2 float32 rounding bound with room for window and squaring;
  per bin    |dB^ - dB| <= 0.005                          half a unit of the last digit the log line prints.
The goldens record what numpy's complex64 FFT differs from float64 by; the GPU's own difference is printed beside it."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import power_cases as pc                                   # noqa: E402
from radiosonde_auto_rx_amd import power as pw                        # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "host", "bin", "sonde_power")
DB_TOL = 0.005


def norm_tol(nfft):
    return 8.0 * np.log2(nfft) * 2.0 ** -24


@pytest.fixture(scope="module")
def spectra():
    return np.load(os.path.join(GOLDEN, "power_spectra.npz"))


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "power_fixture.npz"))


def survey_db(x, nfft, window, bits, *, crop=0.0, cuts=None, n_streams=1):
    """-> (dB per stream over the kept bins, segments, freq, step); cuts: complex samples per call (the rest in a last call)"""
    x = np.atleast_2d(x)
    n = x.shape[1] // 2
    ps = pw.PowerSurvey(pc.SR, nfft, center_hz=pc.CENTER_HZ, n_streams=n_streams, bits=bits, window=window, crop=crop, max_chunk=max(n, 1))
    try:
        pos = 0
        for c in list(cuts or []) + [n]:
            c = min(c, n - pos)
            if c > 0:
                ps.process_host(x[:, 2 * pos:2 * (pos + c)])
                pos += c
        out = [ps.fetch(k) for k in range(n_streams)]
        return [o[1] for o in out], [ps.segments(k) for k in range(n_streams)], out[0][0], out[0][2]
    finally:
        ps.close()


def check_against(db_gpu, p_ref, nfft, label, c64=None):
    """db_gpu: all nfft bins, ascending; p_ref: float64 linear power in transform order"""
    d_ref, _ = pc.shift_crop_db(p_ref, 0.0)
    p_gpu = 10.0 ** (db_gpu / 10.0)
    nrm = np.linalg.norm(p_gpu - 10.0 ** (d_ref / 10.0)) / np.linalg.norm(p_ref)
    drop = int(pc.CROP * nfft / 2.0)
    worst = np.max(np.abs(db_gpu - d_ref)[drop:nfft - drop])
    print("%-20s norm-wise %.2e (bound %.2e%s)   worst kept bin %.2e dB (bound %.3f%s)"
          % (label, nrm, norm_tol(nfft), "" if c64 is None else ", complex64 %.2e" % c64[0], worst, DB_TOL, "" if c64 is None else ", complex64 %.2e" % c64[1]))
    assert nrm <= norm_tol(nfft), (label, nrm)
    assert worst <= DB_TOL, (label, worst)


@pytest.mark.parametrize("name", list(pc.SPECTRA))
def test_spectrum_matches_float64_golden(name, spectra):
    nfft, window, bits, n, first = pc.SPECTRA[name]
    db, segs, freq, step = survey_db(pc.spectrum_input(name), nfft, window, bits)
    assert segs == [n // nfft] and len(db[0]) == nfft and step == pc.SR / nfft
    assert freq[0] == pc.CENTER_HZ - pc.SR / 2 and abs(freq[nfft // 2] - pc.CENTER_HZ) < 1e-3
    assert np.isfinite(db[0]).all()
    check_against(db[0], spectra[name + "/power"], nfft, name, (float(spectra[name + "/c64_norm"]), float(spectra[name + "/c64_db"])))


@pytest.mark.parametrize("nfft", [256, 16384])
def test_full_scale_tone_reads_0_db_at_its_bin(nfft):
    """guards the shift, the sign of the exponent and the scaling: +k lands above the centre, -k below, both at 0 dB; every other bin is rounding noise"""
    t = np.arange(2 * nfft)
    for k in (+37, -5, nfft // 2 - 1, -nfft // 2):
        z = np.exp(2j * np.pi * k * t / nfft)
        x = np.empty(4 * nfft, np.float32)
        x[0::2], x[1::2] = z.real, z.imag
        db, segs, freq, step = survey_db(x, nfft, pc.RECT, 32)
        i = nfft // 2 + k
        assert segs == [2] and abs(db[0][i]) <= DB_TOL, (k, db[0][i])
        assert abs(freq[i] - (pc.CENTER_HZ + k * step)) < 1e-3
        assert np.delete(db[0], i).max() < -100.0, (k, np.delete(db[0], i).max())
    x16 = np.empty(2 * nfft, np.int16)                       # the integer formats: full scale is 32767 / 32768 and 127 / 128
    z = np.exp(2j * np.pi * 8 * t[:nfft] / nfft)             # (a period of 32 or 2048 samples: the quantisation error repeats and stays in few bins)
    x16[0::2], x16[1::2] = np.round(32767 * z.real), np.round(32767 * z.imag)
    db, _, _, _ = survey_db(x16, nfft, pc.HANN, 16)
    assert abs(db[0][nfft // 2 + 8]) <= DB_TOL and abs(db[0][nfft // 2 + 9] + 6.02) < 0.01     # Hann: the neighbours at half the amplitude


@pytest.mark.parametrize("nfft,window", [(256, pc.RECT), (4096, pc.HANN)])
def test_call_cuts_do_not_move_segments(nfft, window):
    n = 7 * nfft + 100
    x = pc.capture(1)[2 * 50_000:2 * (50_000 + n)]
    p_ref = pc.ref_power(x, 16, nfft, window)
    whole, segs_w, _, _ = survey_db(x, nfft, window, 16)
    cuts = [1, nfft - 1, 3 * nfft + 5]
    ragged, segs_r, _, _ = survey_db(x, nfft, window, 16, cuts=cuts)
    again, segs_a, _, _ = survey_db(x, nfft, window, 16, cuts=cuts)
    assert segs_w == segs_r == segs_a == [7]
    check_against(whole[0], p_ref, nfft, "one call %d" % nfft)
    check_against(ragged[0], p_ref, nfft, "ragged calls %d" % nfft)
    assert np.max(np.abs(whole[0] - ragged[0])) <= DB_TOL
    assert np.array_equal(ragged[0], again[0])               # the same call pattern: the same bits
    shifted, _, _, _ = survey_db(x[2:], nfft, window, 16)    # (the check can fail: one sample of offset is another spectrum)
    assert np.max(np.abs(shifted[0] - whole[0])) > DB_TOL


def test_streams_are_isolated_and_reset_clears():
    import torch
    nfft, n = 1024, 5 * 1024 + 77
    cap = pc.capture(1)
    a, b = cap[2 * 10_000:2 * (10_000 + n)], cap[2 * 300_000:2 * (300_000 + n)]
    x = np.stack([a, np.zeros(2 * n, np.int16), b])
    db, segs, _, _ = survey_db(x, nfft, pc.RECT, 16, n_streams=3, cuts=[700, 2000])
    assert segs == [5, 5, 5]
    check_against(db[0], pc.ref_power(a, 16, nfft, pc.RECT), nfft, "stream 0 of 3")
    check_against(db[2], pc.ref_power(b, 16, nfft, pc.RECT), nfft, "stream 2 of 3")
    assert (db[1] == pw.FLOOR_DB).all()                      # silence between two loud streams: exactly the floor, no leak, no nan
    # device input at a stride larger than the call, and reset
    stride = n + 13
    dev = torch.zeros(3, 2 * stride, dtype=torch.int16, device="cuda")
    dev[:, :2 * n] = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    ps = pw.PowerSurvey(pc.SR, nfft, center_hz=pc.CENTER_HZ, n_streams=3, max_chunk=n)
    try:
        assert (ps.fetch(0)[1] == pw.FLOOR_DB).all() and ps.segments(0) == 0          # nothing yet: the floor, not nan
        ps.process_device(dev.data_ptr(), stride, n)
        assert [ps.segments(k) for k in range(3)] == [5, 5, 5]
        one = [ps.fetch(k)[1] for k in range(3)]
        whole, _, _, _ = survey_db(x, nfft, pc.RECT, 16, n_streams=3)
        assert all(np.array_equal(one[k], whole[k]) for k in range(3))
        ps.reset()                                           # accumulators, counts AND the 77 carried samples
        assert ps.segments(2) == 0 and (ps.fetch(2)[1] == pw.FLOOR_DB).all()
        ps.process_device(dev.data_ptr(), stride, n)
        assert [ps.segments(k) for k in range(3)] == [5, 5, 5]
        assert all(np.array_equal(ps.fetch(k)[1], whole[k]) for k in range(3))
        # fetch with reset restarts ONE stream's average; its tail stays, the stream goes on
        first = ps.fetch(0, reset=True)[1]
        assert np.array_equal(first, whole[0]) and ps.segments(0) == 0 and ps.segments(2) == 5
        ps.process_device(dev.data_ptr(), stride, nfft - 77)                           # completes the segment the tail began
        assert ps.segments(0) == 1 and ps.segments(2) == 6
        tail_seg = np.concatenate([a[2 * 5 * nfft:], a[:2 * (nfft - 77)]])
        got = ps.fetch(0)[1]
        d_ref, _ = pc.shift_crop_db(pc.ref_power(tail_seg, 16, nfft, pc.RECT), 0.0)
        assert np.max(np.abs(got - d_ref)) <= DB_TOL
    finally:
        ps.close()


@pytest.mark.parametrize("name", list(pc.PEAKS))
def test_peaks_from_the_gpu_spectrum_are_auto_rx_peaks(name, fixture):
    nfft, window, seed, snr, mind = pc.PEAKS[name]
    x = pc.capture(seed)
    db, segs, freq, step = survey_db(x, nfft, window, 16, crop=pc.CROP, cuts=[250_000])
    lo, hi, st = pc.bin_freqs(nfft, pc.CROP)
    assert segs == [len(x) // 2 // nfft] and len(db[0]) == len(fixture[name + "/db"]) and (freq[0], freq[-1], step) == (lo, hi, st)
    worst = np.max(np.abs(db[0] - fixture[name + "/db"]))
    print("%-12s worst bin %.2e dB against the float64 fixture (bound %.3f; margins of the fixture %s dB)" % (name, worst, DB_TOL, np.round(fixture[name + "/margins"], 3)))
    assert worst <= DB_TOL
    peaks, floor = pw.pick_peaks(freq, db[0], step, snr_threshold=snr, min_distance=mind, return_floor=True, **pc.PICK)
    assert abs(floor - float(fixture[name + "/floor"])) <= DB_TOL
    assert len(peaks) == len(fixture[name + "/peaks"]) and (peaks == fixture[name + "/peaks"]).all(), (peaks, fixture[name + "/peaks"])


def _read_log(path):
    rows = []
    for line in open(path):
        f = line.split(", ")
        rows.append((float(f[2]), float(f[3]), float(f[4]), int(f[5]), np.array([float(v) for v in f[6:]])))
    return rows


def test_rtl_power_command_line(tmp_path):
    """auto_rx's literal rtl_power argument string (sdr_wrappers.py:649-658) with the stream named in the environment"""
    x = pc.capture(1)
    raw = tmp_path / "band.cs16"
    raw.write_bytes(x.tobytes())
    env = dict(os.environ, SONDE_POWER_INPUT=str(raw), SONDE_POWER_CFREQ="402000000", SONDE_POWER_SR=str(pc.SR), SONDE_POWER_BITS="16")
    log = tmp_path / "log_power_0.csv"
    start, stop = 401_500_000.0, 402_500_000.0
    args = "-p 0 -d 0 -g 26.0 -f %s:%s:800 -i 1 -1 -c 25%% %s" % (start, stop, log)
    r = subprocess.run([BIN] + args.split(), env=env, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    (lo, hi, st, samples, p), = _read_log(log)
    nfft = 4096                                              # the smallest power of two with 2.4e6 / nfft <= 800
    assert st == pc.SR / nfft and samples == len(x) // 2 // nfft * nfft
    db, _, freq, step = survey_db(x, nfft, pc.RECT, 16, crop=pc.CROP)
    keep = (freq >= start - 1e-3) & (freq <= stop + 1e-3)
    assert len(p) == keep.sum() and abs(lo - freq[keep][0]) < 1e-3 and abs(hi - freq[keep][-1]) < 1e-3 and start <= lo and hi <= stop
    assert np.max(np.abs(p - db[0][keep])) <= DB_TOL
    # -i is honoured: 0.1 s intervals without -1 give one line per interval, the last one from what is left; Hann on request; the stream on stdin
    log2 = tmp_path / "many.csv"
    r = subprocess.run([BIN, "-f", "401e6:403e6:800", "-i", "0.1", "-w", "hann", "-c", "25%", "--input", "-", "--cfreq", "402e6", "--sr", str(pc.SR), str(log2)],
                       input=x.tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = _read_log(log2)
    assert len(rows) == 3 and [row[3] for row in rows] == [58 * nfft, 59 * nfft, 29 * nfft]      # 240000 samples per line: 58.6 segments, the tail carried on
    h, _, _, _ = survey_db(x[:2 * 58 * nfft], nfft, pc.HANN, 16, crop=pc.CROP)
    assert np.max(np.abs(rows[0][4] - h[0])) <= DB_TOL
    # exit codes: less than one segment -> 1 and no file; a range outside the stream, a step finer than 16384 points -> 2
    log3 = tmp_path / "none.csv"
    r = subprocess.run([BIN, "-f", "401e6:403e6:800", "-i", "1", "-1", "--input", "-", "--cfreq", "402e6", "--sr", str(pc.SR), str(log3)],
                       input=x.tobytes()[:4 * 4000], capture_output=True, timeout=120)
    assert r.returncode == 1 and not log3.exists()
    r = subprocess.run([BIN, "-f", "410e6:411e6:800", "-i", "1", "-1", "--cfreq", "402e6", "--sr", str(pc.SR), str(log3)], input=b"", capture_output=True, timeout=120)
    assert r.returncode == 2 and not log3.exists()
    r = subprocess.run([BIN, "-f", "401e6:403e6:100", "-i", "1", "-1", "--cfreq", "402e6", "--sr", str(pc.SR), str(log3)], input=b"", capture_output=True, timeout=120)
    assert r.returncode == 2 and not log3.exists()


def test_receiver_survey_mode_finds_and_decodes():
    """One 2.4 Msps stream with an RS41 and a DFM09 off the raster, nothing told to the receiver: survey -> peaks -> scanner per peak -> decoders.
    Frames: the raster test's allowance (tests/test_gpu_chain.py: every second but 3) less the first survey (1 s) and one second of dwell."""
    from tools import synth
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden
    from radiosonde_auto_rx_amd.wideband import WidebandReceiver
    sr, cf, secs = 2_400_000, 403_000_000, 6.3
    n = int(sr * secs)
    hz, t0 = +203_400.0, 0.2
    cap = synth.rs41_capture(sr=sr, seconds=secs, fq=0.0, n_frames=int(secs - t0), t_first=t0, noise_sigma=0.0, amp=0.25, seed=200, sonde_id="A1111111", first_frame_no=100,
                             frame_kw=dict(ecef_cm=(418833319, 85974133, 473346430), cal_table=synth.rs41_cal_table(seed=0, freq_khz=int(round((cf + hz) / 10000.0)) * 10)))
    x = (cap[0::2].astype(np.float64) + 1j * cap[1::2].astype(np.float64)) / (32767 * 0.9) * np.exp(2j * np.pi * hz / sr * np.arange(n))
    dsym = (make_golden.dfm_field_symbols(dict(kind="09", n=60, sn=18012345)) > 0).astype(np.uint8)
    dz = 0.2 * synth.gfsk_baseband(dsym, sr, 2500.0, 2400.0)[:n]
    x[:len(dz)] += dz * np.exp(2j * np.pi * (-700_600.0) / sr * np.arange(len(dz)))
    rng = np.random.default_rng(5)
    x += 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    iq = np.empty(2 * n, np.int16)
    iq[0::2] = np.clip(np.round(x.real * 32767 * 0.9), -32768, 32767); iq[1::2] = np.clip(np.round(x.imag * 32767 * 0.9), -32768, 32767)

    plain = WidebandReceiver(sr, cfreq_hz=cf)
    assert plain.survey is None and plain.scanner is not None            # the default: the raster, no PowerSurvey
    plain.close()

    rx = WidebandReceiver(sr, cfreq_hz=cf, survey_s=1.0)
    assert rx.scanner is None and rx.survey is not None                   # no raster scanner in survey mode
    out = rx.push(iq, finish=True)
    found = {s["khz"]: s["type"] for s in rx.sondes}
    log = rx.log
    rx.close()
    for j in out[:3]:
        print(j)
    rounds = [e for e in log if e["event"] == "survey"]
    assert len(rounds) >= 2 and all(len(e["freq"]) == len(e["power"]) == 3072 and len(e["peak_freq"]) == len(e["peak_lvl"]) for e in rounds)
    assert {round(f, 2) for f in rounds[0]["peak_freq"]} >= {403.20, 402.30} and rounds[0]["threshold"] < -50.0
    assert any(abs(k - (cf + hz) / 1e3) <= 2 and t == "RS41" for k, t in found.items()), found
    assert any(abs(k - (cf - 700_600) / 1e3) <= 2 and t == "DFM" for k, t in found.items()), found
    assert len(found) == 2, log
    rs = [j for j in out if j["type"] == "RS41"]
    # "freq" is the channel frequency until the sonde's own configuration subframe 0 has been seen, then the transmitted one (10 kHz steps)
    assert all(j["id"] == "A1111111" and abs(j["freq"] - (cf + hz) / 1e3) <= 6 and abs(j["lat"] - 48.1) < 1e-4 for j in rs), rs[:2]
    frames = [j["frame"] for j in rs]
    assert frames == sorted(frames) and len(set(frames)) == len(frames)
    assert len(rs) >= int(secs - t0) - 3 - 1 - 1, len(rs)
    dfm = [j for j in out if j["type"] == "DFM"]
    assert len(dfm) >= 3 and all(j["id"] in ("DFM-18012345", "DFM-xxxxxxxx") and abs(j["freq"] - (cf - 700_600) // 1000) <= 2 for j in dfm), dfm[:2]
