"""Goldens of the spectrum survey (tests/golden/power_*.npz).  Runs on the CPU; auto_rx is imported read-only from the reference tree and only
DATA is written: float64 spectra, peak lists, random peak-pick cases with auto_rx's answers, one parsed log line.  Captures are not stored; the
tests regenerate them with the seeded tools.synth.wideband_capture.

    python -m tools.make_golden_power

power_spectra.npz  per case of power_cases.SPECTRA: the float64 periodogram (linear, transform order) and numpy's complex64 periodogram's
                   difference from it (norm-wise, and worst kept bin in dB): the yardstick the GPU's own difference is printed beside.
power_fixture.npz  per fixture of power_cases.PEAKS: the float64 spectrum [dB] over the kept bins, auto_rx's peak list and noise floor, and
                   the three margins the fixture is chosen for (all >= 0.05 dB, ten times the spectrum tolerance, so that a spectrum within
                   0.005 dB per bin cannot change the answer).
power_peaks.npz    random peak-pick cases (power_cases.random_case) with auto_rx's peaks and noise floor.
power_csv.npz      one log line of sonde_power_csv_line as auto_rx's two readers parse it.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import power_cases as pc                                   # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
N_RANDOM = 240
MARGIN_DB = 0.05


def spectra():
    out = {}
    for name, (nfft, window, bits, n, first) in pc.SPECTRA.items():
        x = pc.spectrum_input(name)
        p64 = pc.ref_power(x, bits, nfft, window)
        p32 = pc.ref_power(x, bits, nfft, window, single=True)
        d64, _ = pc.shift_crop_db(p64, pc.CROP)
        d32, _ = pc.shift_crop_db(p32, pc.CROP)
        out[name + "/power"] = p64
        out[name + "/c64_norm"] = np.linalg.norm(p32 - p64) / np.linalg.norm(p64)
        out[name + "/c64_db"] = np.max(np.abs(d32 - d64))
        print("%-18s segments %d  dynamic range %.1f dB  complex64: norm-wise %.2e, worst kept bin %.2e dB (bound %.2e / 0.005)"
              % (name, n // nfft, d64.max() - d64.min(), out[name + "/c64_norm"], out[name + "/c64_db"], 8 * np.log2(nfft) * 2.0 ** -24))
    np.savez_compressed(os.path.join(GOLDEN, "power_spectra.npz"), **out)


def fixture_margins(db, step, snr, min_distance, nf, kept_idx):
    """the three distances a 0.005 dB error would have to bridge to change the pick"""
    thr = nf + snr
    mx = pc.local_maxima(db)
    m_thr = np.min(np.abs(db[mx] - thr))
    above = mx[db[mx] >= thr]
    mpd = min_distance / step
    m_pair = np.inf
    for a in above:
        for b in above:
            if a < b and b - a <= mpd + 1:
                m_pair = min(m_pair, abs(db[a] - db[b]))
    lv = np.sort(db[kept_idx])
    m_order = np.min(np.diff(lv)) if len(lv) > 1 else np.inf
    return float(m_thr), float(m_pair), float(m_order)


def fixtures(scan_mod):
    out = {}
    for name, (nfft, window, seed, snr, mind) in pc.PEAKS.items():
        x = pc.capture(seed)
        db, _ = pc.shift_crop_db(pc.ref_power(x, 16, nfft, window), pc.CROP)
        lo, hi, step = pc.bin_freqs(nfft, pc.CROP)
        freq = np.linspace(lo, hi, len(db))
        peaks, nf = pc.autorx_pick(scan_mod, freq, db, step, snr_threshold=snr, min_distance=mind, never_scan=[], **pc.PICK)
        # bins auto_rx's detect_peaks kept (before quantisation): the local maxima above the threshold that no higher one within mpd suppresses
        import autorx.utils as au
        kept = au.detect_peaks(db, mph=nf + snr, mpd=mind / step)
        # the median moves by at most the tolerance too: it enters the threshold margin
        margins = fixture_margins(db, step, snr, mind, nf, kept)
        print("%-12s bins %d  floor %.2f dB  peaks %s  margins: threshold %.3f dB, neighbours %.3f dB, order %.3f dB"
              % (name, len(db), nf, [round(p / 1e3) for p in peaks], *margins))
        assert min(margins) >= MARGIN_DB, (name, margins)
        for sg in pc.SIGNALS:                                                           # the three sondes are among the peaks (to one quantisation step)
            assert np.min(np.abs(peaks - (pc.CENTER_HZ + sg["fq"] * pc.SR))) <= pc.PICK["quantization"], (name, peaks, sg)
        out[name + "/db"] = db
        out[name + "/peaks"] = peaks
        out[name + "/floor"] = nf
        out[name + "/margins"] = np.array(margins)
    np.savez_compressed(os.path.join(GOLDEN, "power_fixture.npz"), **out)


def random_cases(scan_mod):
    rng = np.random.default_rng(20240611)
    powers, peaks, meta, never = [], [], [], []
    kinds = {}
    for i in range(N_RANDOM):
        c = pc.random_case(rng, i)
        n = len(c["power"])
        freq = np.linspace(c["f_low"], c["f_high"], n)
        mx = pc.local_maxima(c["power"]) if n >= 3 else np.array([], dtype=int)
        v = c["power"][mx]
        v = v[~np.isnan(v)]
        assert len(np.unique(v)) == len(v), "tie between local maxima"
        pk, nf = pc.autorx_pick(scan_mod, freq, c["power"], c["step"], **pc.case_kwargs(c))
        kinds[i % 12] = kinds.get(i % 12, 0) + len(pk)
        powers.append(c["power"]); peaks.append(pk); never.append(np.array(c["never_scan"], dtype=np.float64))
        meta.append([c["f_low"], c["f_high"], c["step"], c["snr_threshold"], c["min_distance"], c["quantization"], c["min_freq"], c["max_freq"],
                     c["max_peaks"], nf])
    print("random cases: %d, peaks per kind %s" % (N_RANDOM, kinds))
    cat = lambda a: (np.concatenate(a) if a else np.zeros(0), np.cumsum([0] + [len(v) for v in a]))
    p, po = cat(powers); k, ko = cat(peaks); nv, no = cat(never)
    np.savez_compressed(os.path.join(GOLDEN, "power_peaks.npz"), power=p, power_off=po, peaks=k, peaks_off=ko, never=nv, never_off=no, meta=np.array(meta))


def csv_case(scan_mod, sdr_mod):
    from radiosonde_auto_rx_amd import power as pw
    rng = np.random.default_rng(5)
    nfft = 4096
    lo, hi, step = pc.bin_freqs(nfft, pc.CROP)
    db = (-80.0 + 60.0 * rng.random(nfft - 2 * int(pc.CROP * nfft / 2))).astype(np.float32)
    db[7] = pc.FLOOR_DB
    line = pw.csv_line(1_700_000_000, lo, hi, step, 600_000, db)
    with tempfile.NamedTemporaryFile("w", suffix=".csv", delete=False) as f:
        f.write(line)
    try:
        f1, p1, s1 = sdr_mod.read_rtl_power_log(f.name, "golden")
        f2, p2, s2 = scan_mod.read_rtl_power(f.name)
    finally:
        os.unlink(f.name)
    assert (f1 == f2).all() and (p1 == p2).all() and s1 == s2
    assert (f1 == np.linspace(lo, hi, len(db))).all() and np.max(np.abs(p1 - db)) <= 0.005 and s1 == step
    np.savez_compressed(os.path.join(GOLDEN, "power_csv.npz"), db=db, line=np.array(line), freq=f1, power=p1, step=s1, args=np.array([lo, hi, step]))
    print("csv: %d bins, line %d bytes, head %r" % (len(db), len(line), line[:90]))


def main():
    mods = pc.autorx_modules()
    assert mods, "the reference tree is needed to record auto_rx's answers"
    scan_mod, sdr_mod, _ = mods
    spectra()
    fixtures(scan_mod)
    random_cases(scan_mod)
    csv_case(scan_mod, sdr_mod)


if __name__ == "__main__":
    main()
