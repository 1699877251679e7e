"""Jobs, decoders and the emulator shared by tests/test_gps_subsets_emu.py (the device RS92 subset search under the CPU wave emulator) and tests/test_gpu_gps.py (the
same source as k_gps_subsets on the device).  A job is what sonde_rs92_dec_begin makes of a frame (tools/synth_rs92.py flights decoded with ephemerides), so the
constructed cases are flights too: the satellite count through `order=`, the height through `alt=`, bad geometry through a sub-horizon constellation; a duplicated
satellite, garbage ranges and the height-gate job are edits of such a job.  The oracle is sonde_gps_host_solve: the host decoder's own closed form and DOP."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np

import rs92_softin_cases as M
from tools import synth_rs92 as R
from radiosonde_auto_rx_amd import gps

sys.path.insert(0, os.path.join(M.ROOT, "tools"))
import make_golden  # noqa: E402

EMU_SRC = os.path.join(M.EMU_DIR, "gps_subsets_emu.cpp")
EMU_SO = os.path.join(M.EMU_DIR, "libgps_subsets_emu.so")
REPLAY_SRC = os.path.join(M.EMU_DIR, "gps_subsets_replay.cpp")
DEPS = [EMU_SRC, os.path.join(M.EMU_DIR, "wave_emu.h"), os.path.join(M.CSRC, "sonde_gps_dev.h"), os.path.join(M.CSRC, "sonde_rs_dev.h"),
        os.path.join(M.ROOT, "include", "sonde_rs92.h")]
SOLVE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p)
SCENARIOS = ["rs92f_sgp_36", "rs92f_ngp_36", "rs92f_spoiled_8", "rs92f_prn32_6", "rs92f_noisy_12"]
# tests/test_rs92_corrected.py OPTS, plus --vel2 with ephemerides
OPTS = {
    "raw": (dict(raw=1, verbose=1), None),
    "autorx_eph": (dict(M.AUTORX, inv=1, version=b"test"), "E"),
    "vv_ecc2_eph": (dict(verbose=4, aux=1, ptu=1, ecc=2, gpsepoch=-1), "E"),
    "g2_vel2_alm": (dict(verbose=1, gps_verbose=2, gps_vel=2, gpsepoch=-1), "A"),
    "vel_alm_epoch2": (dict(verbose=1, gps_vel=4, gpsepoch=2), "A"),
    "vel2_eph": (dict(verbose=1, gps_vel=2, gpsepoch=-1), "E"),
}
SUBHORIZON = [17, 32, 11, 6, 28, 1, 13, 19, 24, 30, 3, 9]          # the slot order of rs92f_prn32_6: twelve satellites wherever they stand


def load_emu():
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(d) > os.path.getmtime(EMU_SO) for d in DEPS):
        tmp = EMU_SO + ".%d.tmp" % os.getpid()
        # (-ffp-contract=off: which subset wins is decided by products and sums each rounded on its own)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", tmp, EMU_SRC])
        os.replace(tmp, EMU_SO)
    L = C.CDLL(EMU_SO)
    L.emu_gps_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.emu_gps_unrank.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
    return L


def load_host():
    H = M.load_host()
    gps._lib()
    H.sonde_rs92_dec_begin.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.POINTER(gps.GpsJob)]
    H.sonde_rs92_dec_end.argtypes = [C.c_void_p, C.POINTER(gps.GpsPick), C.c_char_p, C.c_size_t]
    H.sonde_rs92_dec_gps_via.argtypes = [C.c_void_p]
    H.sonde_gps_host_solve.argtypes = [C.POINTER(gps.GpsJob), C.POINTER(gps.GpsPick)]
    H.sonde_gps_job_fill.argtypes = [C.POINTER(gps.GpsJob), C.c_int32] + [C.POINTER(C.c_double)] * 4
    H.sonde_gps_rs92_text_batch_with.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_size_t,
                                                 C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    H.sonde_gps_rs92_text_batch.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)]
    return H


def emu_solve(E, jobs):
    n = len(jobs)
    arr = (gps.GpsJob * max(n, 1))(*jobs)
    picks = (gps.GpsPick * max(n, 1))()
    assert E.emu_gps_solve(None, arr, n, picks) == 0
    return [picks[i] for i in range(n)]


def host_solve(H, job):
    p = gps.GpsPick()
    assert H.sonde_gps_host_solve(C.byref(job), C.byref(p)) == 0
    return p


def total(n):
    return n * (n - 1) * (n - 2) * (n - 3) // 24


def scenario_frames(name, eph):
    sc = make_golden.RS92_FIELD_SCENARIOS[name]
    kw = {k: v for k, v in sc.items() if k not in ("n", "ngp", "aux", "sigma")}
    cal = R.cal_rows(seed=5, freq_khz=1680500, ngp_key=bytes(range(0x31, 0x41))) if sc.get("ngp") else None
    return R.flight(sc["n"], eph, cal=cal, ngp=bool(sc.get("ngp")), aux=sc.get("aux", (0, 0, 0, 0)), **kw)


def damaged(frames, seed):
    """every third frame clean, the others with byte errors, two beyond correction: their CRCs fail, and the decoder gets them as received"""
    rng = np.random.default_rng(seed)
    out = []
    for k, f in enumerate(frames):
        f = bytearray(f)
        nerr = 0 if k % 3 == 0 else 14 if k == 4 else 30 if k == 7 else 1 + (5 * k) % 12
        for p in rng.choice(np.arange(6, 240), nerr, replace=False):
            f[int(p)] ^= int(rng.integers(1, 256))
        out.append(bytes(f))
    return out


def corrected(H, frames):
    """[(frame bytes behind rs92_ecc, ec)] by a `-r -v` decoder, as tests/test_rs92_corrected.py takes them"""
    r = M.host_dec(H, raw=1, verbose=1)
    line, out = C.create_string_buffer(1024), []
    for f in frames:
        assert H.sonde_rs92_dec_bytes(r, f, 240, line, 1024) > 0
        ec, fixed = M.parse_raw_line(line.value.decode().rstrip("\n"))
        out.append((fixed, ec))
    H.sonde_rs92_dec_destroy(r)
    return out


def jobs_of(H, frames, E, **kw):
    """the jobs sonde_rs92_dec_begin makes of clean frames under the auto_rx options with ephemerides (frames that give none are left out)"""
    o = dict(M.AUTORX, inv=1)
    o.update(kw)
    d = M.host_dec(H, ephemeris=E, **o)
    buf, out = C.create_string_buffer(1 << 16), []
    for f in frames:
        j = gps.GpsJob()
        rc = H.sonde_rs92_dec_begin(d, f, 0, C.byref(j))
        assert rc in (0, 1)
        assert H.sonde_rs92_dec_end(d, None, buf, len(buf)) >= 0
        if rc:
            out.append(j)
    H.sonde_rs92_dec_destroy(d)
    return out


def refill(H, X, Y, Z, p):
    n = len(p)
    a = [(C.c_double * n)(*[float(v) for v in q]) for q in (X, Y, Z, p)]
    j = gps.GpsJob()
    assert H.sonde_gps_job_fill(C.byref(j), n, *a) == 0
    return j


def columns(job):
    n = job.n
    return ([job.sat[i].X for i in range(n)], [job.sat[i].Y for i in range(n)], [job.sat[i].Z for i in range(n)], [job.sat[i].p for i in range(n)])


_constructed = {}
DUP_SLOTS = []                # per job of constructed()["duplicate"]: the two slots that hold the same satellite


def constructed(H, eph, E):
    """name -> list of jobs (see the module text)"""
    if _constructed:
        return _constructed
    c = _constructed
    for n in (4, 5, 11, 12):
        c["n%d" % n] = jobs_of(H, R.flight(2, eph, order=SUBHORIZON[:n], min_elev_deg=-90.0), E)
        assert len(c["n%d" % n]) == 2 and all(j.n == n for j in c["n%d" % n]), (n, [j.n for j in c["n%d" % n]])
    # a satellite in two slots: subsets with both copies have two equal rows (|det| < 1e-4: GDOP -1), and a subset with one copy has a twin with the other
    base = jobs_of(H, R.flight(1, eph), E)[0]
    X, Y, Z, p = [q[:8] for q in columns(base)]
    w = list(itertools.combinations(range(8), 4))[host_solve(H, refill(H, X, Y, Z, p)).best]      # (the copies are of satellites of the winning subset: its twin ties)
    a, b = w[3], w[0]            # (the copy takes the original's PLACE in the subset, last or first: the same operands in the same order, the same bits)
    c["duplicate"] = [refill(H, X + [X[a]], Y + [Y[a]], Z + [Z[a]], p + [p[a]]), refill(H, [X[b]] + X, [Y[b]] + Y, [Z[b]] + Z, [p[b]] + p)]
    DUP_SLOTS[:] = [(a, 8), (0, b + 1)]
    # ranges of garbage: no subset has a solution inside the height gate
    rng = np.random.default_rng(92)
    c["garbage"] = [refill(H, X, Y, Z, list(rng.uniform(1e8, 3e8, len(p)))), refill(H, X, Y, Z, list(rng.uniform(0.0, 5e7, len(p))))]
    # ranges that agree within 1000 km: an odd subset has a solution inside the gate, hardly ever with a usable geometry
    c["near_garbage"] = [refill(H, X, Y, Z, list(np.random.default_rng(s).uniform(-1e6, 1e6, len(p)))) for s in (92, 93)]
    # a flight at the upper edge of the height gate: the 1.5 m range noise puts subsets on both sides of it
    c["gate_50km"] = jobs_of(H, R.flight(6, eph, alt=50000.0, vel_enu=(12.5, -7.25, 0.0)), E)
    # sub-horizon constellation: bad geometries
    c["subhorizon"] = jobs_of(H, R.flight(4, eph, order=SUBHORIZON, min_elev_deg=-90.0, tow_ms=302470_000), E)
    return c


def gate_job(H, base):
    """base (a flight a few metres below the 50000 m edge of the height gate, no range noise) with ONE pseudorange moved, by bisection with the host oracle, until
    the closed-form height of subset (0, 1, 2, 3) stands on the edge: num of the 4-satellite job flips from 1 to 0 there.  The bisection runs until the two
    pseudoranges are neighbours as doubles, so the height is within a rounding of the edge: far inside 0.005 m.  -> (the job with all its satellites, the move in
    metres: a few tens at the most, which is what tells this edge from the lower one 50 km away)"""
    X, Y, Z, p = columns(base)

    def inside(dp):
        return host_solve(H, refill(H, X[:4], Y[:4], Z[:4], p[:3] + [p[3] + dp])).num == 1
    assert inside(0.0)
    for sign in (1.0, -1.0):
        lo, hi, step = 0.0, None, 0.25
        while step <= 256.0 and hi is None:
            if inside(sign * step):
                lo = step
            else:
                hi = step
            step *= 2
        if hi is None:
            continue
        while True:
            mid = 0.5 * (lo + hi)
            if mid == lo or mid == hi or p[3] + sign * mid in (p[3] + sign * lo, p[3] + sign * hi):
                break
            if inside(sign * mid):
                lo = mid
            else:
                hi = mid
        return refill(H, X, Y, Z, p[:3] + [p[3] + sign * lo] + p[4:]), sign * lo
    raise AssertionError("no move of 256 m takes the subset through the gate")


_gate = []


def gate(H, eph, E):
    """the job with a subset on the 50000 m edge of the height gate (gate_job), made once"""
    if not _gate:
        base = jobs_of(H, R.flight(1, eph, alt=49990.0, vel_enu=(12.5, -7.25, 0.0), noise_m=0.0), E)[0]
        job, dp = gate_job(H, base)
        assert abs(dp) < 256.0
        _gate.append(job)
    return _gate[0]


def all_jobs(H, eph, E):
    """the jobs of the selection and doubt tests in one list (the sanitizer replay and the GPU test run them)"""
    jobs = [j for v in constructed(H, eph, E).values() for j in v] + [gate(H, eph, E)]
    for name in ("rs92f_sgp_36", "rs92f_prn32_6"):
        jobs += jobs_of(H, scenario_frames(name, eph), E)[:6]
    return jobs


def handles(hs):
    return (C.c_void_p * len(hs))(*[h.value for h in hs])
