"""k_gps_subsets on the device (radiosonde_auto_rx_amd/csrc/sonde_gps.hip): the RS92 position solve's 4-satellite subset search.
1. the direct entry sonde_gps_dev_solve on the jobs of tests/test_gps_subsets_emu.py: every pick equals the CPU wave emulator's field for field, gdop bit for bit
   (which is what shows that the device's f64 divide and sqrt round as the host's do), in batches of 1, 63, 64, 65 and one larger than max_jobs;
2. SoftinDev(kind="rs92", gps_device=True) against gps_device=False on the same soft symbols: texts and JSON byte for byte, no mismatch, the emulator's doubts;
3. family.rs92_text_batch on the records of a generic RS92 engine against FamilyDecoder.decoded record by record;
4. with the switch off nothing is counted and the existing path runs."""
import ctypes as C

import numpy as np
import pytest

import gps_cases as G
import rs92_softin_cases as M
from radiosonde_auto_rx_amd import gps
from tools import synth_rs92 as R

pytestmark = pytest.mark.gpu
SR = 48_000


@pytest.fixture(scope="module")
def host():
    return G.load_host()


@pytest.fixture(scope="module")
def emu():
    return G.load_emu()


@pytest.fixture(scope="module")
def orbits(tmp_path_factory):
    return G.make_golden.rs92_orbit_files(str(tmp_path_factory.mktemp("gpsgpu")))


# ---------------------------------------------------------------- 1. the direct entry against the emulator
def test_direct_entry_equals_the_emulator_bit_for_bit(host, emu, orbits):
    eph, E, A = orbits
    jobs = G.all_jobs(host, eph, E)
    want = [p.key() for p in G.emu_solve(emu, jobs)]
    assert len(jobs) > 20 and sum(k[2] for k in want) >= 1                       # (the gate job is in doubt)
    s = gps.GpsSolver(max_jobs=64)
    launches = 0
    for n in (1, 63, 64, 65, 150):                                               # 150: three chunks of at most 64
        idx = [i % len(jobs) for i in range(n)]
        got = s.solve([jobs[i] for i in idx])
        assert [p.key() for p in got] == [want[i] for i in idx], n
        launches += -(-n // 64)
        st = s.stats()
        assert st["launches"] == launches
    st = s.stats()
    assert st["jobs"] == 1 + 63 + 64 + 65 + 150 and st["doubts"] >= 5 and st["mismatches"] == 0
    assert s.solve([]) == []
    s.close()


def test_solve_refuses_bad_jobs(host, orbits):
    eph, E, A = orbits
    j = G.jobs_of(host, R.flight(1, eph), E)[0]
    s = gps.GpsSolver(max_jobs=4)
    L = gps._lib()
    picks = (gps.GpsPick * 2)()
    for n in (3, 13, 0, -1):
        bad = gps.GpsJob.from_buffer_copy(bytes(j))
        bad.n = n
        assert L.sonde_gps_dev_solve(s._h, (gps.GpsJob * 2)(j, bad), 2, picks) == -1
    for field, v in (("X", float("nan")), ("p", float("inf")), ("z", float("-inf"))):
        bad = gps.GpsJob.from_buffer_copy(bytes(j))
        setattr(bad.sat[j.n - 1], field, v)
        assert L.sonde_gps_dev_solve(s._h, (gps.GpsJob * 2)(j, bad), 2, picks) == -1
    bad = gps.GpsJob.from_buffer_copy(bytes(j))
    if j.n < 12:
        bad.sat[11].X = float("nan")                                              # behind the job's n: not looked at
        assert L.sonde_gps_dev_solve(s._h, (gps.GpsJob * 1)(bad), 1, picks) == 0
    assert L.sonde_gps_dev_solve(None, (gps.GpsJob * 1)(j), 1, picks) == -1 and L.sonde_gps_dev_solve(s._h, None, 1, picks) == -1
    assert L.sonde_gps_dev_solve(s._h, (gps.GpsJob * 1)(j), 1, None) == -1 and L.sonde_gps_dev_solve(s._h, (gps.GpsJob * 1)(j), -1, picks) == -1
    assert s.stats()["launches"] == (1 if j.n < 12 else 0)
    h = C.c_void_p()
    assert L.sonde_gps_dev_create(0, C.byref(h)) == -1 and L.sonde_gps_dev_create(4, None) == -1 and L.sonde_gps_dev_stats(None, None) == -1
    s.close()


# ---------------------------------------------------------------- 2. the soft-bit consumer with and without the device search
CONSUMERS = {
    "sgp_eph_autorx": (dict(M.AUTORX, inv=0, version="t"), "E", {}),
    "ngp_eph": (dict(M.AUTORX, inv=0, ngp=1, ptu=1), "E", dict(ngp=True)),
    "alm_vel": (dict(verbose=1, gps_vel=4, gpsepoch=2, json=0, ecc=1, aux=0, inv=0), "A", {}),
}


def _streams(eph, ngp=False):
    """three channels, six frames each (different flights), behind leads of different length: equally long soft-symbol streams"""
    cal = R.cal_rows(seed=5, freq_khz=1680500, ngp_key=bytes(range(0x31, 0x41))) if ngp else None
    rng = np.random.default_rng(7)
    body = [M.soft(R.onair_symbols(R.flight(6, eph, seed=1 + c, frame0=100 + 40 * c, cal=cal, ngp=ngp, lat=47.7 + c), lead=0)) for c in range(3)]
    n = max(len(b) for b in body) + 3000
    out = []
    for c, b in enumerate(body):
        lead = M.noise(rng, 300 + 1100 * c, 0.05)
        out.append(np.concatenate([lead, b, M.noise(rng, n - len(lead) - len(b), 0.05)]))
    return out


def _consume(streams, opts, files, gps_device, call):
    import torch
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    S = np.ascontiguousarray(np.stack(streams), np.float32)
    sf = SoftinDev(len(streams), kind="rs92", rs92_opts=opts, gps_device=gps_device, **files)
    d = torch.from_numpy(S).cuda()
    fetches = []
    for pos in range(0, S.shape[1], call):
        chunk = d[:, pos:pos + call].contiguous()
        sf.push_device(chunk.data_ptr(), chunk.shape[1], chunk.shape[1])
        fetches.append(sf.fetch_rs92())
    st = sf.rs92_gps_stats()
    sf.close()
    return fetches, st


@pytest.mark.parametrize("name", sorted(CONSUMERS))
def test_consumer_with_the_device_search_prints_the_same(host, emu, orbits, name):
    eph, E, A = orbits
    opts, orb, skw = CONSUMERS[name]
    files = dict(ephemeris=E) if orb == "E" else dict(almanac=A)
    streams = _streams(eph, **skw)
    call = 3 * M.ONAIR                                                           # three frames a call: a fetch holds two or three records of a channel
    on, st = _consume(streams, opts, files, True, call)
    off, st_off = _consume(streams, opts, files, False, call)
    # (records of different channels come in the order their waves finished; a channel's own are in stream order)
    per = lambda fetches: [[[(r["ec"], r["hdr_bit"], r["frame"], r["text"]) for r in f if r["channel"] == c] for f in fetches] for c in range(3)]      # noqa: E731
    assert per(on) == per(off)
    recs = [r for f in on for r in f]
    assert len(recs) == 18 and all(" lat: " in r["text"] for r in recs)
    assert any(sum(r["channel"] == c for r in f) >= 2 for f in on for c in range(3))
    if opts.get("json"):
        assert sum(r["text"].count('"lat"') for r in recs) == 18
    # the emulator's doubts on the same frames: a decoder per channel gives the jobs
    doubts = jobs = 0
    for c in range(3):
        o = dict(opts)
        if isinstance(o.get("version"), str):
            o["version"] = o["version"].encode()
        d = M.host_dec(host, **files, **o)
        buf = C.create_string_buffer(1 << 16)
        for r in recs:
            if r["channel"] != c:
                continue
            j = gps.GpsJob()
            rc = host.sonde_rs92_dec_begin(d, r["frame"], r["ec"], C.byref(j))
            assert host.sonde_rs92_dec_end(d, None, buf, len(buf)) >= 0
            if rc == 1:
                jobs += 1
                doubts += G.emu_solve(emu, [j])[0].doubt
        host.sonde_rs92_dec_destroy(d)
    assert st["mismatches"] == 0 and st["doubts"] == doubts and st["jobs"] == jobs == 18 and st["picked"] == jobs - doubts
    assert st["launches"] <= 3 * len([f for f in on if f])                       # a launch per round of a fetch, not per frame
    assert st_off == dict(jobs=0, launches=0, doubts=0, mismatches=0, picked=0)


# ---------------------------------------------------------------- 3. family hits of a generic RS92 engine
def test_family_batch_equals_decoded_record_by_record(orbits, tmp_path):
    from radiosonde_auto_rx_amd.engine import Engine
    from radiosonde_auto_rx_amd.family import FAMILY, FamilyDecoder, rs92_text_batch
    eph, E, A = orbits
    caps = [R.rs92_capture(R.flight(4, eph, seed=3 + c, lat=47.7 - c), sr=SR, noise_sigma=0.01, seed=17 + c) for c in range(2)]
    n = min(len(a) for a in caps) // 2
    x = np.stack([a[:2 * n] for a in caps])
    f = FAMILY["RS92"]
    eng = Engine([0.0] * 2, SR, sonde="generic", generic=f["generic"], thres=f["thres"], auto=f["auto"], keep_soft=True, lp_iq=True, max_chunk=SR // 2, max_frames=64)
    eng.set_family("RS92", ecc=1)
    mk = lambda: [FamilyDecoder("RS92", version="t", freq_khz=403000, ephemeris=E, verbose=1) for _ in range(2)]      # noqa: E731
    da, db = mk(), mk()
    solver = gps.GpsSolver(max_jobs=16)
    one, batch = [], []
    for s0 in range(0, n, SR // 2):
        eng.process_host(np.ascontiguousarray(x[:, 2 * s0:2 * min(n, s0 + SR // 2)]))
        recs = eng.fetch_family()
        one += [da[r["channel"]].decoded(r) for r in recs]
        batch += rs92_text_batch(db, recs, solver)
    recs = eng.fetch_family(finish=True)
    one += [da[r["channel"]].decoded(r) for r in recs]
    batch += rs92_text_batch(db, recs, solver)
    eng.close()
    assert batch == one and len(one) >= 7 and sum('"lat"' in t for t in one) >= 7
    st = solver.stats()
    assert st["mismatches"] == 0 and st["jobs"] >= 7 and st["picked"] == st["jobs"] - st["doubts"]
    assert rs92_text_batch(db, [], solver) == []
    solver.close()


# ---------------------------------------------------------------- 4. off by default
def test_default_is_off(orbits):
    import torch
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    eph, E, A = orbits
    s = np.concatenate([M.soft(R.onair_symbols(R.flight(2, eph), lead=0)), np.zeros(200, np.float32)])
    sf = SoftinDev(1, kind="rs92", rs92_opts=dict(inv=0), ephemeris=E)
    d = torch.from_numpy(s[None, :].copy()).cuda()
    sf.push_device(d.data_ptr(), len(s), len(s))
    recs = sf.fetch_rs92()
    assert len(recs) == 2 and all(" lat: " in r["text"] for r in recs)
    assert sf.rs92_gps_stats() == dict(jobs=0, launches=0, doubts=0, mismatches=0, picked=0)
    sf.set_rs92_gps(True); sf.set_rs92_gps(False)                                # made and switched off again: still the existing path
    sf.push_device(d.data_ptr(), len(s), len(s))
    assert len(sf.fetch_rs92()) >= 1 and sf.rs92_gps_stats()["jobs"] == 0
    sf.close()
    with pytest.raises(ValueError):
        SoftinDev(1, kind="m20", gps_device=True)
