"""k_family_hits on the device (radiosonde_auto_rx_amd/csrc/sonde_family_hits.hip): the per-hit decoders of generic engines carrying Meisei, iMet-54, MTS01 or RS92.
1. the direct entry on the constructed hits of tests/test_family_hits_emu.py: records equal the CPU wave emulator's, field for field;
2. per kind two engines on the same samples — one with set_family / fetch_family / FamilyDecoder.decoded, one with fetch_hits / FamilyDecoder.hit: text, mv,
   mv_pos and nbits per channel are identical, and the clean channel decodes (the arbiter is the host tier sonde_<kind>_dec_frame on the same soft bits);
3. ring and fetch edges on Meisei; 4. refusals; 5. the WidebandReceiver with device_family on and off.
Every comparison is byte for byte."""
import re

import numpy as np
import pytest

import family_hits_cases as F
from radiosonde_auto_rx_amd.family import FAMILY, FamilyDecoder, decode_hits_device

pytestmark = pytest.mark.gpu
SR = 48_000


# ---------------------------------------------------------------- 1. the direct entry against the emulator
@pytest.mark.parametrize("kind", F.KINDS)
def test_direct_entry_equals_the_emulator_field_for_field(kind):
    emu = F.load_emu()
    for ecc, hs in F.by_ecc(kind):
        reps = -(-300 // len(hs)) if ecc else 1                                  # a few hundred hits in one launch
        softs = [h[1] for h in hs] * reps
        want, _ = F.emu_run(emu, kind, ecc, [h[1] for h in hs], None, grid=len(hs))      # (the direct entry has no header score: mv = 0)
        got = decode_hits_device(kind, softs, ecc=ecc)
        assert len(got) == len(softs)
        for i, r in enumerate(got):
            w = dict(want[i % len(hs)], channel=i)
            assert F.rec_key(r) == F.rec_key(w), (hs[i % len(hs)][0], i)
        assert sum(r["decoded"] for r in got) == reps * sum(len(h[1]) == F.NB[kind] for h in hs) > 0


# ---------------------------------------------------------------- 2. two engines on the same samples
def _noise(n, seed, sigma=0.05):
    rng = np.random.default_rng(seed)
    return np.clip(np.round(rng.normal(0.0, sigma * 32767, 2 * n)), -32768, 32767).astype(np.int16)


def _captures(kind, tmp_path):
    """-> ([clean, noisier, noise only] int16 IQ of equal length, frames synthesized whole on the clean channel, decoder keywords)"""
    from tools import synth, synth_rs92 as R
    kw = {}
    if kind == "MEISEI":
        a, b, frames = synth.meisei_capture(sr=SR, seconds=5.2, noise_sigma=0.02, seed=11), synth.meisei_capture(sr=SR, seconds=5.2, noise_sigma=0.22, seed=12), 10
    elif kind == "IMET5":
        a, b, frames = synth.imet54_capture(sr=SR, seconds=5.2, noise_sigma=0.02, seed=13), synth.imet54_capture(sr=SR, seconds=5.2, noise_sigma=0.2, seed=14, check="cont"), 5
    elif kind == "MTS01":
        a, b, frames = synth.mts01_capture(sr=SR, seconds=5.2, noise_sigma=0.02, seed=15), synth.mts01_capture(sr=SR, seconds=5.2, noise_sigma=0.15, seed=16, invert=True), 5
    else:
        eph = R.constellation()
        p = tmp_path / "brdc.nav"
        p.write_bytes(R.rinex_nav(eph))                                          # the orbit file tools/synth_rs92.py writes
        kw = dict(ephemeris=str(p))
        fl = R.flight(5, eph)
        a, b, frames = R.rs92_capture(fl, sr=SR, noise_sigma=0.01, seed=17), R.rs92_capture(fl, sr=SR, noise_sigma=0.12, seed=18), 5
    n = min(len(a), len(b)) // 2
    return [a[:2 * n], b[:2 * n], _noise(n, 19)], frames, kw


def _engine(kind, n_ch, max_frames=64):
    from radiosonde_auto_rx_amd.engine import Engine
    f = FAMILY[kind]
    return Engine([0.0] * n_ch, SR, sonde="generic", generic=f["generic"], thres=f["thres"], auto=f["auto"], keep_soft=True, lp_iq=True, max_chunk=SR // 2,
                  max_frames=max_frames)


def _good(kind, text):
    """the frame passed its checks, by the `-r -v` line"""
    if kind == "MEISEI":
        v = re.findall(r"#([0-9A-F]{6})#", text)
        return len(v) == 2 and not any(c in "EF" for c in "".join(v))
    return "[OK]" in text


@pytest.mark.parametrize("kind", F.KINDS)
def test_engine_with_the_device_decoder_equals_the_engine_with_the_host_tier(kind, tmp_path):
    caps, frames, dkw = _captures(kind, tmp_path)
    x = np.stack(caps)
    n = x.shape[1] // 2
    A, B = _engine(kind, 3), _engine(kind, 3)
    A.set_family(kind, ecc=1)
    opts = [dict(F.raw_opts(kind, 1)), dict(F.JSON[kind], **dkw)]
    mk = lambda: [[FamilyDecoder(kind, version="t", freq_khz=403000, **o) for o in opts] for _ in range(3)]      # noqa: E731  a decoder per channel and option set
    da, db = mk(), mk()
    ra, rb = [[] for _ in range(3)], [[] for _ in range(3)]
    for s0 in range(0, n, SR // 2):
        blk = np.ascontiguousarray(x[:, 2 * s0:2 * min(n, s0 + SR // 2)])
        A.process_host(blk); B.process_host(blk)
        for r in A.fetch_family():
            ra[r["channel"]].append((r["mv"], r["mv_pos"], r["nbits"], r["decoded"], [d.decoded(r) for d in da[r["channel"]]]))
        for h in B.fetch_hits():
            rb[h["channel"]].append((h["mv"], h["mv_pos"], h["nbits"], [d.hit(h) for d in db[h["channel"]]]))
    assert not A.overflowed() and not B.overflowed()
    A.close(); B.close()
    for c in range(3):
        assert [(a[0], a[1], a[2], a[4]) for a in ra[c]] == [(b[0], b[1], b[2], b[3]) for b in rb[c]], c
        assert all(a[3] == 1 and a[2] == F.NB[kind] for a in ra[c])             # no end of input here: every hit is whole and was decoded on the device
    good = sum(_good(kind, b[3][0]) for b in rb[0])
    assert good >= frames - 1, (good, frames, [b[3][0][-40:] for b in rb[0]])   # a condition on the input: the test cannot pass empty
    assert any(l.startswith("{") for a in ra[0] for l in a[4][1].splitlines())  # and JSON objects came out of the device's records
    if kind == "MTS01":                                                          # the inverted channel: a header of negative score, the stored bits flipped back on
        assert ra[1] and all(a[0] < 0 for a in ra[1]) and not any(_good(kind, a[4][0]) for a in ra[1])      # the device — read raw, as the reference reads them: no CRC


# ---------------------------------------------------------------- 3. ring and fetch edges (Meisei: the smallest shape at which the bookkeeping can go wrong)
@pytest.fixture(scope="module")
def meisei_iq():
    from tools import synth
    return synth.meisei_capture(sr=SR, seconds=5.2, noise_sigma=0.02, seed=21)


def _texts(dec, recs, how):
    return [(r["mv"], r["mv_pos"], r["nbits"], getattr(dec, how)(r)) for r in recs]


def test_ring_overflow_delivers_what_the_host_path_delivers(meisei_iq):
    A, B = _engine("MEISEI", 1, max_frames=4), _engine("MEISEI", 1, max_frames=4)
    A.set_family("MEISEI")
    n = len(meisei_iq) // 2
    for s0 in range(0, n, SR // 2):                                              # ten hits queued into a ring of four, no fetch in between
        blk = meisei_iq[2 * s0:2 * min(n, s0 + SR // 2)]
        A.process_host(blk); B.process_host(blk)
    ra, rb = A.fetch_family(), B.fetch_hits()
    assert A.overflowed() and B.overflowed() and len(ra) == len(rb) == 4
    da, db = FamilyDecoder("MEISEI", **F.raw_opts("MEISEI", 1)), FamilyDecoder("MEISEI", **F.raw_opts("MEISEI", 1))
    assert _texts(da, ra, "decoded") == _texts(db, rb, "hit") and all(r["decoded"] for r in ra)
    assert all(_good("MEISEI", da.decoded(r)) for r in ra)                      # (the last four frames of a clean signal: the comparison is not one of rubbish)
    A.close(); B.close()


def test_fetch_one_at_a_time_finish_and_the_switch_to_the_host_path(meisei_iq):
    A, B = _engine("MEISEI", 1, max_frames=16), _engine("MEISEI", 1, max_frames=16)
    A.set_family("MEISEI")
    da, db = FamilyDecoder("MEISEI", **F.raw_opts("MEISEI", 1)), FamilyDecoder("MEISEI", **F.raw_opts("MEISEI", 1))
    cut = [0, int(1.6 * SR), int(2.7 * SR), int(3.8 * SR), int(4.85 * SR)]

    def feed(k):
        blk = meisei_iq[2 * cut[k]:2 * cut[k + 1]]
        for s0 in range(0, len(blk) // 2, SR // 2):
            A.process_host(blk[2 * s0:2 * s0 + SR]); B.process_host(blk[2 * s0:2 * s0 + SR])

    # a fetch with max = 1, repeated: the rest stays queued, nothing is lost or doubled
    feed(0)
    ra = []
    while True:
        got = A.fetch_family(max_hits=1)
        assert len(got) <= 1
        if not got:
            break
        ra += got
    rb = B.fetch_hits()
    assert len(ra) == len(rb) >= 2 and _texts(da, ra, "decoded") == _texts(db, rb, "hit") and all(r["decoded"] for r in ra)
    assert len({r["mv_pos"] for r in ra}) == len(ra) and A.fetch_family() == []
    # device decoding switched off between fetches: the records that follow come undecoded and get the host decode, the same text
    A.set_device_ecc(False)
    feed(1)
    ra, rb = A.fetch_family(), B.fetch_hits()
    assert len(ra) == len(rb) >= 1 and all(r["decoded"] == 0 and len(r["soft"]) == 1152 for r in ra)
    assert _texts(da, ra, "decoded") == _texts(db, rb, "hit")
    # ... and on again: decoded on the device from the next record on; a record goes to whichever fetch takes it (here fetch_hits on the device engine)
    A.set_device_ecc(True)
    feed(2)
    ra, rb = A.fetch_hits(), B.fetch_hits()
    assert len(ra) == len(rb) >= 1 and _texts(da, ra, "hit") == _texts(db, rb, "hit") and A.fetch_family() == []
    # the end of input with a hit in progress: decoded = 0, fewer bits, and the fallback prints what the host path prints for the partial frame
    feed(3)
    ra, rb = A.fetch_family(finish=True), B.fetch_hits(finish=True)
    assert len(ra) == len(rb) >= 2
    assert [r["decoded"] for r in ra] == [1] * (len(ra) - 1) + [0] and 0 < ra[-1]["nbits"] < 1152 and len(ra[-1]["soft"]) == ra[-1]["nbits"] == rb[-1]["nbits"]
    assert _texts(da, ra, "decoded") == _texts(db, rb, "hit")
    assert not A.overflowed() and not B.overflowed()
    A.close(); B.close()


# ---------------------------------------------------------------- 4. refusals
def test_refusals():
    from radiosonde_auto_rx_amd.engine import Engine, MixedEngine, SondeError
    e = _engine("MEISEI", 1)
    with pytest.raises(SondeError):
        e.fetch_family()                                                         # without set_family
    with pytest.raises(SondeError):
        e.set_family("MTS01")                                                    # the engine's description has Meisei's nbits
    with pytest.raises(SondeError):
        e.set_family("LMS6")                                                     # not a kind of the device decoder
    e.set_family("MEISEI")
    with pytest.raises(SondeError):
        e.set_family("MEISEI")                                                   # once
    e.close()
    e = _engine("RS92", 1)
    with pytest.raises(SondeError):
        e.set_family("RS92", ecc=0)                                              # RS92 always corrects
    e.process_host(_noise(SR // 2, 3))
    with pytest.raises(SondeError):
        e.set_family("RS92")                                                     # after a process call
    e.close()
    e = Engine([0.0], SR, keep_soft=True, max_chunk=SR // 2)                     # a preset-type engine (RS41)
    with pytest.raises(SondeError):
        e.set_family("MEISEI")
    e.close()
    m = MixedEngine([0.0, 0.0], ["rs41", "dfm"], 2_400_000, max_chunk=240_000)
    with pytest.raises(SondeError):
        m.set_family("MEISEI")
    m.close()


# ---------------------------------------------------------------- 5. the receiver
def test_wideband_receiver_with_the_device_decoder_prints_the_same_objects():
    from tools import synth
    from radiosonde_auto_rx_amd.wideband import WidebandReceiver
    sr, cf, secs = 2_400_000, 403_000_000, 4.4
    n = int(sr * secs)
    sig = [("MEISEI", synth.snap_fq(0.125, sr), lambda fq: synth.meisei_capture(sr=sr, seconds=secs, fq=fq, noise_sigma=0.0, amp=0.25, seed=31)),
           ("IMET5", synth.snap_fq(-0.2, sr), lambda fq: synth.imet54_capture(sr=sr, seconds=secs, fq=fq, noise_sigma=0.0, amp=0.25, seed=32)),
           ("MTS01", synth.snap_fq(0.3, sr), lambda fq: synth.mts01_capture(sr=sr, seconds=secs, fq=fq, noise_sigma=0.0, amp=0.25, seed=33))]
    acc = np.random.default_rng(34).normal(0.0, 80.0, size=2 * n)
    for _, fq, make in sig:
        acc += make(fq).astype(np.float64)[:2 * n]
    iq = np.clip(np.round(acc), -32768, 32767).astype(np.int16)
    del acc
    outs = []
    for on in (False, True):
        rx = WidebandReceiver(sr, cfreq_hz=cf, raster_hz=1_000_000, version="t", device_family=on)      # (three raster points: the decoders are started by hand)
        for typ, fq, _ in sig:
            rx.add_channel(typ, fq)
        assert [bool(getattr(s["engine"], "device_family", False)) for s in rx.sondes] == [on] * 3
        out = []
        for s0 in range(0, n, rx.chunk):
            out += rx.push(iq[2 * s0:2 * min(n, s0 + rx.chunk)], finish=(s0 + rx.chunk >= n))
        rx.close()
        outs.append(out)
    assert outs[0] == outs[1]
    for typ in ("MEISEI", "IMET5", "MTS01"):
        assert sum(j["type"] == typ for j in outs[1]) >= 1, (typ, [j["type"] for j in outs[1]])
