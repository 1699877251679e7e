"""k_mrz_hits on the device (radiosonde_auto_rx_amd/csrc/sonde_mrz_hits.hip): the per-hit decoder of generic engines carrying MRZ, which gives the CRC verdict under
both frame lengths and leaves the choice to the channel's host decoder.
1. the direct entry on the constructed hits of tests/test_mrz_hits_emu.py: records equal the CPU wave emulator's, field for field;
2. two engines on the same samples — one with set_family("MRZ") / fetch_family / FamilyDecoder.decoded, one with fetch_hits / FamilyDecoder.hit: text, mv, mv_pos and
   nbits per channel are identical, on an ECEF channel, a lat / lon channel (whose decoder goes over to 362 bits) and a noise channel (the arbiter is the host tier
   sonde_mrz_dec_frame on the same soft bits);
3. ring and fetch edges; 4. refusals; 5. the WidebandReceiver with device_family on and off.
Every comparison is byte for byte."""
import numpy as np
import pytest

import mrz_hits_cases as Z
from radiosonde_auto_rx_amd.family import FAMILY, FamilyDecoder, decode_mrz_hits_device

pytestmark = pytest.mark.gpu
SR = 48_000
K0 = 12                                                      # the captures start at sub-frame 12: serial numbers and date, which the JSON waits for, come first


# ---------------------------------------------------------------- 1. the direct entry against the emulator
def test_direct_entry_equals_the_emulator_field_for_field():
    emu = Z.load_emu()
    for _, ofs, hs in Z.sequences():
        reps = -(-300 // len(hs)) if ofs == 8 else 1                             # a few hundred hits in one launch
        softs = [h[1] for h in hs] * reps
        want, _ = Z.emu_run(emu, ofs, [h[1] for h in hs], None, grid=len(hs))    # (the direct entry has no header score: mv = 0)
        got = decode_mrz_hits_device(softs, bits_ofs=ofs)
        assert len(got) == len(softs)
        for i, r in enumerate(got):
            w = dict(want[i % len(hs)], channel=i)
            assert Z.rec_key(r) == Z.rec_key(w), (hs[i % len(hs)][0], i)
        assert sum(r["decoded"] for r in got) == reps * sum(len(h[1]) == Z.NB for h in hs) > 0
    assert decode_mrz_hits_device([]) == []


# ---------------------------------------------------------------- 2. two engines on the same samples
def _noise(n, seed, sigma=0.05):
    rng = np.random.default_rng(seed)
    return np.clip(np.round(rng.normal(0.0, sigma * 32767, 2 * n)), -32768, 32767).astype(np.int16)


def _engine(n_ch, max_frames=64, typ="MRZ"):
    from radiosonde_auto_rx_amd.engine import Engine
    f = FAMILY[typ]
    return Engine([0.0] * n_ch, SR, sonde="generic", generic=f["generic"], thres=f["thres"], auto=f["auto"], keep_soft=True, lp_iq=True, max_chunk=SR // 2,
                  max_frames=max_frames)


def _frame_bits(d):
    from radiosonde_auto_rx_amd.engine import lib
    return lib().sonde_mrz_dec_frame_bits(d._h)


def test_engine_with_the_device_decoder_equals_the_engine_with_the_host_tier():
    from tools import synth
    a = synth.mrz_capture(sr=SR, seconds=5.2, noise_sigma=0.02, seed=41, k0=K0)
    b = synth.mrz_capture(sr=SR, seconds=5.2, noise_sigma=0.12, seed=42, k0=K0, latlon=True)
    n = min(len(a), len(b)) // 2
    x = np.stack([a[:2 * n], b[:2 * n], _noise(n, 43)])
    A, B = _engine(3), _engine(3)
    A.set_family("MRZ")
    opts = [Z.RAW, Z.JSON]
    mk = lambda: [[FamilyDecoder("MRZ", version="t", freq_khz=403000, **o) for o in opts] for _ in range(3)]      # noqa: E731  a decoder per channel and option set
    da, db = mk(), mk()
    ra, rb = [[] for _ in range(3)], [[] for _ in range(3)]
    for s0 in range(0, n, SR // 2):
        blk = np.ascontiguousarray(x[:, 2 * s0:2 * min(n, s0 + SR // 2)])
        A.process_host(blk); B.process_host(blk)
        for r in A.fetch_family():
            ra[r["channel"]].append((r["mv"], r["mv_pos"], r["nbits"], r["decoded"], [d.decoded(r) for d in da[r["channel"]]]))
        for h in B.fetch_hits():
            at = _frame_bits(db[h["channel"]][0])                                # what the host tier reads of this hit
            rb[h["channel"]].append((h["mv"], h["mv_pos"], h["nbits"], [d.hit(h) for d in db[h["channel"]]], at))
    assert not A.overflowed() and not B.overflowed()
    A.close(); B.close()
    for c in range(3):
        print("channel", c, "hits", len(rb[c]), "[OK]", sum("[OK]" in t[3][0] for t in rb[c]), "read at", [t[4] for t in rb[c]])
        assert [(t[0], t[1], t[2], t[4]) for t in ra[c]] == [(t[0], t[1], t[2], t[3]) for t in rb[c]], c
        assert all(t[3] == 1 and t[2] == Z.NB for t in ra[c])                   # no end of input here: every hit is whole and was decoded on the device
        assert [_frame_bits(d) for d in da[c]] == [_frame_bits(d) for d in db[c]]
    # conditions on the input, from the host-tier engine: the test cannot pass empty
    for c in (0, 1):
        assert sum("[OK]" in t[3][0] for t in rb[c]) >= 3, (c, [t[3][0][-12:] for t in rb[c]])
    assert any(t[4] == 362 for t in rb[1])                                      # a hit printed while its decoder stood at 362 bits
    assert any(l.startswith("{") for t in ra[0] for l in t[4][1].splitlines())  # and a JSON object came out of the device's records


# ---------------------------------------------------------------- 3. ring and fetch edges
@pytest.fixture(scope="module")
def mrz_iq():
    from tools import synth
    return synth.mrz_capture(sr=SR, seconds=5.2, noise_sigma=0.02, seed=44)


def _texts(dec, recs, how):
    return [(r["mv"], r["mv_pos"], r["nbits"], getattr(dec, how)(r)) for r in recs]


def test_ring_overflow_delivers_what_the_host_path_delivers(mrz_iq):
    A, B = _engine(1, max_frames=4), _engine(1, max_frames=4)
    A.set_family("MRZ")
    n = len(mrz_iq) // 2
    for s0 in range(0, n, SR // 2):                                              # ten hits queued into a ring of four, no fetch in between
        blk = mrz_iq[2 * s0:2 * min(n, s0 + SR // 2)]
        A.process_host(blk); B.process_host(blk)
    ra, rb = A.fetch_family(), B.fetch_hits()
    assert A.overflowed() and B.overflowed() and len(ra) == len(rb) == 4
    da, db = FamilyDecoder("MRZ", **Z.RAW), FamilyDecoder("MRZ", **Z.RAW)
    assert _texts(da, ra, "decoded") == _texts(db, rb, "hit") and all(r["decoded"] for r in ra)
    assert all(r["v"][0] == 1 for r in ra)                                      # (the last four frames of a clean signal: the comparison is not one of rubbish)
    A.close(); B.close()


def test_fetch_one_at_a_time_finish_and_the_switch_to_the_host_path(mrz_iq):
    A, B = _engine(1, max_frames=16), _engine(1, max_frames=16)
    A.set_family("MRZ")
    da, db = FamilyDecoder("MRZ", **Z.RAW), FamilyDecoder("MRZ", **Z.RAW)
    cut = [0, int(1.8 * SR), int(2.8 * SR), int(3.8 * SR), int(4.5 * SR)]      # the last one inside the second copy of a frame

    def feed(k):
        blk = mrz_iq[2 * cut[k]:2 * cut[k + 1]]
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
    assert len(ra) == len(rb) >= 1 and all(r["decoded"] == 0 and len(r["soft"]) == Z.NB for r in ra)
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
    assert [r["decoded"] for r in ra] == [1] * (len(ra) - 1) + [0] and 0 < ra[-1]["nbits"] < Z.NB and len(ra[-1]["soft"]) == ra[-1]["nbits"] == rb[-1]["nbits"]
    assert _texts(da, ra, "decoded") == _texts(db, rb, "hit")
    assert not A.overflowed() and not B.overflowed()
    A.close(); B.close()


# ---------------------------------------------------------------- 4. refusals
def test_refusals():
    from radiosonde_auto_rx_amd.engine import MixedEngine, SondeError
    e = _engine(1, typ="MEISEI")
    with pytest.raises(SondeError):
        e.set_family("MRZ")                                                      # the engine's description has Meisei's nbits
    e.close()
    e = _engine(1)
    with pytest.raises(SondeError):
        e.set_family("LMS6")                                                     # still not a kind of the device decoder
    with pytest.raises(SondeError):
        e.set_family("MRZ", bits_ofs=65)
    with pytest.raises(SondeError):
        e.set_family("MRZ", bits_ofs=-1)
    e.set_family("MRZ", bits_ofs=64)
    with pytest.raises(SondeError):
        e.set_family("MRZ")                                                      # once
    e.close()
    e = _engine(1)
    e.process_host(_noise(SR // 2, 3))
    with pytest.raises(SondeError):
        e.set_family("MRZ")                                                      # after a process call
    e.close()
    m = MixedEngine([0.0, 0.0], ["rs41", "dfm"], 2_400_000, max_chunk=240_000)
    with pytest.raises(SondeError):
        m.set_family("MRZ")
    m.close()


# ---------------------------------------------------------------- 5. the receiver
def test_wideband_receiver_with_the_device_decoder_prints_the_same_objects():
    from tools import synth
    from radiosonde_auto_rx_amd.wideband import WidebandReceiver
    sr, cf, secs = 2_400_000, 403_000_000, 4.4
    n = int(sr * secs)
    fq = synth.snap_fq(0.125, sr)
    acc = np.random.default_rng(51).normal(0.0, 80.0, size=2 * n)
    acc += synth.mrz_capture(sr=sr, seconds=secs, fq=fq, noise_sigma=0.0, amp=0.25, seed=52, k0=K0).astype(np.float64)[:2 * n]
    iq = np.clip(np.round(acc), -32768, 32767).astype(np.int16)
    del acc
    outs = []
    for on in (False, True):
        rx = WidebandReceiver(sr, cfreq_hz=cf, raster_hz=1_000_000, version="t", device_family=on)      # (three raster points: the decoder is started by hand)
        rx.add_channel("MRZ", fq)
        assert [bool(getattr(s["engine"], "device_family", False)) for s in rx.sondes] == [on]
        out = []
        for s0 in range(0, n, rx.chunk):
            out += rx.push(iq[2 * s0:2 * min(n, s0 + rx.chunk)], finish=(s0 + rx.chunk >= n))
        rx.close()
        outs.append(out)
    assert outs[0] == outs[1]
    assert sum(j["type"] == "MRZ" for j in outs[1]) >= 1, [j["type"] for j in outs[1]]
