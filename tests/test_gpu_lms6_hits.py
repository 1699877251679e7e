"""k_lms6_hits on the device (radiosonde_auto_rx_amd/csrc/sonde_lms6_hits.hip): the per-hit decoder of generic engines carrying LMS6 / LMS-X — the raw-bit sign
alternation, the wave Viterbi, deconv and bits2bytes — whose block bytes the channel's host decoder takes from there (sonde_lms6_dec_block_bytes).
1. the direct entry on the constructed hits of tests/test_lms6_hits_emu.py: records equal the CPU wave emulator's, field for field, at both vit values;
2. two engines on the same samples — one with set_family("LMS6" | "LMSX") / fetch_family / FamilyDecoder.decoded, one with fetch_hits / FamilyDecoder.hit: text, mv,
   mv_pos and nbits per channel are identical, on a clean channel, a noisy one and a noise channel (the arbiter is the host tier sonde_lms6_dec_block on the same
   soft bits);
3. the device ECC switch; 4. refusals; 5. the WidebandReceiver with device_family on and off, also across the LMS6 -> LMS-X follow.
Every comparison is for equality."""
import ctypes as C

import numpy as np
import pytest

import lms6_hits_cases as Z
from radiosonde_auto_rx_amd.family import FAMILY, FamilyDecoder, FamilyHit, decode_lms6_hits_device

pytestmark = pytest.mark.gpu
SR = 48_000
RAW2 = dict(raw=1, ecc=1, vit=2, json=0)                      # `-r --ecc --vit2`: the engines decode with one vit, the receivers' 2


# ---------------------------------------------------------------- 1. the direct entry against the emulator
@pytest.mark.parametrize("vit", [1, 2])
def test_direct_entry_equals_the_emulator_field_for_field(vit):
    emu = Z.load_emu()
    for lmsx in (False, True):
        hs = Z.hits(lmsx)
        reps = 1 if lmsx else -(-150 // len(hs))                                 # about 150 hits in one launch
        want = Z.records(emu, lmsx, vit)
        got = decode_lms6_hits_device([h[1] for h in hs] * reps, [h[2] for h in hs] * reps, vit=vit, lmsx=lmsx)
        assert len(got) == reps * len(hs)
        for i, r in enumerate(got):
            w = dict(want[i % len(hs)], channel=i)
            assert Z.rec_key(r) == Z.rec_key(w), (hs[i % len(hs)][0], i)
        assert sum(r["decoded"] for r in got) == reps * (len(hs) - 1) > 0
    assert decode_lms6_hits_device([], [], vit=vit) == []


# ---------------------------------------------------------------- 2. two engines on the same samples
def _noise(n, seed, sigma=0.05):
    rng = np.random.default_rng(seed)
    return np.clip(np.round(rng.normal(0.0, sigma * 32767, 2 * n)), -32768, 32767).astype(np.int16)


def _engine(n_ch, max_frames=64, typ="LMS6"):
    from radiosonde_auto_rx_amd.engine import Engine
    f = FAMILY[typ]
    return Engine([0.0] * n_ch, SR, sonde="generic", generic=f["generic"], thres=f["thres"], auto=f["auto"], keep_soft=True, lp_iq=True, max_chunk=SR // 2,
                  max_frames=max_frames)


@pytest.mark.parametrize("typ", ["LMS6", "LMSX"])
def test_engine_with_the_device_decoder_equals_the_engine_with_the_host_tier(typ):
    from tools import synth
    kw = dict(lmsx=True, baud=4797.8) if typ == "LMSX" else {}
    a = synth.lms6_capture(sr=SR, seconds=5.2, noise_sigma=0.02, seed=61, **kw)
    b = synth.lms6_capture(sr=SR, seconds=5.2, noise_sigma=0.3, seed=62, **kw)
    n = min(len(a), len(b)) // 2
    x = np.stack([a[:2 * n], b[:2 * n], _noise(n, 63)])
    A, B = _engine(3, typ=typ), _engine(3, typ=typ)
    A.set_family(typ)
    opts = [RAW2, Z.JSON]
    mk = lambda: [[FamilyDecoder("LMS6", version="t", freq_khz=403000, **o) for o in opts] for _ in range(3)]      # noqa: E731  a decoder per channel and option set
    da, db = mk(), mk()                                                          # auto detection: on the LMS-X engine they start as LMS6 and find out
    ra, rb = [[] for _ in range(3)], [[] for _ in range(3)]
    long_for = lambda r: r["nbits"] > min(d.lms_block_bits() for d in da[r["channel"]])      # noqa: E731
    cuts = list(range(0, n, SR // 2))
    for s0 in cuts:
        blk = np.ascontiguousarray(x[:, 2 * s0:2 * min(n, s0 + SR // 2)])
        last = s0 == cuts[-1]
        A.process_host(blk); B.process_host(blk)
        for r in A.fetch_family(finish=last, need_soft=long_for):
            ra[r["channel"]].append((r["mv"], r["mv_pos"], r["nbits"], [d.decoded(r) for d in da[r["channel"]]], r["decoded"], "soft" in r))
        for h in B.fetch_hits(finish=last):
            rb[h["channel"]].append((h["mv"], h["mv_pos"], h["nbits"], [d.hit(h) for d in db[h["channel"]]]))
    assert not A.overflowed() and not B.overflowed()
    A.close(); B.close()
    nb = FAMILY[typ]["generic"]["nbits"]
    for c in range(3):
        print(typ, "channel", c, "hits", len(rb[c]), "[OK]", sum("[OK]" in t[3][0] for t in rb[c]), "decoded", [t[4] for t in ra[c]], "soft", [t[5] for t in ra[c]])
        assert [t[:4] for t in ra[c]] == rb[c], c
        assert all(t[4] == int(t[2] == nb) for t in ra[c])                      # whole hits were decoded on the device, the one of the end of input was not
        assert [d.lms_type() for d in da[c]] == [d.lms_type() for d in db[c]]
    # conditions on the input, from the host-tier engine: the test cannot pass empty
    assert sum("[OK]" in t[3][0] for t in rb[0]) >= 3, [t[3][0][-12:] for t in rb[0]]
    assert any(l.startswith("{") for t in ra[0] for l in t[3][1].splitlines())  # a JSON object came out of the device's records
    # the end of input: a record of fewer bits, not decoded, with its soft bits
    assert ra[0][-1][4] == 0 and ra[0][-1][5] and 0 < ra[0][-1][2] < nb
    assert sum(t[4] for t in ra[0]) >= 3 and not any(t[5] for t in ra[0][1:-1])  # the device's bytes were printed, not soft bits
    if typ == "LMSX":
        assert ra[0][0][5] and ra[0][0][4] == 1                                  # the first LMS-X block is longer than an LMS6 decoder reads: decoded from its soft bits
        assert da[0][0].lms_type()[0] == "LMSX"


# ---------------------------------------------------------------- 3. the device ECC switch, fetch_hits on such an engine
def _texts(dec, recs, how):
    return [(r["mv"], r["mv_pos"], r["nbits"], getattr(dec, how)(r)) for r in recs]


def test_the_switch_to_the_host_path_and_back():
    from tools import synth
    iq = synth.lms6_capture(sr=SR, seconds=5.0, noise_sigma=0.02, seed=64)
    A, B = _engine(1, max_frames=16), _engine(1, max_frames=16)
    A.set_family("LMS6", vit=1)
    da, db = FamilyDecoder("LMS6", **Z.RAW), FamilyDecoder("LMS6", **Z.RAW)      # --vit
    cut = [0, int(2.0 * SR), int(3.0 * SR), int(4.0 * SR), int(5.0 * SR)]

    def feed(k):
        blk = iq[2 * cut[k]:2 * cut[k + 1]]
        for s0 in range(0, len(blk) // 2, SR // 2):
            A.process_host(blk[2 * s0:2 * s0 + SR]); B.process_host(blk[2 * s0:2 * s0 + SR])

    feed(0)
    ra, rb = A.fetch_family(), B.fetch_hits()
    assert len(ra) == len(rb) >= 1 and all(r["decoded"] == 1 and r["vit"] == 1 and "soft" not in r for r in ra)
    assert _texts(da, ra, "decoded") == _texts(db, rb, "hit") and A.fetch_family() == []
    # device decoding switched off between records: the records that follow come undecoded and get the host decode, the same text
    A.set_device_ecc(False)
    feed(1)
    ra, rb = A.fetch_family(), B.fetch_hits()
    assert len(ra) == len(rb) >= 1 and all(r["decoded"] == 0 and r["blen"] == 0 and r["bytes"] == bytes(308) and len(r["soft"]) == Z.NB6 for r in ra)
    assert _texts(da, ra, "decoded") == _texts(db, rb, "hit")
    # ... and on again; a record goes to whichever fetch takes it (here fetch_hits on the device engine)
    A.set_device_ecc(True)
    feed(2)
    ra, rb = A.fetch_hits(), B.fetch_hits()
    assert len(ra) == len(rb) >= 1 and _texts(da, ra, "hit") == _texts(db, rb, "hit") and A.fetch_family() == []
    feed(3)
    ra, rb = A.fetch_family(finish=True), B.fetch_hits(finish=True)
    assert len(ra) == len(rb) >= 2 and [r["decoded"] for r in ra] == [1] * (len(ra) - 1) + [0]
    t = _texts(da, ra, "decoded")
    assert t == _texts(db, rb, "hit") and any("[OK]" in x[3] for x in t)
    assert not A.overflowed() and not B.overflowed()
    A.close(); B.close()


# ---------------------------------------------------------------- 4. refusals
def test_refusals():
    from radiosonde_auto_rx_amd.engine import MixedEngine, SondeError, lib
    e = _engine(1)
    for vit in (0, 3):
        with pytest.raises(SondeError):
            e.set_family("LMS6", vit=vit)
    with pytest.raises(SondeError):
        e.set_family("MEISEI")                                                   # the engine's description has LMS6's nbits
    f = lib().sonde_engine_set_family
    f.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    assert f(e._h, 6, 1) == -1                                                   # SONDE_LMS6 is not a kind of sonde_engine_set_family
    e.set_family("LMS6", vit=2)
    with pytest.raises(SondeError):
        e.set_family("LMS6")                                                     # once
    ff = lib().sonde_engine_fetch_family                                         # the old record type on an LMS engine
    ff.argtypes = [C.c_void_p, C.POINTER(FamilyHit), C.c_int32, C.c_int32]
    buf = (FamilyHit * 4)()
    assert ff(e._h, buf, 4, 0) == -1
    e.close()
    e = _engine(1, typ="MEISEI")
    with pytest.raises(SondeError):
        e.set_family("LMS6")                                                     # a Meisei engine
    with pytest.raises(SondeError):
        e.set_family("LMSX")
    e.close()
    e = _engine(1, typ="LMSX")
    e.process_host(_noise(SR // 2, 3))
    with pytest.raises(SondeError):
        e.set_family("LMSX")                                                     # after a process call
    e.close()
    m = MixedEngine([0.0, 0.0], ["rs41", "dfm"], 2_400_000, max_chunk=240_000)
    with pytest.raises(SondeError):
        m.set_family("LMS6")
    m.close()


# ---------------------------------------------------------------- 5. the receivers
def _receive(iq, sr, cf, fq, on):
    from radiosonde_auto_rx_amd.wideband import WidebandReceiver
    n = len(iq) // 2
    rx = WidebandReceiver(sr, cfreq_hz=cf, raster_hz=1_000_000, version="t", device_family=on)      # (three raster points: the decoder is started by hand)
    rx.add_channel("LMS6", fq)
    assert [bool(getattr(s["engine"], "device_family", False)) for s in rx.sondes] == [on]
    out = []
    for s0 in range(0, n, rx.chunk):
        out += rx.push(iq[2 * s0:2 * min(n, s0 + rx.chunk)], finish=(s0 + rx.chunk >= n))
    log = [e for e in rx.log if e["event"] == "retuned"]
    on_dev = [bool(getattr(s["engine"], "device_family", False)) for s in rx.sondes]
    rx.close()
    return out, log, on_dev


def test_wideband_receiver_with_the_device_decoder_prints_the_same_objects():
    from tools import synth
    sr, cf, secs = 2_400_000, 403_000_000, 4.4                                   # the stream of test_wideband_receiver_decodes_the_generic_family, the LMS6 alone
    n = int(sr * secs)
    fq = synth.snap_fq(0.125, sr)
    acc = synth.lms6_capture(sr=sr, seconds=secs, fq=fq, noise_sigma=0.0, amp=0.25, seed=95).astype(np.float64)[:2 * n]
    acc += np.random.default_rng(94).normal(0.0, 80.0, size=2 * n)
    iq = np.clip(np.round(acc), -32768, 32767).astype(np.int16)
    del acc
    off, on = _receive(iq, sr, cf, fq, False), _receive(iq, sr, cf, fq, True)
    assert off[0] == on[0] and off[1] == on[1] == []
    assert sum(j["type"] == "LMS" and j["id"] == "LMS6-8123456" for j in on[0]) >= 2, [j["id"] for j in on[0]]


def test_the_receiver_follows_an_lms6_that_turns_out_to_be_lmsx_with_the_device_decoder():
    from tools import synth
    sr, cf = 2_400_000, 403_000_000
    fq = synth.snap_fq((8 * sr / 64 + 900.0) / sr, sr)
    iq = synth.lms6_capture(sr=sr, seconds=6.6, fq=fq, noise_sigma=0.004, amp=0.25, seed=31, baud=4797.8, lmsx=True)
    off, on = _receive(iq, sr, cf, fq, False), _receive(iq, sr, cf, fq, True)
    assert off[0] == on[0] and off[1] == on[1]
    assert [e["type"] for e in on[1]] == ["LMSX"] and on[2] == [True]           # the engine the sonde moved to decodes on the device as well
    assert sum(j["id"] == "LMSX-8123456" for j in on[0]) >= 3, [j["id"] for j in on[0]]
