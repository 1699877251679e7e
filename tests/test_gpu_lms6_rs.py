"""k_lms6_rs on the device (radiosonde_auto_rx_amd/csrc/sonde_lms6_rs.hip): RS(255,223) of LMS6 / LMS-X blocks, one wavefront per block record, under each
hypothesis the channel's host decoder can ask for (sonde_lms6_rs_t), which that decoder then takes instead of decoding (sonde_lms6_dec_block_rs).
1. the direct entry on the word cases (embedded at offset 5) and the block cases of tests/lms6_rs_cases.py: records equal the CPU wave emulator's byte for byte;
2. a generic LMS6 engine and an LMS-X engine with set_family(.., rs=True) beside one without: the same hits, RS records equal to the model (the compiled
   reference's rs_decode plus frmsync_X), the same text, no host fallback;
3. entry preconditions; 4. the soft-bit consumer with lms6_rs on and off: the same text per channel.
Every comparison is for equality."""
import ctypes as C

import numpy as np
import pytest

import lms6_hits_cases as Z
import lms6_rs_cases as R
from radiosonde_auto_rx_amd.family import FAMILY, FamilyDecoder, Lms6Hit, Lms6Rs, decode_lms6_rs_device

pytestmark = pytest.mark.gpu
SR = 48_000
RAW2 = dict(raw=1, ecc=1, vit=2, json=0)


# ---------------------------------------------------------------- 1. the direct entry against the emulator
_all = []


def all_records():
    """every word case as a block and every block case -> [(name, bytes, blen)], and the emulator's records of them (one emulated launch, computed once)"""
    if not _all:
        cases = [(n, *R.word_block(w)) for n, w, _ in R.word_cases()] + [(n, b, blen) for n, b, blen, dec in R.block_cases() if dec]
        want, _ = R.emu_records(R.load_emu(), [c[1] for c in cases], [c[2] for c in cases], grid=4)
        _all.append((cases, want))
    return _all[0]


@pytest.mark.parametrize("n", [1, 3, 65, None])
def test_direct_entry_equals_the_emulator_byte_for_byte(n):
    cases, want = all_records()
    cases, want = cases[-n:] if n else cases, want[-n:] if n else want      # (the block cases are at the end)
    assert len(cases) == (n or len(cases)) and (n is not None or len(cases) >= 300)
    got = decode_lms6_rs_device([c[1] for c in cases], [c[2] for c in cases])
    assert len(got) == len(cases)
    for c, g, w in zip(cases, got, want):
        assert R.rs_bytes(g) == R.rs_bytes(w), c[0]
    if n is None:
        assert sum(g.h6.err > 0 for g in got) >= 100 and sum(g.h6.err < 0 for g in got) >= 100 and sum(g.h6X.at >= 0 for g in got) >= 100


def test_direct_entry_checks_its_arguments_and_a_zero_length_block():
    from radiosonde_auto_rx_amd.engine import lib
    assert decode_lms6_rs_device([], []) == []
    got = decode_lms6_rs_device([bytes(308), R.block_cases()[1][1]], [0, 260])
    assert R.rs_bytes(got[0]) == bytes(120) and got[1].h6.err == 3
    fn = lib().sonde_lms6_rs_device
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.POINTER(Lms6Rs)]
    by, bl, out = np.zeros((2, 308), np.uint8), np.array([260, 301], np.int32), (Lms6Rs * 2)()
    assert fn(by.ctypes.data, 308, bl.ctypes.data, 2, out) == -1                 # blen beyond a block
    assert fn(by.ctypes.data, 307, bl.ctypes.data, 1, out) == -1                 # a stride shorter than a record
    assert fn(None, 308, bl.ctypes.data, 1, out) == -1 and fn(by.ctypes.data, 308, bl.ctypes.data, -1, out) == -1


# ---------------------------------------------------------------- 2. two engines on the same samples
def _engine(n_ch, max_frames=64, typ="LMS6"):
    from radiosonde_auto_rx_amd.engine import Engine
    f = FAMILY[typ]
    return Engine([0.0] * n_ch, SR, sonde="generic", generic=f["generic"], thres=f["thres"], auto=f["auto"], keep_soft=True, lp_iq=True, max_chunk=SR // 2,
                  max_frames=max_frames)


@pytest.mark.parametrize("typ", ["LMS6", "LMSX"])
def test_engine_with_device_rs_equals_the_engine_without(typ):
    from tools import synth
    kw = dict(lmsx=True, baud=4797.8) if typ == "LMSX" else {}
    a = synth.lms6_capture(sr=SR, seconds=4.2, noise_sigma=0.02, seed=61, **kw)
    b = synth.lms6_capture(sr=SR, seconds=4.2, noise_sigma=0.3, seed=62, **kw)
    n = min(len(a), len(b)) // 2
    x = np.stack([a[:2 * n], b[:2 * n]])
    A, B = _engine(2, typ=typ), _engine(2, typ=typ)
    A.set_family(typ, rs=True); B.set_family(typ)
    mk = lambda: [FamilyDecoder("LMS6", version="t", freq_khz=403000, **RAW2) for _ in range(2)]      # noqa: E731  auto detection, a decoder per channel
    da, db = mk(), mk()
    ta, tb = [[] for _ in range(2)], [[] for _ in range(2)]
    n_rs = 0
    cuts = list(range(0, n, SR // 2))
    for s0 in cuts:
        blk = np.ascontiguousarray(x[:, 2 * s0:2 * min(n, s0 + SR // 2)])
        last = s0 == cuts[-1]
        A.process_host(blk); B.process_host(blk)
        long_for = lambda r: r["nbits"] > da[r["channel"]].lms_block_bits()      # noqa: E731
        ra, rb = A.fetch_family(finish=last, need_soft=long_for), B.fetch_family(finish=last, need_soft=long_for)
        assert len(ra) == len(rb)
        order = lambda r: (r["channel"], r["mv_pos"])                            # noqa: E731  (channels interleave as their frame syncs finish)
        for p, q in zip(sorted(ra, key=order), sorted(rb, key=order)):
            assert Z.rec_key(p) == Z.rec_key(q)                                  # hits[] is what the engine without the switch returns
            assert R.rs_bytes(p["rs"]) == R.rs_bytes(R.model_record(p["bytes"], p["blen"], p["decoded"])), (p["channel"], p["mv_pos"])
            n_rs += p["rs"].h6.at == 5
            c = p["channel"]
            ta[c].append(da[c].decoded(p))                                       # the record's "rs" goes to sonde_lms6_dec_block_rs
            tb[c].append(db[c].decoded(q))
    assert not A.overflowed() and not B.overflowed()
    A.close(); B.close()
    assert ta == tb and n_rs >= 4
    assert sum("[OK]" in t for t in ta[0]) >= 2, [t[-12:] for t in ta[0]]
    stats = [d.lms_rs_stats() for d in da]
    print(typ, "rs records", n_rs, "used / missed per channel", stats)
    assert all(m == 0 for _, m in stats) and stats[0][0] > 0
    assert all(d.lms_rs_stats() == (0, 0) for d in db)
    if typ == "LMSX":
        assert da[0].lms_type()[0] == "LMSX"


# ---------------------------------------------------------------- 3. entry preconditions
def _noise(n, seed, sigma=0.05):
    rng = np.random.default_rng(seed)
    return np.clip(np.round(rng.normal(0.0, sigma * 32767, 2 * n)), -32768, 32767).astype(np.int16)


def test_entry_preconditions():
    from radiosonde_auto_rx_amd.engine import SondeError, lib
    f = lib().sonde_engine_set_family_lms6_rs
    f.argtypes = [C.c_void_p, C.c_int32]
    e = _engine(1)
    assert f(e._h, 1) == -1                                                      # before sonde_engine_set_family_lms6
    e.set_family("LMS6", vit=1)
    assert f(e._h, 1) == 0 and f(e._h, 0) == 0 and f(e._h, 1) == 0
    e.process_host(_noise(SR // 2, 3))
    assert f(e._h, 1) == -1 and f(e._h, 0) == -1                                 # after the first process call
    # sonde_engine_fetch_family_lms6 is unchanged with the switch on; the fetch with records wants a place for them
    ff = lib().sonde_engine_fetch_family_lms6
    ff.argtypes = [C.c_void_p, C.POINTER(Lms6Hit), C.c_int32, C.c_int32]
    buf = (Lms6Hit * 4)()
    assert ff(e._h, buf, 4, 0) == 0
    fr = lib().sonde_engine_fetch_family_lms6_rs
    fr.argtypes = [C.c_void_p, C.POINTER(Lms6Hit), C.POINTER(Lms6Rs), C.c_int32, C.c_int32]
    assert fr(e._h, buf, None, 4, 0) == -1
    e.close()
    e = _engine(1, typ="MEISEI")
    e.set_family("MEISEI")
    assert f(e._h, 1) == -1                                                      # not an LMS6 engine
    with pytest.raises(SondeError):
        e.set_family("MEISEI", rs=True)
    e.close()
    assert f(None, 1) == -1


def test_fetch_family_lms6_is_unchanged_with_the_switch_on_and_rs_is_zero_with_it_off():
    from tools import synth
    from radiosonde_auto_rx_amd.engine import lib
    iq = synth.lms6_capture(sr=SR, seconds=2.6, noise_sigma=0.02, seed=64)
    A, B, D = _engine(1, max_frames=16), _engine(1, max_frames=16), _engine(1, max_frames=16)
    A.set_family("LMS6", vit=1, rs=True); B.set_family("LMS6", vit=1); D.set_family("LMS6", vit=1)
    A._family_lms_rs = False                                                     # the plain fetch on the engine with the switch on
    D._family_lms_rs = True                                                      # the fetch with records on an engine with the switch off
    ra, rb, rd = [], [], []
    for s0 in range(0, len(iq) // 2, SR // 2):
        for E_, out in ((A, ra), (B, rb), (D, rd)):
            E_.process_host(iq[2 * s0:2 * s0 + SR])
            out += E_.fetch_family()
    assert len(ra) == len(rb) == len(rd) >= 2
    assert [Z.rec_key(r) for r in ra] == [Z.rec_key(r) for r in rb] == [Z.rec_key(r) for r in rd]
    assert all("rs" not in r for r in ra) and all(R.rs_bytes(r["rs"]) == bytes(120) for r in rd)
    A.close(); B.close(); D.close()


# ---------------------------------------------------------------- 4. the soft-bit consumer
def _consume(S, seed, **kw):
    """the streams S [channels, n] from device memory through a consumer in calls of uneven length -> (text per channel, (used, missed))"""
    import torch
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    rng = np.random.default_rng(seed)
    nch, n = S.shape
    sf = SoftinDev(nch, kind="lms6", **kw)
    d = torch.from_numpy(np.ascontiguousarray(S)).cuda()
    text = {c: "" for c in range(nch)}
    pos = 0
    while pos < n:
        k = min(int(rng.choice((301, 1000, 4800, 4097, 77, 9000))), n - pos)
        chunk = d[:, pos:pos + k].contiguous()
        sf.push_device(chunk.data_ptr(), k, k)
        for r in sf.fetch_lms6():
            text[r["channel"]] += r["text"]
        pos += k
    st = sf.lms6_rs_stats()
    sf.close()
    return text, st


@pytest.mark.parametrize("name", ["lms6_fixed", "lmsx_fixed", "auto"])
def test_consumer_with_device_rs_prints_what_it_prints_without(name):
    from test_gpu_softin_lms6 import _soft, _stack
    if name == "lms6_fixed":
        S, kw = _stack([_soft(3), _soft(3, sigma=0.3, seed=2), _soft(3, sigma=0.3, seed=3, invert=True)], 11), dict(vit=2, ecc=1, typ=6)
    elif name == "lmsx_fixed":
        S, kw = _stack([_soft(3, lmsx=True, sigma=0.1, seed=4), _soft(3, lmsx=True, sigma=0.4, seed=5)], 12), dict(vit=2, ecc=1, typ=10)
    else:
        mixed = np.concatenate([_soft(2, sigma=0.2, seed=6), _soft(3, lmsx=True, sigma=0.2, seed=7, lead=16), _soft(3, sigma=0.2, seed=8, lead=0)])
        S, kw = _stack([_soft(3, lmsx=True, sigma=0.2, seed=9), mixed], 13), dict(vit=2, ecc=1, typ=0)
    off, st_off = _consume(S, 21, **kw)
    on, st_on = _consume(S, 21, lms6_rs=True, **kw)
    assert on == off
    assert all(sum("[OK]" in l for l in off[c].splitlines()) >= 2 for c in off), {c: off[c][-40:] for c in off}
    print(name, "used / missed", st_on)
    assert st_off == (0, 0) and st_on[0] > 0 and st_on[1] == 0
