"""GPU parity of the LMS6 / LMS-X soft-bit consumer on the device (include/sonde_fsk.h sonde_softin_dev_create_lms6 / _fetch_lms6: header search, block assembly
and the K = 7 Viterbi decoder of `lms6Xmod --softin --vit | --vit2` on one wavefront per channel, k_softin_lms6; RS(255,223), frame sync, CRC and text per
channel on the host) against the compiled reference decoder `oracle/_ref/lms6Xmod` on the same float32 soft-bit streams, and — fed by the modem — against the
reference's own pipe `fsk_demod -s | lms6Xmod --json --softin --vit2 -i` (auto_rx/autorx/decode.py:1200-1209).

A consumer has no `finish`: every stream here ends in noise long enough for the last block to complete and with no header in it, so the reference has nothing
in progress at EOF either and the two outputs must be equal; the slack of the other consumer tests (the last reference line may be missing) is all that is allowed."""
import os
import subprocess

import numpy as np
import pytest

import lms6_vit_model as M
from golden_cases import need_ref
from tools import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDIR = os.path.join(ROOT, "oracle", "_ref")
REF = os.path.join(REFDIR, "lms6Xmod")


def _soft(n_blocks, lmsx=False, sigma=0.0, seed=1, lead=37, invert=False):
    """as tests/test_lms6_native.py::_soft"""
    bits = synth.lms6_onair_bits(n_blocks, lmsx)
    s = 2.0 * bits.astype(np.float64) - 1.0
    rng = np.random.default_rng(seed)
    s = np.concatenate([rng.normal(0, 0.3, lead), s])
    s = s + rng.normal(0.0, sigma, len(s))
    if invert:
        s = -s
    return s.astype(np.float32)


def _stack(streams, seed):
    """channels of equal length: every stream followed by noise (no header in it) up to the longest + 200"""
    rng = np.random.default_rng(seed)
    n = max(len(s) for s in streams) + 200
    return np.stack([np.concatenate([s, rng.normal(0, 0.3, n - len(s)).astype(np.float32)]) for s in streams])


def _ref_lines(soft, args):
    r = subprocess.run([REF] + args, input=np.ascontiguousarray(soft, np.float32).tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-300:]
    return r.stdout.decode().splitlines()


def _run(S, rng, cuts=(301, 1000, 4800, 4097, 77, 9000), **kw):
    """the streams S [channels, n] from device memory through a consumer in calls of uneven length -> (lines per channel, records, counts)"""
    import torch
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    C, n = S.shape
    sf = SoftinDev(C, kind="lms6", **kw)
    d = torch.from_numpy(np.ascontiguousarray(S)).cuda()
    text = {c: "" for c in range(C)}
    recs = []
    pos = 0
    while pos < n:
        k = min(int(rng.choice(cuts)), n - pos)
        chunk = d[:, pos:pos + k].contiguous()
        sf.push_device(chunk.data_ptr(), k, k)
        for r in sf.fetch_lms6():
            text[r["channel"]] += r["text"]
            recs.append(r)
        pos += k
    cnt = sf.counts()
    sf.close()
    return {c: text[c].splitlines() for c in range(C)}, recs, cnt


def _same(got, ref):
    return got == ref or got == ref[:-1]


LMS6_STREAMS = None


def _lms6_streams():
    global LMS6_STREAMS
    if LMS6_STREAMS is None:
        LMS6_STREAMS = _stack([_soft(4), _soft(4, sigma=0.3, seed=2), _soft(4, sigma=0.3, seed=3, invert=True)], 11)
    return LMS6_STREAMS


@pytest.mark.parametrize("args,kw", [(["--vit", "--ecc", "-r"], dict(vit=1, ecc=1, raw=True)),
                                     (["--vit2", "--ecc"], dict(vit=2, ecc=1)),
                                     (["--json", "--vit2", "-i"], dict(json=True, vit=2, ecc=0, version="oracle"))], ids=lambda a: " ".join(a) if isinstance(a, list) else "")
def test_streams_in_device_memory_equal_reference_lms6xmod(args, kw):
    """3 channels x 4 blocks (clean, sigma 0.3, inverted), random call cuts; then the negated streams with --softinv"""
    need_ref()
    S = _lms6_streams()
    rng = np.random.default_rng(21)
    got, recs, cnt = _run(S, rng, **kw)
    for c in range(3):
        ref = _ref_lines(S[c], ["--softin"] + args)
        assert sum("[OK]" in l for l in ref) >= 3
        assert _same(got[c], ref), (c, got[c][:3], ref[:3])
    assert cnt["frames"] == len(recs) == 12 and cnt["dropped"] == 0 and cnt["ecc_ok"] >= 9
    assert all(r["type"] == 6 and r["blen"] == 261 and r["err"] == 0 for r in recs)
    hb = sorted(r["hdr_bit"] for r in recs if r["channel"] == 0)
    assert hb == [37 + 80 + 4160 * k for k in range(4)]                     # 64 header bits are bits 16 .. 79 of a block
    assert all((r["mv"] < -0.7) == (r["channel"] == 2) for r in recs)
    got2, _, _ = _run(-S, rng, softinv=True, **kw)
    assert got2 == got


def test_forced_lmsx():
    need_ref()
    S = _stack([_soft(3, lmsx=True, sigma=0.1, seed=4), _soft(3, lmsx=True, sigma=0.4, seed=5)], 12)
    got, recs, cnt = _run(S, np.random.default_rng(22), vit=2, ecc=1, typ=10)
    for c in range(2):
        ref = _ref_lines(S[c], ["--softin", "--vit2", "--ecc", "--lmsX"])
        assert sum("[OK]" in l for l in ref) >= 3
        assert _same(got[c], ref), (c, got[c][:3], ref[:3])
    assert all(r["type"] == 10 and r["blen"] == 300 for r in recs) and len(recs) == 6


def test_auto_detection_follows_the_host_decoder_block_by_block():
    """an LMS-X stream under auto detection (the first block is read as LMS6 and shows the LMS-X frame sync), and LMS6 -> LMS-X -> LMS6 in one stream:
    the length of every block is what the host decoder made of the one before it, whatever the cut of the calls"""
    need_ref()
    mixed = np.concatenate([_soft(3, sigma=0.2, seed=6), _soft(3, lmsx=True, sigma=0.2, seed=7, lead=16), _soft(4, sigma=0.2, seed=8, lead=0)])
    S = _stack([_soft(4, lmsx=True, sigma=0.2, seed=9), mixed], 13)
    for vit, flag in ((1, "--vit"), (2, "--vit2")):
        got, recs, cnt = _run(S, np.random.default_rng(23 + vit), vit=vit, ecc=1, typ=0)
        for c in range(2):
            ref = _ref_lines(S[c], ["--softin", flag, "--ecc"])
            assert sum("[OK]" in l for l in ref) >= 3
            assert _same(got[c], ref), (vit, c, got[c][:3], ref[:3])
        types = [r["type"] for r in recs if r["channel"] == 1]
        assert 6 in types and 10 in types and types[-1] == 6, types
        assert {r["type"] for r in recs if r["channel"] == 0} == {10}
        assert cnt["dropped"] == 0


def test_modem_to_text_on_the_device_equals_the_reference_pipe():
    """`fsk_demod --cs16 -b -10000 -u 10000 -s 2 48000 4800 | lms6Xmod --json --softin --vit2 -i` (decode.py:1200-1209): modem and consumer on the device
    (push_fsk), against both halves of the compiled reference; then the same seconds through submit_fsk / collect"""
    need_ref()
    from radiosonde_auto_rx_amd.fsk import FskModem, SoftinDev
    sr = 48_000
    x = synth.lms6_capture(sr=sr, seconds=5.0, noise_sigma=0.05, seed=81)
    rng = np.random.default_rng(82)
    tail = np.clip(np.round(rng.normal(0, 0.05 * 32767, 2 * int(1.5 * sr))), -32768, 32767).astype(np.int16)       # the last block completes in noise
    x = np.concatenate([x, tail])
    m = subprocess.run([os.path.join(REFDIR, "fsk_demod"), "--cs16", "-b", "-10000", "-u", "10000", "-s", "--stats=5", "2", "48000", "4800", "-", "-"],
                       input=x.tobytes(), capture_output=True, timeout=300)
    assert m.returncode == 0, m.stderr[-300:]
    r = subprocess.run([REF, "--json", "--softin", "--vit2", "-i"], input=m.stdout, capture_output=True, timeout=300)
    assert r.returncode == 0
    ref = r.stdout.decode().splitlines()
    assert sum('"type": "LMS"' in l for l in ref) >= 3
    X = np.stack([x, x])
    md = FskModem(sr, 4800, n_channels=2, P=10, lower=-10000, upper=10000, max_chunk=sr)       # (fsk_demod's default -p)
    kw = dict(kind="lms6", json=True, vit=2, ecc=0, version="oracle")
    sync, split = SoftinDev(2, **kw), SoftinDev(2, **kw)
    a, b = {0: "", 1: ""}, {0: "", 1: ""}
    for s0 in range(0, len(x) // 2, sr):
        md.process_host(X[:, 2 * s0:2 * (s0 + sr)])
        split.collect()                                       # (the second before)
        sync.push_fsk(md)
        split.submit_fsk(md)
        for f in sync.fetch_lms6():
            a[f["channel"]] += f["text"]
    split.collect()
    for f in split.fetch_lms6():
        b[f["channel"]] += f["text"]
    assert a[0] == a[1] and a == b
    assert _same(a[0].splitlines(), ref), (a[0][:300], ref[:3])
    md.close(); sync.close(); split.close()


def test_the_algebraic_decoder_alone_is_refused():
    from radiosonde_auto_rx_amd.engine import SondeError
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    with pytest.raises(SondeError, match=r"\(-1\)"):
        SoftinDev(1, kind="lms6", vit=0, ecc=1)
    SoftinDev(1, kind="lms6", vit=0, json=True).close()      # --json implies --vit (lms6Xmod.c:1153-1157)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# The decoder where it works (tests/lms6_vit_model.py, tests/test_softin_lms6_emu.py): streams whose noise the wave Viterbi has to correct, printed with -r and
# without --ecc — every frame line is the decoder's output as it stands, nothing repairs a survivor path that differs from the reference's.
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _model_recs(s, vit, typ, types):
    """(hdr_bit, mv > 0, blen, err) per block of the numpy model; types = the decoder's type after each block (the length of the next one)"""
    first = M.RAWBLKX if typ == 10 else M.RAWBLK6
    lens = [first] + [M.RAWBLKX if t == 10 else M.RAWBLK6 for t in types]
    out = []
    for hb, mv, raw in M.frame_stream(s, lambda k: lens[min(k, len(lens) - 1)] - M.BLOCKSTART):
        _, blen, err = M.decode_block(M.block_sb(raw, mv, vit))
        out.append((hb, bool(mv > 0), blen, err))
    return out


@pytest.mark.parametrize("vit", [1, 2])
@pytest.mark.parametrize("tn", list(M.NOISY_TYPES))
def test_noisy_streams_raw_text_equals_reference_and_records_equal_model(tn, vit):
    """four blocks per channel at sigma 0.7 (--vit), 0.9 (--vit2), on the 0.5 grid, with 15 % erasures, inverted; LMS6 forced, LMS-X forced, auto detection:
    the reference prints at least three frame lines of which at least three differ from the noiseless stream's; the device prints the same lines, and blen / err
    of every record are the model's"""
    need_ref()
    kinds = [k for k, (v, _) in M.NOISY_KINDS.items() if v == vit]
    built = [M.noisy_stream(tn, k) for k in kinds]
    typ = built[0][2]
    S = _stack([b[0] for b in built], 31)
    got, recs, cnt = _run(S, np.random.default_rng(40 + vit), vit=vit, ecc=0, raw=True, typ=typ)
    for c, (s, clean, _, _, ropt) in enumerate(built):
        ref, base = _ref_lines(S[c], ["--softin", "-r"] + ropt), _ref_lines(clean, ["--softin", "-r"] + ropt)
        assert len(ref) >= 3 and sum(l not in base for l in ref) >= 3, (kinds[c], len(ref))
        assert _same(got[c], ref), (kinds[c], len(got[c]), len(ref))
        mine = [r for r in recs if r["channel"] == c]
        assert [(r["hdr_bit"], r["mv"] > 0, r["blen"], r["err"]) for r in mine] == _model_recs(S[c], vit, typ, [r["type"] for r in mine]), kinds[c]
    assert cnt["dropped"] == 0


@pytest.mark.parametrize("call", [1, 63, 64, 65])
def test_calls_shorter_than_the_header_window(call):
    """one block in calls of 1, 63, 64 and 65 soft bits: the header window lies in the ring the channel keeps in device memory between calls"""
    need_ref()
    s, _, typ, vit, ropt = M.noisy_stream("lms6", "vit_s07", n_blocks=1)
    ref = _ref_lines(s, ["--softin", "-r"] + ropt)
    assert len(ref) >= 1
    got, recs, cnt = _run(s[None, :], np.random.default_rng(1), cuts=(call,), vit=vit, ecc=0, raw=True, typ=typ)
    assert _same(got[0], ref)
    assert [(r["hdr_bit"], r["mv"] > 0, r["blen"], r["err"]) for r in recs] == _model_recs(s, vit, typ, [6])


def test_header_at_the_threshold():
    """9 and 10 flips among the 64 header bits (0.71875 / 0.6875) and scores within 1e-3 of 0.7 on either side, both polarities, a channel each: the reference
    decides whether a block is found; the device agrees, with the header's bit index and the sign of the score"""
    need_ref()
    cases = [(n, inv) + M.threshold_stream(f, t, inv) for n, (f, t) in M.THRESHOLD_CASES.items() for inv in (False, True)]
    S = _stack([c[2] for c in cases], 32)
    got, recs, cnt = _run(S, np.random.default_rng(51), vit=1, ecc=0, raw=True, typ=6)
    found = 0
    for c, (name, inv, s, score, hdr_bit) in enumerate(cases):
        ref = _ref_lines(S[c], ["--softin", "-r", "--lms6", "--vit"])
        assert bool(ref) == (score > 0.7), (name, inv, score)
        assert _same(got[c], ref), (name, inv)
        mine = [(r["hdr_bit"], r["mv"] < 0) for r in recs if r["channel"] == c]
        assert mine == ([(hdr_bit, inv)] if ref else []), (name, inv, mine)
        found += bool(ref)
    assert found == 6 and cnt["frames"] == 6


def test_many_waves_in_one_launch():
    """320 channels (more than one wave per CU at 38.6 KB of LDS each) from 8 distinct noisy two-block streams, each channel behind its own lead of 0 .. 127 noise
    samples, pushed in uneven calls: every channel prints its stream's reference text, its headers are found `lead` bits later, nothing is dropped and the
    number of records is exact"""
    need_ref()
    kw = [dict(sigma=0.9, seed=301), dict(sigma=0.9, seed=302), dict(sigma=0.8, grid=True, seed=303), dict(sigma=0.8, grid=True, seed=304),
          dict(sigma=0.75, erase=0.15, seed=305), dict(sigma=0.75, erase=0.15, seed=306), dict(sigma=0.9, invert=True, seed=307), dict(sigma=0.7, seed=308)]
    base = [M.soft_stream(2, lead=0, **k) for k in kw]
    ref = [_ref_lines(b, ["--softin", "-r", "--lms6", "--vit2"]) for b in base]
    model = [_model_recs(b, 2, 6, [6]) for b in base]
    assert sum(len(r) for r in ref) >= 12 and all(len(m) >= 1 for m in model)
    rng = np.random.default_rng(33)
    C = 320
    leads = rng.permutation(np.arange(C) % 128)
    S = _stack([np.concatenate([rng.normal(0, 0.3, leads[c]).astype(np.float32), base[c % 8]]) for c in range(C)], 34)
    got, recs, cnt = _run(S, np.random.default_rng(35), vit=2, ecc=0, raw=True, typ=6)
    for c in range(C):
        assert _same(got[c], ref[c % 8]), (c, leads[c], len(got[c]), len(ref[c % 8]))
        mine = [(r["hdr_bit"], r["mv"] > 0, r["blen"], r["err"]) for r in recs if r["channel"] == c]
        assert mine == [(hb + int(leads[c]), p, bl, er) for hb, p, bl, er in model[c % 8]], (c, leads[c])
    assert cnt["dropped"] == 0 and cnt["frames"] == len(recs) == sum(len(model[c % 8]) for c in range(C))


def test_blocks_beyond_the_record_buffer_are_dropped_and_the_channel_goes_on():
    """the documented overflow: one channel holds 4 * 1 + 16 = 20 records a call.  22 blocks in one push_device call: 20 records with the reference's text for
    those blocks, two counted as dropped (decoded into the tail of the wave's LDS); three more blocks in the next call come back whole"""
    need_ref()
    import torch
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    lead = 37
    s = M.soft_stream(25, sigma=0.6, seed=60, lead=lead)
    ref = _ref_lines(s, ["--softin", "-r", "--lms6", "--vit"])
    assert len(ref) == 25 and sum(a != b for a, b in zip(ref, _ref_lines(M.soft_stream(25, seed=60, lead=lead), ["--softin", "-r", "--lms6", "--vit"]))) >= 3
    cut = lead + 22 * 4160 + 16                                  # block 22 is complete (its last 16 positions are the head of block 23), the header of block 23 is not
    d = torch.from_numpy(s).cuda()
    sf = SoftinDev(1, kind="lms6", vit=1, ecc=0, raw=True, typ=6)
    sf.push_device(d[:cut].contiguous().data_ptr(), cut, cut)
    a = sf.fetch_lms6()
    assert len(a) == 20 and sf.counts()["dropped"] == 2
    assert "".join(r["text"] for r in a).splitlines() == ref[:20]
    assert [r["hdr_bit"] for r in a] == [lead + 80 + 4160 * k for k in range(20)]
    rest = d[cut:].contiguous()
    sf.push_device(rest.data_ptr(), len(s) - cut, len(s) - cut)
    b = sf.fetch_lms6()
    assert [r["hdr_bit"] for r in b] == [lead + 80 + 4160 * k for k in (22, 23, 24)]
    assert "".join(r["text"] for r in b).splitlines() == ref[22:] and "[OK]" in b[-1]["text"] and b[-1]["text"].splitlines()[-1] == ref[-1]
    cnt = sf.counts()
    assert cnt["dropped"] == 2 and cnt["frames"] == 23
    sf.close()
