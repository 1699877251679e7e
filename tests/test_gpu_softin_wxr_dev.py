"""`weathex301d --softin [-i] [--pn9]` on the device (SoftinDev(kind="wxr"), k_softin_wxr): the consumer half of auto_rx's WxR-301D soft-bit pipe
`fsk_demod --cs16 -s -b -40000 -u 40000 --mask 50000 --stats=N 2 <96000|100000> <4800|5000> - - | weathex301d --softin -i --json [--pn9]`, compared as text with the
reference pipe's stdout (goldens of tools/make_golden_wxr.py and tools/make_golden_wxr_softin.py):
 - alone: the signs of the reference modem's soft bits as floats in device memory through push_device, in calls of 63 .. 9616 bits, three channels;
 - the synthetic streams of tests/wxr_softin_cases.py (damaged frames, zeros and NaNs, the ring behind a frame), one channel each;
 - behind the GPU modem: push_fsk, and the submit_fsk_behind / collect order with a second of signal per call.
The text is WxrPrinter.decoded on the device's records: bytes, PN9 and the check are not recomputed on the host."""
import numpy as np
import pytest

from tests import wxr_cases as cases
from tests import wxr_softin_cases as W

pytestmark = pytest.mark.gpu
SOFT = ["soft", "soft_pn9"]
SHIFT = 777


def _consumer(n_ch, argv, softinv=False):
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    o = W.opts_of(argv)
    return SoftinDev(n_ch, kind="wxr", softinv=softinv, wxr_opts=dict(pn9=o["pn9"], inv=o["inv"]))


def _printer(argv):
    from radiosonde_auto_rx_amd.wxr import WxrPrinter
    o = W.opts_of(argv)
    return WxrPrinter(raw=o["raw"], vbs=o["vbs"], json=o["json"], pn9=o["pn9"], version=W.VERSION, ts=o["ts"])


def _check(r, pn9):
    """a record against the serial model of its own bytes"""
    assert (r["x"], r["chkval"], r["chkdat"], r["chk_ok"], r["frid"], r["sn"], r["cnt"]) == W.verdict(r["raw"], pn9)


def _take(sf, printers, text, last, pn9, shift=()):
    for r in sf.fetch_wxr():
        _check(r, pn9)
        assert r["hdr_bit"] > last[r["channel"]]
        last[r["channel"]] = r["hdr_bit"]
        if r["channel"] in shift:                                # the same stream SHIFT bits earlier: -t prints the time in that stream
            r = dict(r, hdr_bit=r["hdr_bit"] + SHIFT)
        text[r["channel"]] += printers[r["channel"]].decoded(r)


def _push_in_calls(sf, d, n, rng, take):
    pos = 0
    while pos < n:
        k = min(int(rng.choice([9616, 63, 552, 2401, 1000])), n - pos)
        chunk = d[:, pos:pos + k].contiguous()
        sf.push_device(chunk.data_ptr(), k, k)
        take()
        pos += k


@pytest.mark.parametrize("name", SOFT)
def test_soft_streams_in_device_memory_equal_reference(name):
    import torch
    g = cases.load(name)
    s = g["soft_sign"].astype(np.float32)
    assert len(s) == (12950 if name == "soft_pn9" else 12850) and ((s == 0).sum() == 1) == (name == "soft_pn9")
    n, C = len(s), 3
    S = np.stack([s, s, np.concatenate([s[SHIFT:], np.ones(SHIFT, np.float32)])])           # the third channel: the same stream 777 bits earlier
    d = torch.from_numpy(np.ascontiguousarray(S)).cuda()
    rng = np.random.default_rng(5)
    for argv, ref in zip(g["argv"], g["stdout"]):
        o = W.opts_of(argv)
        sf = _consumer(C, argv)
        printers, text, last = [_printer(argv) for _ in range(C)], [""] * C, [0] * C
        _push_in_calls(sf, d, n, rng, lambda: _take(sf, printers, text, last, o["pn9"], shift=(2,)))
        c = sf.counts()
        sf.close()
        assert (text[0] + "\n").encode("latin-1") == ref, (name, argv, text[0][-600:], ref[-600:])
        assert text[1] == text[0] and text[2] == text[0]
        if o["inv"]:
            assert ref.count(b"[OK]") == (16 if o["raw"] else 8) and c["frames"] == 3 * 16 and c["ecc_ok"] == 3 * 16 and c["dropped"] == 0
            if o["json"]:
                assert ref.count(b'"type"') == 8
        else:
            assert ref == b"\n" and c["frames"] == 0                # the modem's polarity is the other one: nothing without -i


@pytest.mark.parametrize("name", W.GOLDEN_CASES)
def test_synthetic_streams_equal_recorded_reference(name):
    """the damaged streams (flips, flips_pn9) and every other stream of the emulator suite, one channel each, on the device"""
    import torch
    g = W.load_golden(name)
    s = g["soft"]
    d = torch.from_numpy(np.ascontiguousarray(s[None, :])).cuda()
    rng = np.random.default_rng(6)
    for argv, ref in zip(g["argv"], g["stdout"]):
        o = W.opts_of(argv)
        sf = _consumer(1, argv)
        printers, text, last = [_printer(argv)], [""], [0]
        _push_in_calls(sf, d, len(s), rng, lambda: _take(sf, printers, text, last, o["pn9"]))
        c = sf.counts()
        sf.close()
        assert (text[0] + "\n").encode("latin-1") == ref, (name, argv, text[0][-600:], ref[-600:])
        assert c["dropped"] == 0 and c["frames"] >= c["ecc_ok"]
        if o["raw"] == 1:
            assert (c["ecc_ok"], c["frames"] - c["ecc_ok"]) == (ref.count(b"[OK]"), ref.count(b"[NO]"))


@pytest.mark.parametrize("softinv,inv", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_invert_stream_xor_invert(softinv, inv):
    import torch
    g = W.load_golden("clean")
    s = g["soft"] if softinv == inv else -g["soft"]
    d = torch.from_numpy(np.ascontiguousarray(np.stack([s, -s]))).cuda()
    sf = _consumer(2, ["-i"] if inv else [], softinv=bool(softinv))
    sf.push_device(d.data_ptr(), len(s), len(s))
    recs = sf.fetch_wxr()
    sf.close()
    assert [r["channel"] for r in recs] == [0] * 4
    p = _printer(["--json"])
    assert ("".join(p.decoded(r) for r in recs) + "\n").encode() == g["stdout"][g["argv"].index(["--softin", "--json"])]


def test_record_cap_and_the_refusals_between_kinds():
    import ctypes as C
    import torch
    from radiosonde_auto_rx_amd.engine import SondeError, SONDE_WXR301
    from radiosonde_auto_rx_amd.fsk import SoftinDev, _lib
    assert SONDE_WXR301 == 301
    # 1 channel: 20 + 16 records a call; 40 frames back to back in one call lose 4, and the next call is intact
    first = W.cases()["back_to_back"]["s"]
    many = np.concatenate([first] * 8)
    nxt = W.cases()["header_in_payload"]["s"]
    d, d2 = torch.from_numpy(many).cuda(), torch.from_numpy(nxt).cuda()
    sf = _consumer(1, [])
    sf.push_device(d.data_ptr(), len(many), len(many))
    got = sf.fetch_wxr()
    assert len(got) == 36 and sf.counts()["dropped"] == 4 and [r["hdr_bit"] for r in got] == [39 + 552 * k for k in range(36)]
    sf.push_device(d2.data_ptr(), len(nxt), len(nxt))
    got = sf.fetch_wxr()
    assert [r["hdr_bit"] - len(many) for r in got] == W.cases()["header_in_payload"]["hb"] and sf.counts() == dict(frames=38, ecc_ok=38, repaired=0, symbols=0, dropped=4)
    with pytest.raises(SondeError):
        sf.fetch_drop()
    sf.close()
    other = SoftinDev(1, kind="drop")
    with pytest.raises(SondeError):
        other.fetch_wxr()
    other.close()
    h = C.c_void_p()
    assert _lib().sonde_softin_dev_create(1, SONDE_WXR301, 0, 0, 0, 0, C.byref(h)) == -1        # SONDE_E_ARG: the kind needs its options


# ---------------------------------------------------------------- behind the GPU modem
def _modem(n_ch, sr, baud):
    from radiosonde_auto_rx_amd.fsk import FskModem
    return FskModem(sr, baud, n_channels=n_ch, P=10, nsym=50, lower=-40000, upper=40000, mask=50000, max_chunk=sr)


@pytest.mark.parametrize("name", SOFT)
def test_modem_to_frames_on_the_device_equals_the_reference_pipe(name):
    """both halves of auto_rx's pipe on the device, a second of signal per call: push_fsk, then the wait / submit_device / collect / submit_fsk_behind order; both give
    the golden's text and the same records"""
    import torch
    case, g = cases.CASES[name], cases.load(name)
    sr, baud = (100000, 5000) if name == "soft_pn9" else (96000, 4800)
    x = np.frombuffer(cases.capture(case), "<i2")
    X = torch.from_numpy(np.stack([x, x]).copy()).cuda()
    n = X.shape[1] // 2
    argv, ref = g["argv"][0], g["stdout"][0]
    assert "-i" in argv and "--json" in argv and ref.count(b'"type"') == 8
    pn9 = W.opts_of(argv)["pn9"]

    def run(behind):
        md, sf = _modem(2, sr, baud), _consumer(2, argv)
        recs = []
        for s0 in range(0, n, sr):
            m = min(sr, n - s0)
            ptr = X.data_ptr() + 2 * s0 * X.element_size()
            if behind:
                if s0 > 0:
                    md.wait()
                md.submit_device(ptr, n, m)
                if s0 > 0:
                    sf.collect()
                    sf.submit_fsk_behind(md)
            else:
                md.process_device(ptr, n, m)
                sf.push_fsk(md)
            recs += sf.fetch_wxr()
        if behind:
            md.wait(); sf.collect(); sf.submit_fsk_behind(md); sf.collect()
            recs += sf.fetch_wxr()
        c = sf.counts()
        md.close(); sf.close()
        return recs, c

    plain, got = run(False), run(True)
    for recs, c in (plain, got):
        for ch in range(2):
            p = _printer(argv)
            mine = [r for r in recs if r["channel"] == ch]
            for r in mine:
                _check(r, pn9)
            text = "".join(p.decoded(r) for r in mine)
            assert (text + "\n").encode() == ref, (ch, text[-400:])
        assert c["ecc_ok"] == 2 * 16 and c["frames"] == 2 * 16 and c["dropped"] == 0
    key = lambda r: (r["channel"], r["hdr_bit"])
    assert sorted(plain[0], key=key) == sorted(got[0], key=key)
