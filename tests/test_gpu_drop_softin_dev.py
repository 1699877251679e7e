"""`rd94rd41drop --softin / --softinv [-i]` on the device (SoftinDev(kind="drop"), k_softin_drop): the consumer half of auto_rx's dropsonde
pipe `fsk_demod --cs16 -b -20000 -u 20000 -s --stats=N 2 48000 4800 - - | rd94rd41drop --json --softinv`, compared as text with the
reference pipe's stdout (goldens of tools/make_golden_drop.py):
 - alone: the signs of the reference modem's soft bits as +-1 floats in device memory through push_device, in calls of 63 .. 9616 bits;
 - behind the GPU modem: push_fsk, and the submit_fsk_behind / collect order with a second of signal per call;
 - the device's bytes and check masks of every frame against the host code, and the tallies of sonde_softin_dev_counts."""
import numpy as np
import pytest

from tests import drop_cases as cases
from tests.test_drop_fields import _printer

pytestmark = pytest.mark.gpu
SOFT = sorted(n for n, c in cases.CASES.items() if c["gen"].get("form") == "soft")


def _consumer(n_ch, argv):
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    return SoftinDev(n_ch, kind="drop", softinv="--softinv" in argv, inv="-i" in argv)


def _modem(n_ch, sr=48000):
    from radiosonde_auto_rx_amd.fsk import FskModem
    return FskModem(sr, 4800, n_channels=n_ch, P=10, nsym=50, lower=-20000, upper=20000, max_chunk=sr)       # fsk_demod's defaults: -p 10, --nsym 50


def _take(sf, printers, text, last):
    from radiosonde_auto_rx_amd import drop
    for f in sf.fetch_drop():
        assert (f["err94"], f["err41"]) == drop.errs(f["bytes"]) and f["complete"] and f["nraw"] == 2400
        assert f["sample"] > last[f["channel"]]
        last[f["channel"]] = f["sample"]
        text[f["channel"]] += printers[f["channel"]].frame(f["bytes"])


@pytest.mark.parametrize("name", SOFT)
def test_soft_streams_in_device_memory_equal_reference(name):
    import torch
    g = cases.load(name)
    s = g["soft_sign"].astype(np.float32)
    n, C = len(s), 3
    S = np.stack([s, s, np.concatenate([s[777:], -np.ones(777, np.float32)])])          # the third channel: the same stream 777 bits earlier
    d = torch.from_numpy(np.ascontiguousarray(S)).cuda()
    rng = np.random.default_rng(5)
    for argv, ref in zip(g["argv"], g["stdout"]):
        sf = _consumer(C, argv)
        printers, text, last = [_printer(argv) for _ in range(C)], [""] * C, [0] * C
        pos = 0
        while pos < n:
            k = min(int(rng.choice([9616, 63, 4800, 2401, 1000])), n - pos)
            chunk = d[:, pos:pos + k].contiguous()
            sf.push_device(chunk.data_ptr(), k, k)
            _take(sf, printers, text, last)
            pos += k
        c = sf.counts()
        sf.close()
        assert text[0].encode() == ref, (name, argv, text[0][-600:], ref[-600:])
        assert text[1] == text[0] and text[2] == text[0]
        if "-r" not in argv and "--json" in argv:
            assert c["ecc_ok"] == 3 * ref.count(b'"type"') and c["dropped"] == 0
        assert c["frames"] >= c["ecc_ok"]


@pytest.mark.parametrize("name", SOFT)
def test_modem_to_frames_on_the_device_equals_the_reference_pipe(name):
    """both halves of auto_rx's pipe on the device, a second of signal per call, against both halves of the reference on the same capture"""
    case, g = cases.CASES[name], cases.load(name)
    x = np.frombuffer(cases.capture(case), "<i2")
    sr = 48000
    X = np.stack([x, x])
    for argv, ref in zip(g["argv"], g["stdout"]):
        md, sf = _modem(2), _consumer(2, argv)
        printers, text, last = [_printer(argv) for _ in range(2)], [""] * 2, [0] * 2
        for s0 in range(0, X.shape[1] // 2, sr):
            md.process_host(X[:, 2 * s0:2 * (s0 + sr)])
            sf.push_fsk(md)
            _take(sf, printers, text, last)
        md.close(); sf.close()
        assert text[0].encode() == ref, (name, argv, text[0][-600:], ref[-600:])
        assert text[1] == text[0]


def test_decoder_submitted_behind_the_modems_next_second_gives_the_same_frames():
    """wait (k - 1), submit_device (k), collect (k - 2), submit_fsk_behind (k - 1): the golden's text again, and the same records as push_fsk"""
    import torch
    name, sr = "soft41", 48000
    g = cases.load(name)
    x = np.frombuffer(cases.capture(cases.CASES[name]), "<i2")
    X = torch.from_numpy(np.stack([x, x, x]).copy()).cuda()
    n = X.shape[1] // 2
    argv, ref = g["argv"][0], g["stdout"][0]
    assert argv == ["--json", "--softinv"] and ref.count(b'"type"') >= cases.N_FRAMES - 1

    def run(behind):
        md, sf = _modem(3), _consumer(3, argv)
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
            recs += sf.fetch_drop()
        if behind:
            md.wait(); sf.collect(); sf.submit_fsk_behind(md); sf.collect()
            recs += sf.fetch_drop()
        c = sf.counts()
        md.close(); sf.close()
        return recs, c

    plain, got = run(False), run(True)
    for recs, c in (plain, got):
        for ch in range(3):
            p = _printer(argv)
            text = "".join(p.frame(f["bytes"]) for f in recs if f["channel"] == ch)
            assert text.encode() == ref, (ch, text[-400:])
        assert c["ecc_ok"] == 3 * ref.count(b'"type"') and c["dropped"] == 0
    key = lambda f: (f["channel"], f["sample"])
    assert sorted(plain[0], key=key) == sorted(got[0], key=key)
