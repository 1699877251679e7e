"""iMet-4 in the channelized receiver (wideband.py, ChannelizedReceiver): one 2.4 Msps stream, M = 64, D = 48 (50 kHz channels 37.5 kHz apart)
with an iMet-4 and an RS41.  The iMet JSON objects are those the compiled reference prints on the same channelizer channel's float32 samples
(`imet4iq --iq <offset> --lpIQ --dc --json - 50000 32`): with the start given by add_channel, and with the scanner finding the sonde by
itself (1.5 kHz off its channel's centre; at the 6 kHz of the known-start stream the scanner names nothing: an expected failure).  An
iMet-1-RS detection in a 50 kHz channel, and an iMet-4 at a channel rate imet4iq would decimate, are logged once as not decodable and start
nothing; an idle slot goes back to the pool."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "imet4iq")
SR, M, D = 2_400_000, 64, 48
SPACING = SR / M
SECS = 8.0
CF = 403_000_000
F_IMET = 9 * SPACING + 6000.0
F_NEAR = 9 * SPACING + 1500.0                # an iMet-4 the scanner can name: inside its capture range of about 3 kHz
F_RS41 = -20 * SPACING - 1500.0


@functools.lru_cache(maxsize=None)
def _stream(f_imet=F_IMET):
    from tools import synth
    n = int(SR * SECS)
    acc = np.zeros(2 * n, np.float64)
    x = synth.imet4_capture(sr=SR, seconds=SECS, fq=f_imet / SR, seed=61, noise_sigma=0.0, amp=0.2)
    acc[:len(x)] += x[:2 * n]
    x = synth.rs41_capture(sr=SR, seconds=SECS, fq=F_RS41 / SR, seed=62, noise_sigma=0.0, amp=0.2, sonde_id="N3333333", t_first=0.2,
                           frame_kw=dict(ecef_cm=(418833319, 85974133, 473346430)))
    acc[:len(x)] += x[:2 * n]
    acc += np.random.default_rng(63).normal(0.0, 60.0, size=2 * n)
    iq = np.clip(np.round(acc), -32768, 32767).astype(np.int16)
    iq.setflags(write=False)
    return iq


def _receive(add, f_imet=F_IMET):
    from radiosonde_auto_rx_amd.wideband import ChannelizedReceiver
    iq = _stream(f_imet)
    n = len(iq) // 2
    rx = ChannelizedReceiver(SR, M=M, D=D, cfreq_hz=CF, slots=2, version="oracle")
    assert rx.if_sr == 50000
    if add:
        rx.add_channel("IMET4", F_IMET)
    out = []
    for s0 in range(0, n, rx.chunk):
        out += rx.push(iq[2 * s0:2 * min(n, s0 + rx.chunk)], finish=(s0 + rx.chunk >= n))
    res = dict(out=out, log=list(rx.log), chunk=rx.chunk, sondes=[dict(type=s["type"], f_hz=s["f_hz"], chan=s["chan"], frames=s["frames"]) for s in rx.sondes])
    rx.close()
    return res


@functools.lru_cache(maxsize=None)
def _channel_samples(k, chunk, f_imet=F_IMET):
    """channel k of the stream through a second channelizer, in the receiver's blocks: float32 IQ"""
    import torch
    from radiosonde_auto_rx_amd.chan import Channelizer
    iq = _stream(f_imet)
    n = len(iq) // 2
    ch = Channelizer(SR, M, D, 16, max_chunk=chunk)
    total = n // D + ch.max_frames
    buf = torch.zeros(M, total, 2, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    got = 0
    for pos in range(0, n - n % D, chunk):
        take = min(chunk, n - n % D - pos)
        got += ch.process_host(iq[2 * pos:2 * (pos + take)], buf.data_ptr() + 8 * got, total)
    ch.sync()
    y = np.ascontiguousarray(buf[k, :got].cpu().numpy()).astype(np.float32)
    assert int(ch.out_rate) == 50000 and abs(ch.channel_freq(k) - _chan_freq(k)) < 1e-6
    ch.close()
    return y


def _chan_freq(k):
    return (k if k < M // 2 else k - M) * SPACING


def _reference(y, resid):
    if not os.path.exists(REF):
        pytest.fail("oracle/_ref/imet4iq missing: build it where the reference lies (make -C oracle ref)")
    r = subprocess.run([REF, "--iq", repr(resid), "--lpIQ", "--dc", "--json", "-", "50000", "32"], input=y.tobytes(), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-300:]
    return [json.loads(l) for l in r.stdout.decode("latin-1").split("\n") if l.startswith("{")]


def _without_freq(j):
    return {k: v for k, v in j.items() if k != "freq"}


def test_receiver_known_start_prints_the_references_objects():
    r = _receive(add=True)
    started = [e for e in r["log"] if e["event"] == "detected" and e["type"] == "IMET4"]
    assert len(started) == 1 and started[0]["if_sample"] == 0 and started[0]["channel"] == 9, r["log"]
    resid = (started[0]["f_hz"] - 9 * SPACING) / 50000
    assert abs(resid - 0.12) < 1e-12
    ref = _reference(_channel_samples(9, r["chunk"]), resid)
    assert len(ref) >= 5, len(ref)
    imet = [j for j in r["out"] if j["type"] == "IMET"]
    assert [_without_freq(j) for j in imet] == ref, (len(imet), len(ref))
    assert all("freq" not in j for j in ref)
    assert all(j["freq"] == int(round((CF + F_IMET) / 1000.0)) for j in imet), imet[0]
    assert sum(s["frames"] for s in r["sondes"] if s["type"] == "RS41") >= 3, r["log"]


@pytest.mark.xfail(strict=True, reason="the scanner names no iMet-4 that sits 6 kHz off its channel's centre: over the 8 s of this stream its only lines are "
                   "'RS41: 0.9871 , -1768.0Hz' ... 'RS41: 0.9935 , -1612.2Hz' (one per second, channel 44) and none for channel 9.  It is the detector's "
                   "capture range, not the 50 kHz IF: the compiled reference `dft_detect --iq --dc - <sr> 32` on a clean iMet-4 prints "
                   "'IMET4: 0.9949 , +1.7Hz' at 50 kHz and 0 Hz offset, 'IMET4: 0.9360 , +3000.4Hz' at 3 kHz, and nothing at 6 kHz, at 48 kHz as at 50 kHz")
def test_receiver_told_nothing_finds_and_decodes_the_imet4():
    """(the stream and the 6 kHz offset are the ones the known-start test uses; see the reason above for what the scanner says)"""
    _told_nothing(F_IMET)


def test_receiver_told_nothing_decodes_an_imet4_inside_the_scanners_range():
    """the same stream with the iMet-4 1.5 kHz off its channel's centre: the scanner names it, its offset reaches `--iq` with the right sign
    (the frequency is the sonde's, and the objects are the reference's when it is started at the logged block with the logged offset)"""
    _told_nothing(F_NEAR)


def _told_nothing(f_imet):
    r = _receive(add=False, f_imet=f_imet)
    assert sorted(s["type"] for s in r["sondes"]) == ["IMET4", "RS41"], [e for e in r["log"] if e["event"] != "released"]
    s = [s for s in r["sondes"] if s["type"] == "IMET4"][0]
    assert abs(s["f_hz"] - f_imet) < 600.0, s
    started = [e for e in r["log"] if e["event"] == "detected" and e["type"] == "IMET4"][0]
    k = started["channel"]
    resid = (started["f_hz"] - _chan_freq(k)) / 50000
    y = _channel_samples(k, r["chunk"], f_imet)
    ref = {j["frame"]: j for j in _reference(y[started["if_sample"]:], resid)}
    imet = [j for j in r["out"] if j["type"] == "IMET"]
    assert len(imet) >= 3, (len(imet), started)
    for j in imet:
        assert j["frame"] in ref and _without_freq(j) == ref[j["frame"]], (j, ref.get(j["frame"]))
    assert len(imet) == len(ref)


def test_imet1rs_in_a_50_khz_channel_is_logged_once_and_starts_nothing():
    from radiosonde_auto_rx_amd.wideband import ChannelizedReceiver
    rx = ChannelizedReceiver(SR, M=M, D=D, cfreq_hz=CF, slots=2, chunk=48000, version="oracle")
    for _ in range(3):                                        # the scanner names a sonde again and again while nothing decodes it
        rx._on_detection(dict(type="IMET1RS", channel=9, df=0.12, score=1.0))
    rx._on_detection(dict(type="IMET1RS", channel=10, df=-0.63, score=1.0))     # the same sonde seen from the neighbouring channel
    log, groups, sondes = list(rx.log), dict(rx.groups), list(rx.sondes)
    rx.close()
    assert [e["event"] for e in log] == ["not decodable at this channel rate"], log
    assert log[0]["type"] == "IMET1RS" and abs(log[0]["f_hz"] - F_IMET) < 1e-6
    assert groups == {} and sondes == []


def test_idle_imet_slot_goes_back_to_the_pool():
    """a slot that prints no JSON object for idle_s is released (sonde_imet4_release_channel) and serves the next start"""
    from radiosonde_auto_rx_amd.wideband import ChannelizedReceiver
    rx = ChannelizedReceiver(SR, M=M, D=D, cfreq_hz=CF, slots=1, chunk=240000, idle_s=0.25, version="oracle")
    rx.add_channel("IMET4", F_IMET)
    eng = rx.groups["IMET4"]["engine"]
    assert eng.channel_active(0) and len(rx.sondes) == 1
    rx.add_channel("IMET4", F_IMET + 5 * SPACING)              # the pool has one slot
    assert rx.log[-1]["event"] == "no free channel" and len(rx.sondes) == 1
    noise = np.random.default_rng(64).normal(0.0, 60.0, size=2 * 240000).round().astype(np.int16)
    out = []
    for _ in range(6):                                         # 0.6 s of noise
        out += rx.push(noise)
    released = [e for e in rx.log if e["event"] == "released"]
    assert out == [] and len(released) == 1 and released[0]["type"] == "IMET4" and released[0]["slot"] == 0, rx.log
    assert not eng.channel_active(0) and rx.sondes == []
    rx.add_channel("IMET4", F_IMET + 5 * SPACING)
    assert eng.channel_active(0) and rx.sondes[0]["slot"] == 0 and rx.log[-1]["if_sample"] == 6 * 240000 // D
    rx.push(noise)
    rx.close()


def test_imet4_at_a_channel_rate_imet4iq_decimates_is_logged_once_and_starts_nothing():
    """100 kHz channels (M = 32, D = 24): imet4iq takes IF 50 kHz, decM 2, and a block's length need not be even"""
    from radiosonde_auto_rx_amd.wideband import ChannelizedReceiver
    rx = ChannelizedReceiver(SR, M=32, D=24, cfreq_hz=CF, slots=2, chunk=48000, version="oracle")
    assert rx.if_sr == 100000
    rx.add_channel("IMET4", 150_000.0 + 2000.0)
    rx._on_detection(dict(type="IMET4", channel=2, df=0.02, score=1.0))
    out = rx.push(np.zeros(2 * 48000, np.int16), finish=True)
    log, groups, sondes = list(rx.log), dict(rx.groups), list(rx.sondes)
    rx.close()
    assert [e["event"] for e in log] == ["not decodable at this channel rate"], log
    assert groups == {"IMET4": None} and sondes == [] and out == []
