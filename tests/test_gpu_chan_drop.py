"""Dropsondes in the channelized receiver (wideband.py, ChannelizedReceiver): one 2.4 Msps stream, M = 64, D = 48 (50 kHz channels 37.5 kHz apart) with
an RD94 at 4.8 kHz of deviation 1.5 kHz off a channel's centre (the deviation the scanner's template answers) and an RS41.  The dropsonde's
JSON objects are those of the golden made from the narrowband capture with the same frames (tests/dropf32_cases.py WIDE: `iq_dec --FM --lpFM --wav --bo 16
--iq 0.0 - 50000 32 | rd94rd41drop -b --json [-i]`): with the start given by add_channel, with the scanner finding the sonde by itself, and for an inverted
capture, which takes a slot of the -i pool.  A channel rate at which iq_dec would decimate is logged once and starts nothing."""
import functools
import json

import numpy as np
import pytest

from tests import dropf32_cases as cases

pytestmark = pytest.mark.gpu
SR, M, D = 2_400_000, 64, 48
SPACING = SR / M
SECS = 4.6
CF = 403_000_000
F_DROP = 9 * SPACING + 1500.0
F_RS41 = -20 * SPACING - 1500.0
LEAD_S = 0.25                                      # synth.drop_capture's default


@functools.lru_cache(maxsize=None)
def _stream(name):
    from tools import synth
    g = dict(cases.WIDE[name]["gen"])
    g.pop("sr"), g.pop("f_offset_hz")
    n = int(SR * SECS)
    acc = np.zeros(2 * n, np.float64)
    x = synth.drop_capture(sr=SR, fq=F_DROP / SR, noise=None, amp=6000.0, **g)          # the same frames, at the stream's rate and the sonde's place in it
    assert len(x) <= 2 * n
    acc[:len(x)] += x
    x = synth.rs41_capture(sr=SR, seconds=SECS, fq=F_RS41 / SR, seed=62, noise_sigma=0.0, amp=0.2, sonde_id="N3333333", t_first=0.2,
                           frame_kw=dict(ecef_cm=(418833319, 85974133, 473346430)))
    acc[:len(x)] += x[:2 * n]
    acc += np.random.default_rng(63).normal(0.0, 60.0, size=2 * n)
    iq = np.clip(np.round(acc), -32768, 32767).astype(np.int16)
    iq.setflags(write=False)
    return iq


def _golden(name):
    g = cases.load(name)
    objs = [json.loads(l) for l in g["stdout"][0].decode("utf-8").split("\n") if l.startswith("{")]
    assert len(objs) == 8 and g["argv"] == cases.WIDE[name]["argv"]
    return objs


@functools.lru_cache(maxsize=None)
def _receive(name, add, invert=False):
    from radiosonde_auto_rx_amd.wideband import ChannelizedReceiver
    iq = _stream(name)
    n = len(iq) // 2
    rx = ChannelizedReceiver(SR, M=M, D=D, cfreq_hz=CF, slots=2, version="oracle")
    assert rx.if_sr == 50000
    if add:
        rx.add_channel("RD94RD41", F_DROP, invert=invert)
    out = []
    for s0 in range(0, n, rx.chunk):
        out += rx.push(iq[2 * s0:2 * min(n, s0 + rx.chunk)], finish=(s0 + rx.chunk >= n))
    res = dict(out=out, log=list(rx.log), groups=sorted(k for k, g in rx.groups.items() if g is not None),
               sondes=[dict(type=s["type"], f_hz=s["f_hz"], chan=s["chan"], frames=s["frames"], invert=s.get("invert")) for s in rx.sondes])
    rx.close()
    return res


def _without_freq(j):
    return {k: v for k, v in j.items() if k != "freq"}


def _drop_objects(r):
    return [j for j in r["out"] if j["type"] in ("RD94", "RD41")]


def test_told_start_prints_the_goldens_objects():
    r = _receive("wide94", True)
    started = [e for e in r["log"] if e["event"] == "detected" and e["type"] == "RD94RD41"]
    assert len(started) == 1 and started[0]["if_sample"] == 0 and started[0]["channel"] == 9 and started[0]["invert"] is False, r["log"]
    assert abs((started[0]["f_hz"] - 9 * SPACING) / 50000 - 0.03) < 1e-12              # --iq of the slot: the 1.5 kHz that are left inside the channel
    ref, got = _golden("wide94"), _drop_objects(r)
    assert [_without_freq(j) for j in got] == ref, (len(got), len(ref), got[:1], ref[:1])
    assert all("freq" not in j for j in ref) and all(j["freq"] == int(round((CF + F_DROP) / 1000.0)) for j in got), got[0]
    assert r["groups"] == ["RD94RD41", "RS41"]
    assert sum(s["frames"] for s in r["sondes"] if s["type"] == "RS41") >= 3, r["log"]   # the RS41 is decoded as before


def _told_nothing(name, invert):
    r = _receive(name, False)
    started = [e for e in r["log"] if e["event"] == "detected" and e["type"] == "RD94RD41"]
    assert len(started) == 1, [e for e in r["log"] if e["event"] != "released"]
    assert started[0]["invert"] is invert and abs(started[0]["f_hz"] - F_DROP) < 600.0, started
    # frame i's header begins LEAD_S + (40 + 2400 i) raw bits into the capture; behind the slot's first sample it is decoded whole
    ref = _golden(name)
    behind = [j for i, j in enumerate(ref) if (LEAD_S + (40 + 2400 * i) / 4800.0) * 50000 > started[0]["if_sample"]]
    assert 2 * len(behind) >= len(ref), (len(behind), started)
    got = {j["frame"]: _without_freq(j) for j in _drop_objects(r)}
    for j in behind:
        assert got.get(j["frame"]) == j, (j, got.get(j["frame"]))
    assert sum(s["frames"] for s in r["sondes"] if s["type"] == "RS41") >= 3, r["log"]
    return r


def test_told_nothing_finds_and_decodes_the_dropsonde():
    r = _told_nothing("wide94", False)
    assert "RD94RD41" in r["groups"] and "RD94RD41 -i" not in r["groups"]


def test_inverted_capture_told_start_takes_the_inverting_pool():
    r = _receive("wide_inv41", True, True)
    started = [e for e in r["log"] if e["event"] == "detected" and e["type"] == "RD94RD41"]
    assert len(started) == 1 and started[0]["invert"] is True
    assert r["groups"] == ["RD94RD41 -i", "RS41"]
    assert [_without_freq(j) for j in _drop_objects(r)] == _golden("wide_inv41")


def test_inverted_capture_told_nothing_starts_with_i():
    r = _told_nothing("wide_inv41", True)
    assert "RD94RD41 -i" in r["groups"] and "RD94RD41" not in r["groups"]


def test_dropsonde_at_a_channel_rate_iq_dec_decimates_is_logged_once_and_starts_nothing():
    """100 kHz channels (M = 32, D = 24): iq_dec takes IF 50 kHz, dec 2"""
    from radiosonde_auto_rx_amd.wideband import ChannelizedReceiver
    rx = ChannelizedReceiver(SR, M=32, D=24, cfreq_hz=CF, slots=2, chunk=48000, version="oracle")
    assert rx.if_sr == 100000
    rx.add_channel("RD94RD41", 150_000.0 + 2000.0)
    rx._on_detection(dict(type="RD94RD41", channel=2, df=0.02, score=-1.0))
    out = rx.push(np.zeros(2 * 48000, np.int16), finish=True)
    log, groups, sondes = list(rx.log), dict(rx.groups), list(rx.sondes)
    rx.close()
    assert [e["event"] for e in log] == ["not decodable at this channel rate"], log
    assert log[0]["type"] == "RD94RD41" and groups == {"RD94RD41": None, "RD94RD41 -i": None} and sondes == [] and out == []


def test_idle_dropsonde_slot_is_finished_and_goes_back_to_the_pool():
    from radiosonde_auto_rx_amd.wideband import ChannelizedReceiver
    rx = ChannelizedReceiver(SR, M=M, D=D, cfreq_hz=CF, slots=1, chunk=240000, idle_s=0.25, version="oracle")
    rx.add_channel("RD94RD41", F_DROP)
    eng = rx.groups["RD94RD41"]["engine"]
    assert eng.channel_active(0) and len(rx.sondes) == 1
    rx.add_channel("RD94RD41", F_DROP + 5 * SPACING)            # the pool has one slot
    assert rx.log[-1]["event"] == "no free channel" and len(rx.sondes) == 1
    noise = np.random.default_rng(64).normal(0.0, 60.0, size=2 * 240000).round().astype(np.int16)
    out = []
    for _ in range(6):                                          # 0.6 s of noise
        out += rx.push(noise)
    released = [e for e in rx.log if e["event"] == "released"]
    assert out == [] and len(released) == 1 and released[0]["type"] == "RD94RD41" and released[0]["slot"] == 0, rx.log
    assert not eng.channel_active(0) and rx.sondes == []
    rx.add_channel("RD94RD41", F_DROP + 5 * SPACING)
    assert eng.channel_active(0) and rx.sondes[0]["slot"] == 0 and rx.log[-1]["if_sample"] == 6 * 240000 // D
    rx.push(noise)
    rx.close()
