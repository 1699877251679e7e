"""Wall time of the LMS6 soft-bit consumer on the device (SoftinDev(kind="lms6"): k_softin_lms6 — header search, block assembly, wave Viterbi — plus the
per-channel host decoder behind block_bytes) per second of soft bits, beside the host tier (sonde_lms6_dec_push_soft: everything on one CPU thread) on the
same streams on the same machine.

N channels x one second (4800 soft bits) per push, the soft bits already in device memory: a 13 s stream of 15 LMS6 blocks (15 x 4160 = 13 x 4800 bits) at
sigma 0.3, repeated, so that every push continues the stream of the one before.  One warm-up round of 13 pushes (module load, the first blocks), then
--pushes timed pushes (>= 30), each waiting for its kernels, the copies of its blocks and the host decoders: median, min and max per push.  The kernel time
alone comes from a run of its own under `rocprofv3 --kernel-trace --stats -- python tools/bench_softin.py --channels 1024`.  The host tier is timed on
--host-channels channels of the same stream (one thread; the figure is per channel and second, and scales linearly).  One JSON line per channel count.

--kind m20 (or all): the M20 consumer (SoftinDev(kind="m20", skip=False): k_softin_m20, auto_rx's form `m20mod --json --ptu -vvv --softin -i`) the same way — N channels x
one second (9600 symbols) per push in device memory, a 13 s stream with one frame per second at sigma 0.3, repeated; the same warm-up and timed counts; beside it the host
framer on the same stream (sonde_softin_push + sonde_softin_fetch_m20, one thread).  Only completed frames cross to the host: 38.4 KB of soft decisions per channel and
second stay where the modem left them.  --out keeps the rows of the kinds that were not run.

--kind rs92 (or all): the RS92 consumer (SoftinDev(kind="rs92"): k_softin_rs92 with RS(255,231) on the wave, auto_rx's form `rs92mod -vx -v --crc --ecc --vel --json
--softin -i -e <rinex> --ptu`) — N channels x one second (4800 symbols) per push in device memory, a 13 s flight of tools/synth_rs92.py (inverted, as -i wants it) at sigma
0.3, repeated.  A push is the kernel and the copies of its records (push_ms); the text is made when the records are fetched, by the channel's host decoder, and is timed
apart: text_ms with the synthetic RINEX file loaded (CRCs, PTU, the GPS solution of every frame, JSON) and text_no_gps_ms without orbit data (no solution, no JSON): the
difference is the GPS solve, which stays on the host.  Beside it the host tier (sonde_rs92_dec_push_soft, one thread) with and without orbit data.

--kind imet54 (or all): the iMet-54 consumer (SoftinDev(kind="imet54"): k_softin_imet54 with Hamming(8,4) and both check sums on the wave, auto_rx's form `imet54mod --ecc
--json --softin -i --ptu`) — N channels x one second (4800 symbols) per push in device memory, a 13 s stream of tools/synth.py frames (imet54_frame_bits, one per second,
inverted, as -i wants it) at sigma 0.3, repeated.  A push is the kernel and the copies of its records (push_ms); the text is made when the records are fetched and is timed
apart (text_ms).  Beside it the host tier (sonde_imet54_dec_push_soft, one thread) on the same stream in the same run.  No speed threshold: the rows are the measured pair
and the 19.2 KB of soft decisions per channel and second that stay on the device.

--kind meisei (or all): the Meisei consumer (SoftinDev(kind="meisei"): k_softin_meisei with BCH(63,51) on the wave, auto_rx's form `meisei100mod --softin --json --ptu
--ecc`) — N channels x one second (2400 half symbols: two frames) per push in device memory, a 13 s stream of 26 continuous iMS-100 frames (tools/synth.py
meisei_symbols) at sigma 0.3, repeated.  A push is the kernel and the copies of its records (push_ms); the text is made when the records are fetched and is timed apart
(text_ms).  Beside it the host tier (sonde_meisei_dec_push_soft, one thread) on the same stream in the same run.  No speed threshold: the rows are the measured pair and
the 9.6 KB of soft decisions per channel and second that stay on the device.

--kind mrz, --kind mts01 (or all): the two CRC-only consumers (SoftinDev(kind="mrz"): k_softin_mrz, auto_rx's form `mp3h1mod --auto --json --softin --ptu`;
SoftinDev(kind="mts01"): k_softin_mts01, `mts01mod --softin --json`), each with its CRC-16 on the wave — N channels x one second per push in device memory (MRZ: 2399 half
symbols of tools/synth.py mrz_symbols, two copies of the frame a second; MTS01: 1200 symbols of mts01_onair_bits, a frame a second), a 13 s stream at sigma 0.3, repeated.
A push is the kernel and the copies of its records (push_ms); the text is made when the records are fetched and is timed apart (text_ms).  Beside each the host tier
(sonde_mrz_dec_push_soft / sonde_mts01_dec_push_soft, one thread) on the same stream in the same run.  No speed threshold: the rows are the measured pair and the 9.6 / 4.8
KB of soft decisions per channel and second that stay on the device.

--kind wxr: the WxR-301D consumer (SoftinDev(kind="wxr"): k_softin_wxr with bytes, PN9 and the xor8 / sum8 check on the wave, auto_rx's form `weathex301d --softin -i
--json --pn9`) — N channels x one second (5000 soft bits, the PN9 variant's rate) per push in device memory, a 13 s stream of frames 96 idle bits apart at sigma 0.3,
negated as the modem delivers it, repeated.  13 warm-up pushes, then three rounds of --pushes timed ones: the median of the three round medians, with the smallest and
the largest push of all.  A push is the kernel and the copies of its records (push_ms); the text (WxrPrinter.decoded per record) is timed apart (text_ms).  Beside it
the host framer and printer (sonde_wxr_softin_push + sonde_wxr_print_frame, one thread) on the same stream in the same run: reported, not a threshold.  This consumer
is there for the completeness of the device path — 176-byte records instead of 20 KB of soft bits per channel and second — not for speed; the one condition is that
1024 channels take less than a second per second.

--kind rs92 --gps-device: the text of the RS92 fetch alone, with the position solve's 4-satellite subset search on the host and on the device (SoftinDev(gps_device=True),
DESIGN.md 4.11c), two consumers on the same pushes timed alternately in one run; rows of kind "rs92_gps" (the rs92 rows stay).

    python tools/bench_softin.py [--kind lms6|m20|rs92|imet54|meisei|mrz|mts01|wxr|all] [--gps-device] [--channels 1,64,341,1024] [--pushes 39] [--vit 2] [--typ 0] [--out profiles/softin_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def lms6_stream(sigma=0.3, seed=1):
    from tools import synth
    bits = synth.lms6_onair_bits(15)
    assert len(bits) == 13 * 4800
    rng = np.random.default_rng(seed)
    return (2.0 * bits.astype(np.float64) - 1.0 + rng.normal(0.0, sigma, len(bits))).astype(np.float32)


def host_tier(s, pushes, nch, vit, typ):
    """ms per push of one channel through sonde_lms6_dec_push_soft (median over the timed pushes), [OK] frames of one channel"""
    from radiosonde_auto_rx_amd.engine import lib
    from radiosonde_auto_rx_amd.fsk import Lms6Opts
    L = lib()
    L.sonde_lms6_dec_create.argtypes = [C.POINTER(Lms6Opts), C.POINTER(C.c_void_p)]
    L.sonde_lms6_dec_destroy.argtypes = [C.c_void_p]
    L.sonde_lms6_dec_push_soft.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]
    o = Lms6Opts(json=1, vit=vit, typ=typ)
    decs = []
    for _ in range(nch):
        d = C.c_void_p()
        assert L.sonde_lms6_dec_create(C.byref(o), C.byref(d)) == 0
        decs.append(d)
    out = C.create_string_buffer(1 << 16)
    walls, ok = [], 0
    for k in range(13 + pushes):
        p = s.ctypes.data + (k % 13) * 4800 * 4
        t0 = time.perf_counter()
        for d in decs:
            n = L.sonde_lms6_dec_push_soft(d, p, 4800, 0, 0, out, len(out))
            assert n >= 0
        dt = (time.perf_counter() - t0) * 1e3
        if k >= 13:
            walls.append(dt / nch)
            ok += out.value.count(b"[OK]")
    for d in decs:
        L.sonde_lms6_dec_destroy(d)
    return walls, ok


def m20_stream(sigma=0.3, seed=2):
    """13 s at 9600 Bd: per second the 1001 idle pattern, the header and one frame (tools/synth.py m20_frame), noise on everything"""
    from tools import synth
    rng = np.random.default_rng(seed)
    out = []
    for k in range(13):
        sym = synth.m10_symbols(data=synth.m20_frame(k))
        out += [np.tile(np.array([1, 0, 0, 1], np.uint8), 250), sym, np.tile(np.array([1, 0, 0, 1], np.uint8), (9600 - 1000 - len(sym)) // 4)]
    s = 2.0 * np.concatenate(out).astype(np.float64) - 1.0
    assert len(s) == 13 * 9600
    return (s + rng.normal(0.0, sigma, len(s))).astype(np.float32)


def m20_host_tier(s, pushes, nch):
    """ms per push of one channel through the host framer (no-skip), frames with a good checksum of one channel"""
    from radiosonde_auto_rx_amd.engine import lib, SondeM20Frame, SONDE_M20
    L = lib()
    L.sonde_softin_create.argtypes = [C.c_int32] * 5 + [C.POINTER(C.c_void_p)]
    L.sonde_softin_destroy.argtypes = [C.c_void_p]
    L.sonde_softin_push.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    L.sonde_softin_set_m10_skip.argtypes = [C.c_void_p, C.c_int32]
    L.sonde_softin_fetch_m20.argtypes = [C.c_void_p, C.POINTER(SondeM20Frame), C.c_int32]
    hs = []
    for _ in range(nch):
        h = C.c_void_p()
        assert L.sonde_softin_create(SONDE_M20, 0, 0, 1, 0, C.byref(h)) == 0 and L.sonde_softin_set_m10_skip(h, 0) == 0
        hs.append(h)
    buf = (SondeM20Frame * 8)()
    walls, ok = [], 0
    for k in range(13 + pushes):
        p = s.ctypes.data + (k % 13) * 9600 * 4
        t0 = time.perf_counter()
        n = 0
        for h in hs:
            assert L.sonde_softin_push(h, p, 9600) == 0
            n = L.sonde_softin_fetch_m20(h, buf, 8)
            assert n >= 0
        dt = (time.perf_counter() - t0) * 1e3
        if k >= 13:
            walls.append(dt / nch)
            ok += sum(buf[i].cs_ok for i in range(n))
    for h in hs:
        L.sonde_softin_destroy(h)
    return walls, ok


def rs92_stream(sigma=0.3, seed=3):
    """13 s at 4800 symbols: 13 frames of one flight back to back (a frame is a second on air), inverted, noise on everything; the flight's RINEX file as bytes"""
    from tools import synth_rs92 as R
    eph = R.constellation()
    sym = R.onair_symbols(R.flight(13, eph), lead=0)
    assert len(sym) == 13 * 4800
    rng = np.random.default_rng(seed)
    return (-(2.0 * sym.astype(np.float64) - 1.0) + rng.normal(0.0, sigma, len(sym))).astype(np.float32), R.rinex_nav(eph, extra_toe=(-7200.0,))


RS92_OPTS = dict(verbose=1, aux=1, ecc=2, gps_vel=4, json=1, inv=1, ptu=1, gpsepoch=-1)


def rs92_host_tier(s, pushes, nch, rinex):
    """ms per push of one channel through sonde_rs92_dec_push_soft (rinex: with orbit data, else without), frames with a position of one channel"""
    from radiosonde_auto_rx_amd.engine import lib
    from radiosonde_auto_rx_amd.family import Rs92Opts
    L = lib()
    L.sonde_rs92_dec_create.argtypes = [C.POINTER(Rs92Opts), C.POINTER(C.c_void_p)]
    L.sonde_rs92_dec_destroy.argtypes = [C.c_void_p]
    L.sonde_rs92_dec_load_ephemeris.argtypes = [C.c_void_p, C.c_char_p]
    L.sonde_rs92_dec_push_soft.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]
    o = Rs92Opts(**RS92_OPTS)
    decs = []
    for _ in range(nch):
        d = C.c_void_p()
        assert L.sonde_rs92_dec_create(C.byref(o), C.byref(d)) == 0
        if rinex:
            assert L.sonde_rs92_dec_load_ephemeris(d, os.fsencode(rinex)) == 0
        decs.append(d)
    out = C.create_string_buffer(1 << 16)
    walls, ok = [], 0
    for k in range(13 + pushes):
        p = s.ctypes.data + (k % 13) * 4800 * 4
        t0 = time.perf_counter()
        for d in decs:
            n = L.sonde_rs92_dec_push_soft(d, p, 4800, 0, 0, out, len(out))
            assert n >= 0
        dt = (time.perf_counter() - t0) * 1e3
        if k >= 13:
            walls.append(dt / nch)
            ok += out.value.count(b'"lat"')
    for d in decs:
        L.sonde_rs92_dec_destroy(d)
    return walls, ok


def rs92_rows(a):
    import tempfile
    import torch
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    s, nav = rs92_stream()
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        rinex = os.path.join(tmp, "brdc.nav")
        with open(rinex, "wb") as f:
            f.write(nav)
        hw, hok = rs92_host_tier(s, a.pushes, a.host_channels, rinex)
        hw0, _ = rs92_host_tier(s, a.pushes, a.host_channels, None)
        host_ms, host0_ms = statistics.median(hw), statistics.median(hw0)
        for nch in [int(c) for c in a.channels.split(",")]:
            d = torch.from_numpy(s).to("cuda").repeat(nch, 1).contiguous()
            torch.cuda.synchronize()
            res = {}
            for orbit in (True, False):
                sf = SoftinDev(nch, kind="rs92", rs92_opts=dict(ptu=1), ephemeris=rinex if orbit else None)
                walls, texts, ok, frames, repaired = [], [], 0, 0, 0
                for k in range(13 + a.pushes):
                    p = d.data_ptr() + (k % 13) * 4800 * 4
                    t0 = time.perf_counter()
                    sf.push_device(p, d.shape[1], 4800)
                    t1 = time.perf_counter()
                    recs = sf.fetch_rs92(nch + 16)
                    t2 = time.perf_counter()
                    if k >= 13:
                        walls.append((t1 - t0) * 1e3); texts.append((t2 - t1) * 1e3)
                        frames += len(recs)
                        ok += sum(r["text"].count('"lat"') for r in recs if r["channel"] == 0)
                        repaired += sum(r["ec"] > 0 for r in recs)
                res[orbit] = (walls, texts, ok, frames, repaired, sf.counts())
                sf.close()
            walls, texts, ok, frames, repaired, cnt = res[True]
            wall, text, text0 = statistics.median(walls), statistics.median(texts), statistics.median(res[False][1])
            row = {"kind": "rs92", "channels": nch, "pushes": a.pushes, "push_ms": round(wall, 3), "min_ms": round(min(walls), 3), "max_ms": round(max(walls), 3),
                   "text_ms": round(text, 3), "text_min_ms": round(min(texts), 3), "text_max_ms": round(max(texts), 3), "text_no_gps_ms": round(text0, 3),
                   "push_plus_text_ms": round(wall + text, 3), "channel_seconds_per_second": round(nch * 1e3 / (wall + text), 1), "frames": frames, "repaired": repaired,
                   "positions_channel0": ok, "dropped": cnt["dropped"], "soft_bytes_per_channel_second_left_on_device": 4800 * 4,
                   "host_tier_ms_per_channel_second": round(host_ms, 4), "host_tier_min_ms": round(min(hw), 4), "host_tier_max_ms": round(max(hw), 4),
                   "host_tier_no_gps_ms_per_channel_second": round(host0_ms, 4), "host_tier_ms_for_these_channels": round(host_ms * nch, 2),
                   "host_tier_positions_one_channel": hok}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def rs92_gps_rows(a):
    """--gps-device: the text of an RS92 fetch with the position solve's subset search on the host (today's path) and on the device (SoftinDev(gps_device=True)),
    timed alternately in ONE run on the same records: two consumers get the same push, their fetches are timed one after the other, the order swapped every push.
    host_text_in_stored_range says whether the host figure of this run lies within min .. max of the stored rs92 row of the same channel count (a.out), or the
    stored text_ms within this run's: otherwise the pair is not comparable with the stored rows."""
    import tempfile
    import torch
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    s, nav = rs92_stream()
    stored = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            stored = {r["channels"]: r for r in json.load(f) if r.get("kind") == "rs92"}
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        rinex = os.path.join(tmp, "brdc.nav")
        with open(rinex, "wb") as f:
            f.write(nav)
        for nch in [int(c) for c in a.channels.split(",")]:
            d = torch.from_numpy(s).to("cuda").repeat(nch, 1).contiguous()
            torch.cuda.synchronize()
            sf = {dev: SoftinDev(nch, kind="rs92", rs92_opts=dict(ptu=1), ephemeris=rinex, gps_device=dev) for dev in (False, True)}
            texts, pos, same = {False: [], True: []}, {False: 0, True: 0}, True
            for k in range(13 + a.pushes):
                p = d.data_ptr() + (k % 13) * 4800 * 4
                got = {}
                for dev in ((False, True) if k % 2 == 0 else (True, False)):
                    sf[dev].push_device(p, d.shape[1], 4800)
                    t1 = time.perf_counter()
                    got[dev] = sf[dev].fetch_rs92(nch + 16)
                    t2 = time.perf_counter()
                    if k >= 13:
                        texts[dev].append((t2 - t1) * 1e3)
                        pos[dev] += sum(r["text"].count('"lat"') for r in got[dev])
                key = lambda recs: sorted((r["channel"], r["hdr_bit"], r["text"]) for r in recs)      # noqa: E731
                same = same and key(got[False]) == key(got[True])
            st = sf[True].rs92_gps_stats()
            for v in sf.values():
                v.close()
            th, td = statistics.median(texts[False]), statistics.median(texts[True])
            row = {"kind": "rs92_gps", "channels": nch, "pushes": a.pushes, "text_host_ms": round(th, 3), "text_host_min_ms": round(min(texts[False]), 3),
                   "text_host_max_ms": round(max(texts[False]), 3), "text_device_ms": round(td, 3), "text_device_min_ms": round(min(texts[True]), 3),
                   "text_device_max_ms": round(max(texts[True]), 3), "host_over_device": round(th / td, 2), "positions_host": pos[False], "positions_device": pos[True],
                   "texts_identical": bool(same), "gps_jobs": st["jobs"], "gps_launches": st["launches"], "gps_doubts": st["doubts"], "gps_mismatches": st["mismatches"]}
            if nch in stored:
                r0 = stored[nch]
                row["stored_text_ms"] = r0["text_ms"]
                row["host_text_in_stored_range"] = bool(min(texts[False]) <= r0["text_ms"] <= max(texts[False]) or r0["text_min_ms"] <= th <= r0["text_max_ms"])
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def imet54_stream(sigma=0.3, seed=4):
    """13 s at 4800 symbols: per second the 00 AA preamble, the header, one frame (tools/synth.py imet54_frame_bits) and idle ones; inverted, noise on everything"""
    from tools import synth
    rng = np.random.default_rng(seed)
    pre = np.array([int(c) for c in ("0000000001" "0101010101") * 9], np.uint8)
    hdr = np.array([int(c) for c in synth.FAMILY["imet54mod"]["header"]], np.uint8)
    out = []
    for k in range(13):
        out += [pre, hdr, synth.imet54_frame_bits(synth.imet54_frame(k)), np.ones(4800 - len(pre) - len(hdr) - 2200, np.uint8)]
    s = -(2.0 * np.concatenate(out).astype(np.float64) - 1.0)
    assert len(s) == 13 * 4800
    return (s + rng.normal(0.0, sigma, len(s))).astype(np.float32)


IMET54_OPTS = dict(ecc=1, json=1, ptu=1, inv=1)


def imet54_host_tier(s, pushes, nch):
    """ms per push of one channel through sonde_imet54_dec_push_soft, JSON objects of one channel"""
    from radiosonde_auto_rx_amd.engine import lib
    from radiosonde_auto_rx_amd.family import Imet54Opts
    L = lib()
    L.sonde_imet54_dec_create.argtypes = [C.POINTER(Imet54Opts), C.POINTER(C.c_void_p)]
    L.sonde_imet54_dec_destroy.argtypes = [C.c_void_p]
    L.sonde_imet54_dec_push_soft.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]
    o = Imet54Opts(**IMET54_OPTS)
    decs = []
    for _ in range(nch):
        d = C.c_void_p()
        assert L.sonde_imet54_dec_create(C.byref(o), C.byref(d)) == 0
        decs.append(d)
    out = C.create_string_buffer(1 << 16)
    walls, ok = [], 0
    for k in range(13 + pushes):
        p = s.ctypes.data + (k % 13) * 4800 * 4
        t0 = time.perf_counter()
        for d in decs:
            n = L.sonde_imet54_dec_push_soft(d, p, 4800, 0, 0, out, len(out))
            assert n >= 0
        dt = (time.perf_counter() - t0) * 1e3
        if k >= 13:
            walls.append(dt / nch)
            ok += out.value.count(b'"type": "IMET5"')
    for d in decs:
        L.sonde_imet54_dec_destroy(d)
    return walls, ok


def imet54_rows(a):
    import torch
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    s = imet54_stream()
    hw, hok = imet54_host_tier(s, a.pushes, a.host_channels)
    host_ms = statistics.median(hw)
    rows = []
    for nch in [int(c) for c in a.channels.split(",")]:
        d = torch.from_numpy(s).to("cuda").repeat(nch, 1).contiguous()
        torch.cuda.synchronize()
        sf = SoftinDev(nch, kind="imet54", imet54_opts=dict(IMET54_OPTS))
        walls, texts, ok, frames, repaired = [], [], 0, 0, 0
        for k in range(13 + a.pushes):
            p = d.data_ptr() + (k % 13) * 4800 * 4
            t0 = time.perf_counter()
            sf.push_device(p, d.shape[1], 4800)
            t1 = time.perf_counter()
            recs = sf.fetch_imet54(4 * nch + 16)
            t2 = time.perf_counter()
            if k >= 13:
                walls.append((t1 - t0) * 1e3); texts.append((t2 - t1) * 1e3)
                frames += len(recs)
                ok += sum(r["text"].count('"type": "IMET5"') for r in recs if r["channel"] == 0)
                repaired += sum(r["ecc_frm"] > 0 for r in recs)
        cnt = sf.counts()
        sf.close()
        wall, text = statistics.median(walls), statistics.median(texts)
        row = {"kind": "imet54", "channels": nch, "pushes": a.pushes, "push_ms": round(wall, 3), "min_ms": round(min(walls), 3), "max_ms": round(max(walls), 3),
               "text_ms": round(text, 3), "text_min_ms": round(min(texts), 3), "text_max_ms": round(max(texts), 3), "push_plus_text_ms": round(wall + text, 3),
               "channel_seconds_per_second": round(nch * 1e3 / (wall + text), 1), "frames": frames, "repaired": repaired, "json_channel0": ok, "dropped": cnt["dropped"],
               "soft_bytes_per_channel_second_left_on_device": 4800 * 4,
               "host_tier_ms_per_channel_second": round(host_ms, 4), "host_tier_min_ms": round(min(hw), 4), "host_tier_max_ms": round(max(hw), 4),
               "host_tier_ms_for_these_channels": round(host_ms * nch, 2), "host_tier_json_one_channel": hok}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def meisei_stream(sigma=0.3, seed=5):
    """13 s at 2400 half symbols: 26 continuous iMS-100 frames (tools/synth.py meisei_symbols), noise on everything"""
    from tools import synth
    rng = np.random.default_rng(seed)
    s = 2.0 * synth.meisei_symbols(26, "ims100").astype(np.float64) - 1.0
    assert len(s) == 13 * 2400
    return (s + rng.normal(0.0, sigma, len(s))).astype(np.float32)


MEISEI_OPTS = dict(ecc=1, json=1, ptu=1)


def meisei_host_tier(s, pushes, nch):
    """ms per push of one channel through sonde_meisei_dec_push_soft, JSON objects of one channel"""
    from radiosonde_auto_rx_amd.engine import lib
    from radiosonde_auto_rx_amd.family import MeiseiOpts
    L = lib()
    L.sonde_meisei_dec_create.argtypes = [C.POINTER(MeiseiOpts), C.POINTER(C.c_void_p)]
    L.sonde_meisei_dec_destroy.argtypes = [C.c_void_p]
    L.sonde_meisei_dec_push_soft.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]
    o = MeiseiOpts(**MEISEI_OPTS)
    decs = []
    for _ in range(nch):
        d = C.c_void_p()
        assert L.sonde_meisei_dec_create(C.byref(o), C.byref(d)) == 0
        decs.append(d)
    out = C.create_string_buffer(1 << 16)
    walls, ok = [], 0
    for k in range(13 + pushes):
        p = s.ctypes.data + (k % 13) * 2400 * 4
        t0 = time.perf_counter()
        for d in decs:
            n = L.sonde_meisei_dec_push_soft(d, p, 2400, 0, 0, out, len(out))
            assert n >= 0
        dt = (time.perf_counter() - t0) * 1e3
        if k >= 13:
            walls.append(dt / nch)
            ok += out.value.count(b'"type": "MEISEI"')
    for d in decs:
        L.sonde_meisei_dec_destroy(d)
    return walls, ok


def meisei_rows(a):
    import torch
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    s = meisei_stream()
    hw, hok = meisei_host_tier(s, a.pushes, a.host_channels)
    host_ms = statistics.median(hw)
    rows = []
    for nch in [int(c) for c in a.channels.split(",")]:
        d = torch.from_numpy(s).to("cuda").repeat(nch, 1).contiguous()
        torch.cuda.synchronize()
        sf = SoftinDev(nch, kind="meisei", meisei_opts=dict(MEISEI_OPTS))
        walls, texts, ok, frames, repaired = [], [], 0, 0, 0
        for k in range(13 + a.pushes):
            p = d.data_ptr() + (k % 13) * 2400 * 4
            t0 = time.perf_counter()
            sf.push_device(p, d.shape[1], 2400)
            t1 = time.perf_counter()
            recs = sf.fetch_meisei(4 * nch + 16)
            t2 = time.perf_counter()
            if k >= 13:
                walls.append((t1 - t0) * 1e3); texts.append((t2 - t1) * 1e3)
                frames += len(recs)
                ok += sum(r["text"].count('"type": "MEISEI"') for r in recs if r["channel"] == 0)
                repaired += sum(any(e in (1, 2) for e in r["block_err"]) for r in recs)
        cnt = sf.counts()
        sf.close()
        wall, text = statistics.median(walls), statistics.median(texts)
        row = {"kind": "meisei", "channels": nch, "pushes": a.pushes, "push_ms": round(wall, 3), "min_ms": round(min(walls), 3), "max_ms": round(max(walls), 3),
               "text_ms": round(text, 3), "text_min_ms": round(min(texts), 3), "text_max_ms": round(max(texts), 3), "push_plus_text_ms": round(wall + text, 3),
               "channel_seconds_per_second": round(nch * 1e3 / (wall + text), 1), "frames": frames, "repaired": repaired, "json_channel0": ok, "dropped": cnt["dropped"],
               "soft_bytes_per_channel_second_left_on_device": 2400 * 4,
               "host_tier_ms_per_channel_second": round(host_ms, 4), "host_tier_min_ms": round(min(hw), 4), "host_tier_max_ms": round(max(hw), 4),
               "host_tier_ms_for_these_channels": round(host_ms * nch, 2), "host_tier_json_one_channel": hok}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def mrz_stream(sigma=0.3, seed=6):
    """13 s at 2399 half symbols: two copies of a frame a second, AA AA and idle (tools/synth.py mrz_symbols), noise on everything"""
    from tools import synth
    rng = np.random.default_rng(seed)
    s = 2.0 * synth.mrz_symbols(13).astype(np.float64) - 1.0
    assert len(s) == 13 * 2399
    return (s + rng.normal(0.0, sigma, len(s))).astype(np.float32)


def mts01_stream(sigma=0.3, seed=7):
    """13 s at 1200 symbols: idle, header and a frame a second (tools/synth.py mts01_onair_bits), noise on everything"""
    from tools import synth
    rng = np.random.default_rng(seed)
    s = 2.0 * synth.mts01_onair_bits(13).astype(np.float64) - 1.0
    assert len(s) == 13 * 1200
    return (s + rng.normal(0.0, sigma, len(s))).astype(np.float32)


# kind -> (stream, symbols a push, options, options struct (family.py), the host tier's calls, what a good frame prints, records a push can hold per channel)
CRC_KINDS = {"mrz": (mrz_stream, 2399, dict(aut=1, json=1, ptu=1), "MrzOpts", "sonde_mrz_dec", b"[OK]", 8),
             "mts01": (mts01_stream, 1200, dict(json=1), "Mts01Opts", "sonde_mts01_dec", b"[OK]", 4)}


def crc_host_tier(kind, s, pushes, nch):
    """ms per push of one channel through the kind's host tier (sonde_*_dec_push_soft), [OK] frames of one channel"""
    from radiosonde_auto_rx_amd.engine import lib
    from radiosonde_auto_rx_amd import family
    _, per, opts, struct, calls, mark, _ = CRC_KINDS[kind]
    L = lib()
    create, destroy, push = (getattr(L, calls + sfx) for sfx in ("_create", "_destroy", "_push_soft"))
    O = getattr(family, struct)
    create.argtypes = [C.POINTER(O), C.POINTER(C.c_void_p)]
    destroy.argtypes = [C.c_void_p]
    push.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]
    o = O(**opts)
    decs = []
    for _ in range(nch):
        d = C.c_void_p()
        assert create(C.byref(o), C.byref(d)) == 0
        decs.append(d)
    out = C.create_string_buffer(1 << 16)
    walls, ok = [], 0
    for k in range(13 + pushes):
        p = s.ctypes.data + (k % 13) * per * 4
        t0 = time.perf_counter()
        for d in decs:
            n = push(d, p, per, 0, 0, out, len(out))
            assert n >= 0
        dt = (time.perf_counter() - t0) * 1e3
        if k >= 13:
            walls.append(dt / nch)
            ok += out.raw[:n].count(mark)
    for d in decs:
        destroy(d)
    return walls, ok


def crc_rows(a, kind):
    import torch
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    stream, per, opts, _, _, mark, per_cap = CRC_KINDS[kind]
    s = stream()
    hw, hok = crc_host_tier(kind, s, a.pushes, a.host_channels)
    host_ms = statistics.median(hw)
    rows = []
    for nch in [int(c) for c in a.channels.split(",")]:
        d = torch.from_numpy(s).to("cuda").repeat(nch, 1).contiguous()
        torch.cuda.synchronize()
        sf = SoftinDev(nch, kind=kind, **{kind + "_opts": dict(opts)})
        fetch = getattr(sf, "fetch_" + kind)
        walls, texts, ok, frames, good = [], [], 0, 0, 0
        for k in range(13 + a.pushes):
            p = d.data_ptr() + (k % 13) * per * 4
            t0 = time.perf_counter()
            sf.push_device(p, d.shape[1], per)
            t1 = time.perf_counter()
            recs = fetch(per_cap * nch + 16)
            t2 = time.perf_counter()
            if k >= 13:
                walls.append((t1 - t0) * 1e3); texts.append((t2 - t1) * 1e3)
                frames += len(recs)
                ok += sum(r["text"].count(mark.decode()) for r in recs if r["channel"] == 0)
                good += sum(r["crc_ok"] for r in recs)
        cnt = sf.counts()
        sf.close()
        wall, text = statistics.median(walls), statistics.median(texts)
        row = {"kind": kind, "channels": nch, "pushes": a.pushes, "push_ms": round(wall, 3), "min_ms": round(min(walls), 3), "max_ms": round(max(walls), 3),
               "text_ms": round(text, 3), "text_min_ms": round(min(texts), 3), "text_max_ms": round(max(texts), 3), "push_plus_text_ms": round(wall + text, 3),
               "channel_seconds_per_second": round(nch * 1e3 / (wall + text), 1), "frames": frames, "crc_ok": good, "ok_channel0": ok, "dropped": cnt["dropped"],
               "soft_bytes_per_channel_second_left_on_device": per * 4,
               "host_tier_ms_per_channel_second": round(host_ms, 4), "host_tier_min_ms": round(min(hw), 4), "host_tier_max_ms": round(max(hw), 4),
               "host_tier_ms_for_these_channels": round(host_ms * nch, 2), "host_tier_ok_one_channel": hok}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


WXR_PER = 5000                                             # soft bits a second at the PN9 variant's rate


def wxr_stream(sigma=0.3, seed=8):
    """13 s at 5000 soft bits: PN9 frames 96 idle bits apart (tools/synth.py wxr_frames), noise on everything, negated (auto_rx runs the decoder with -i)"""
    from tools import synth
    rng = np.random.default_rng(seed)
    n = 13 * WXR_PER
    frames = synth.wxr_frames(n // 648, True)
    bits = np.unpackbits(np.frombuffer(b"".join(b"\xAA" * 12 + f for f in frames), np.uint8))
    bits = np.concatenate([bits, np.tile(np.array([1, 0], np.uint8), n)])[:n]
    s = 2.0 * bits.astype(np.float64) - 1.0
    return np.ascontiguousarray(-(s + rng.normal(0.0, sigma, n)), dtype=np.float32)


def wxr_host_tier(s, pushes, nch):
    """ms per push of one channel through the host framer and printer (one thread), [OK] lines of one channel"""
    from radiosonde_auto_rx_amd.wxr import WxrPrinter, WxrSoftin
    chans = [(WxrSoftin(pn9=True, invert=True), WxrPrinter(json=True, pn9=True)) for _ in range(nch)]
    walls, ok = [], 0
    for k in range(13 + pushes):
        x = s[(k % 13) * WXR_PER:(k % 13 + 1) * WXR_PER]
        t0 = time.perf_counter()
        for fr, pr in chans:
            text = "".join(pr.frame(f["bits"]) for f in fr.push(x))
        dt = (time.perf_counter() - t0) * 1e3
        if k >= 13:
            walls.append(dt / nch)
            ok += text.count("[OK]")
    for fr, pr in chans:
        fr.close(); pr.close()
    return walls, ok


def wxr_rows(a):
    import torch
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    from radiosonde_auto_rx_amd.wxr import WxrPrinter
    s = wxr_stream()
    hw, hok = wxr_host_tier(s, a.pushes, a.host_channels)
    host_ms = statistics.median(hw)
    rows = []
    for nch in [int(c) for c in a.channels.split(",")]:
        d = torch.from_numpy(s).to("cuda").repeat(nch, 1).contiguous()
        torch.cuda.synchronize()
        sf = SoftinDev(nch, kind="wxr", wxr_opts=dict(pn9=1, inv=1))
        printers = [WxrPrinter(json=True, pn9=True) for _ in range(nch)]
        rounds_w, rounds_t, walls, texts, ok, frames, good = [], [], [], [], 0, 0, 0
        for k in range(13 + 3 * a.pushes):
            p = d.data_ptr() + (k % 13) * WXR_PER * 4
            t0 = time.perf_counter()
            sf.push_device(p, d.shape[1], WXR_PER)
            t1 = time.perf_counter()
            recs = sf.fetch_wxr(20 * nch + 16)
            text0 = ""
            for r in recs:
                t = printers[r["channel"]].decoded(r)
                if r["channel"] == 0:
                    text0 += t
            t2 = time.perf_counter()
            if k >= 13:
                walls.append((t1 - t0) * 1e3); texts.append((t2 - t1) * 1e3)
                frames += len(recs)
                ok += text0.count("[OK]")
                good += sum(r["chk_ok"] for r in recs)
                if len(walls) % a.pushes == 0:
                    rounds_w.append(statistics.median(walls[-a.pushes:])); rounds_t.append(statistics.median(texts[-a.pushes:]))
        cnt = sf.counts()
        sf.close()
        for pr in printers:
            pr.close()
        wall, text = statistics.median(rounds_w), statistics.median(rounds_t)
        row = {"kind": "wxr", "channels": nch, "pushes": a.pushes, "rounds": 3, "push_ms": round(wall, 3), "round_medians_ms": [round(v, 3) for v in rounds_w],
               "min_ms": round(min(walls), 3), "max_ms": round(max(walls), 3),
               "text_ms": round(text, 3), "text_min_ms": round(min(texts), 3), "text_max_ms": round(max(texts), 3), "push_plus_text_ms": round(wall + text, 3),
               "channel_seconds_per_second": round(nch * 1e3 / (wall + text), 1), "a_second_in_less_than_a_second": bool(max(walls) + max(texts) < 1000.0),
               "frames": frames, "chk_ok": good, "ok_channel0": ok, "dropped": cnt["dropped"],
               "soft_bytes_per_channel_second_left_on_device": WXR_PER * 4, "record_bytes_per_channel_second": round(176 * frames / (3 * a.pushes) / nch, 1),
               "host_tier_ms_per_channel_second": round(host_ms, 4), "host_tier_min_ms": round(min(hw), 4), "host_tier_max_ms": round(max(hw), 4),
               "host_tier_ms_for_these_channels": round(host_ms * nch, 2), "host_tier_ok_one_channel": hok}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def m20_rows(a):
    import torch
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    s = m20_stream()
    hw, hok = m20_host_tier(s, a.pushes, a.host_channels)
    host_ms = statistics.median(hw)
    rows = []
    for nch in [int(c) for c in a.channels.split(",")]:
        d = torch.from_numpy(s).to("cuda").repeat(nch, 1).contiguous()
        torch.cuda.synchronize()
        sf = SoftinDev(nch, kind="m20", skip=False)
        walls, ok, frames = [], 0, 0
        for k in range(13 + a.pushes):
            p = d.data_ptr() + (k % 13) * 9600 * 4
            t0 = time.perf_counter()
            sf.push_device(p, d.shape[1], 9600)
            dt = (time.perf_counter() - t0) * 1e3
            recs = sf.fetch_m20(4 * nch + 16)
            if k >= 13:
                walls.append(dt)
                frames += len(recs)
                ok += sum(r["cs_ok"] for r in recs if r["channel"] == 0)
        cnt = sf.counts()
        sf.close()
        wall = statistics.median(walls)
        row = {"kind": "m20", "skip": 0, "channels": nch, "pushes": a.pushes, "push_ms": round(wall, 3), "min_ms": round(min(walls), 3), "max_ms": round(max(walls), 3),
               "channel_seconds_per_second": round(nch * 1e3 / wall, 1), "frames": frames, "ok_channel0": ok, "dropped": cnt["dropped"],
               "soft_bytes_per_channel_second_left_on_device": 9600 * 4,
               "host_tier_ms_per_channel_second": round(host_ms, 4), "host_tier_min_ms": round(min(hw), 4), "host_tier_max_ms": round(max(hw), 4),
               "host_tier_ms_for_these_channels": round(host_ms * nch, 2), "host_tier_ok_one_channel": hok}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="lms6", choices=["lms6", "m20", "rs92", "imet54", "meisei", "mrz", "mts01", "wxr", "all"])
    ap.add_argument("--channels", default="1,64,341,1024")
    ap.add_argument("--pushes", type=int, default=39)
    ap.add_argument("--vit", type=int, default=2)
    ap.add_argument("--typ", type=int, default=0)
    ap.add_argument("--host-channels", type=int, default=4)
    ap.add_argument("--out", default="")
    ap.add_argument("--gps-device", action="store_true", help="--kind rs92: the fetch's text with the subset search on the host and on the device, alternately in one run")
    a = ap.parse_args()
    assert a.pushes >= 30
    if a.gps_device:
        assert a.kind == "rs92", "--gps-device goes with --kind rs92"
        rows = rs92_gps_rows(a)
    else:
        rows = main_rows(a)
    write_rows(a, rows)


def main_rows(a):
    return (lms6_rows(a) if a.kind in ("lms6", "all") else []) + (m20_rows(a) if a.kind in ("m20", "all") else []) + (rs92_rows(a) if a.kind in ("rs92", "all") else []) \
        + (imet54_rows(a) if a.kind in ("imet54", "all") else []) + (meisei_rows(a) if a.kind in ("meisei", "all") else []) \
        + (crc_rows(a, "mrz") if a.kind in ("mrz", "all") else []) + (crc_rows(a, "mts01") if a.kind in ("mts01", "all") else []) \
        + (wxr_rows(a) if a.kind in ("wxr", "all") else [])


def write_rows(a, rows):
    if a.out:
        kinds = {r["kind"] for r in rows}
        if os.path.exists(a.out):
            with open(a.out) as f:
                rows = [r for r in json.load(f) if r.get("kind") not in kinds] + rows
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


def lms6_rows(a):
    import torch
    from radiosonde_auto_rx_amd.fsk import SoftinDev
    s = lms6_stream()
    hw, hok = host_tier(s, a.pushes, a.host_channels, a.vit, a.typ)
    host_ms = statistics.median(hw)
    rows = []
    for nch in [int(c) for c in a.channels.split(",")]:
        d = torch.from_numpy(s).to("cuda").repeat(nch, 1).contiguous()
        torch.cuda.synchronize()
        sf = SoftinDev(nch, kind="lms6", json=True, vit=a.vit, typ=a.typ, ecc=0)
        walls, ok, blocks = [], 0, 0
        for k in range(13 + a.pushes):
            p = d.data_ptr() + (k % 13) * 4800 * 4
            t0 = time.perf_counter()
            sf.push_device(p, d.shape[1], 4800)
            dt = (time.perf_counter() - t0) * 1e3
            recs = sf.fetch_lms6(2 * nch + 16)
            if k >= 13:
                walls.append(dt)
                blocks += len(recs)
                ok += sum(r["text"].count("[OK]") for r in recs if r["channel"] == 0)
        cnt = sf.counts()
        sf.close()
        wall = statistics.median(walls)
        row = {"kind": "lms6", "vit": a.vit, "typ": a.typ, "channels": nch, "pushes": a.pushes, "push_ms": round(wall, 3), "min_ms": round(min(walls), 3),
               "max_ms": round(max(walls), 3), "channel_seconds_per_second": round(nch * 1e3 / wall, 1), "blocks": blocks, "ok_channel0": ok, "dropped": cnt["dropped"],
               "host_tier_ms_per_channel_second": round(host_ms, 3), "host_tier_min_ms": round(min(hw), 3), "host_tier_max_ms": round(max(hw), 3),
               "host_tier_ms_for_these_channels": round(host_ms * nch, 1), "host_tier_ok_one_channel": hok}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


if __name__ == "__main__":
    main()
