"""bench.py --config scan_wide | fsk_mixed: the two BASELINE.json configurations beside the headline (configs[2], configs[3]).

scan_wide   One 10 Msps cs16 stream per GPU -> polyphase channelizer (256 channels x 50 kHz, one pass over the stream) -> the
            dft_detect scanner over all 256 channels (IF-rate float IQ, `--iq --dc`).  Step = 1 s of stream.  value = stream samples/s.
            `brute_force`: the same 256 channels mixed out of the stream one by one (k_mix_decimate_wide, channel stride 0), the form
            round 1 had — what the channelizer replaces.  cpu_baseline: the reference's way, one `dft_detect --IQ fq` process per
            channel reading the stream.
fsk_mixed   1024 channels through the 2-FSK modem (fsk_demod of auto_rx): RS41 at 48000 / 4800 Bd, DFM09 at 50000 / 2500 Bd,
            M10 at 48080 / 9616 Bd in equal parts (auto_rx/autorx/decode.py:895-1130).  Step = 1 s of every channel.  value = IF-rate
            samples/s over all channels.  cpu_baseline: the reference fsk_demod.
Both shard by replication: every rank runs the same workload on its own GPU (no collective exists on these paths).
"""
from __future__ import annotations

import json
import os
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))


def _timed_steps(D, step, steps, warmup, min_seconds=0.0, drain=None, run_n=None):
    """-> (seconds, per-rank seconds, steps timed).  min_seconds: the step count is raised (from a probe of three untimed steps, the same count on every rank) until
    the timed region is at least that long — the sub-configurations of the `--full` line are timed over >= 1 s, not over a few milliseconds.
    drain: called behind the last step of every group of steps, inside the timed region — completes what a pipelined step leaves in flight.
    run_n: instead of `step` / `drain`: run_n(n) does n steps and completes them (a configuration whose steps are driven from several host threads)."""
    drain = drain or (lambda: None)
    if run_n is None:
        def run_n(n):
            for _ in range(n):
                step()
            drain()
    run_n(warmup)
    if min_seconds > 0:
        D.barrier()
        t0 = time.perf_counter()
        run_n(3)
        D.barrier()
        probe, _ = D.finish_times(time.perf_counter() - t0)
        steps = max(steps, int(min_seconds / max(probe / 3, 1e-6)) + 1)
    D.barrier()
    t0 = time.perf_counter()
    run_n(steps)
    D.barrier()
    dt, per = D.finish_times(time.perf_counter() - t0)
    return dt, per, steps


def bench_scan_wide(args, D, short=False):
    torch = D.torch
    from tools import synth
    from radiosonde_auto_rx_amd.chan import Channelizer
    from radiosonde_auto_rx_amd.scan import Scanner, IFIQ, BBIQ
    from bench import _time_reference, _traffic
    sr, M, Dd, P = 10_000_000, 256, 200, 16
    steps = args.steps or (12 if short else 40)
    warmup = 2 if args.warmup is None else args.warmup
    spacing = sr / M
    # a stream with a dozen sondes on the channel raster (+- a few kHz), 1 s, repeated every step
    kinds = ("rs41", "dfm", "m10")
    sig = [dict(kind=kinds[i % 3], fq=((-100 + 17 * i) * spacing + 700.0 * (i % 5 - 2)) / sr, t_first=0.03 + 0.02 * i, amp=0.05) for i in range(12)]
    x = synth.wideband_capture(sr, 1.0, sig, noise_sigma=0.01, seed=3)
    wb = torch.from_numpy(x).to(D.dev)
    ch = Channelizer(sr, M, Dd, P, max_chunk=sr, device=D.local_rank)
    if_sr = int(ch.out_rate)
    outs = [torch.zeros(M, ch.max_frames, 2, dtype=torch.float32, device=D.dev) for _ in range(2)]
    torch.cuda.synchronize()                     # torch's fill must be over before another stream writes the buffer
    sc = Scanner(if_sr, n_channels=M, iq_mode=IFIQ, dc=True, cont=True, max_chunk=ch.max_frames, device=D.local_rank, bits=32)
    found = []
    ch_stream = ch.stream()
    # Two stages on two streams, one step apart: while the scanner works on the channels of the stream second before (and its call waits for the
    # prefilter's and the exact kernel's results on the host), the channelizer already produces this second's.  A step is still one pass of each stage
    # over one second of stream; the channelizer's output alternates between two buffers.  SONDE_SCAN_WIDE_SERIAL=1: the stages one after the other.
    serial = os.environ.get("SONDE_SCAN_WIDE_SERIAL") is not None
    state = {"k": 0, "n": 0}

    def step():
        k = state["k"]
        if serial:
            n = ch.process_device(wb.data_ptr(), sr, outs[0].data_ptr(), ch.max_frames)
            sc.wait_stream(ch_stream)                         # the scanner runs on its own stream: ordered behind the channelizer on the device, no host wait
            sc.process_device(outs[0].data_ptr(), ch.max_frames, n)
            found.append(sc.fetch())
            return
        sc.wait_stream(ch_stream)                             # everything the channelizer has queued so far: the buffer the scanner is about to read
        n_prev = state["n"]
        state["n"] = ch.process_device(wb.data_ptr(), sr, outs[k & 1].data_ptr(), ch.max_frames)       # (queued; its own stream)
        if n_prev > 0:
            sc.process_device(outs[(k - 1) & 1].data_ptr(), ch.max_frames, n_prev)     # returns when its detections are on the host
            found.append(sc.fetch())
        state["k"] = k + 1

    dt, per, steps = _timed_steps(D, step, steps, warmup, 1.15 if not args.steps else 0.0)
    det = found[-1]
    kern = {k: sc.kernel_ms(k) for k in ("front_end", "scan_if", "scan_pre", "scan_corr")}
    pre_pairs, exact_pairs = sc.kernel_ms("pre_pairs")[0], sc.kernel_ms("exact_pairs")[0]
    ch.sync()                                                 # (reads the last launch's events)
    ch_ms, ch_n = ch.kernel_ms()
    value = D.world * sr * steps / dt / 1e6
    # dominant kernel: the prefilter k_scan_pre (matrix cores, f16 in / f32 accumulate).  Algorithmic flops per launch = 2 x the multiply-adds of
    # the FM low-pass (window x taps) and of the header correlation ((K+1) x L) of every (window, template) — the zero half of the Toeplitz
    # fragments the MFMAs also multiply is not counted.
    info = sc.info
    Ls = [info["L"][j] for j in range(16) if j not in (11, 14)]
    windows = pre_pairs / max(1, len(Ls))
    flops_per_launch = windows * sum(2.0 * (info["K"] + 1) * L + 2.0 * (info["K"] + L) * info["lpfm_taps"] for L in Ls)
    pre_ms = kern["scan_pre"][0]
    achieved = flops_per_launch / (pre_ms * 1e-3) / 1e12 if pre_ms > 0 else 0.0
    out_json = None
    # ONE 10 Msps stream is 40 MB per second of signal — 0.003 of the HBM roofline however it is processed (verdict round 5, weak #7).  Whether the step above is latency
    # (a chain of short launches with host decisions between them) or work shows with several independent streams on the GPU: S receivers (channelizer + scanner each, their
    # own streams and buffers), every one driven by a host thread of its own (the C calls release the GIL), one second of every stream per step.  Measured: 1.57 ms per
    # stream-second with 4 streams, 1.34 with 8, against 1.54 alone — it is work: the channelizer (0.7-1.1 ms), k_scan_pre (0.69 ms: 45 000 workgroups on 1024 slots) and
    # k_scan_if (0.36 ms) of ONE stream already fill the chip launch by launch; what the pipelined single-stream step hides is their sum, not idle time.
    batch = None
    if D.world == 1 and not getattr(args, "no_extras", False):
        from concurrent.futures import ThreadPoolExecutor
        S = int(os.environ.get("SONDE_SCAN_WIDE_STREAMS", "8"))
        recv = []
        for i in range(S):
            c2 = Channelizer(sr, M, Dd, P, max_chunk=sr, device=D.local_rank)
            o2 = torch.zeros(M, c2.max_frames, 2, dtype=torch.float32, device=D.dev)
            s2 = Scanner(if_sr, n_channels=M, iq_mode=IFIQ, dc=True, cont=True, max_chunk=c2.max_frames, device=D.local_rank, bits=32)
            recv.append((c2, o2, s2, c2.stream()))
        torch.cuda.synchronize()

        def one(r):
            c2, o2, s2, st2 = r
            n2 = c2.process_device(wb.data_ptr(), sr, o2.data_ptr(), c2.max_frames)
            s2.wait_stream(st2)
            s2.process_device(o2.data_ptr(), c2.max_frames, n2)
            return len(s2.fetch())
        with ThreadPoolExecutor(max_workers=S) as pool:
            for _ in range(3):
                list(pool.map(one, recv))
            torch.cuda.synchronize()
            nb, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < 1.0:
                list(pool.map(one, recv)); nb += 1
            torch.cuda.synchronize()
            dtb = (time.perf_counter() - t0) / nb
        for c2, o2, s2, _ in recv:
            s2.close(); c2.close()
        del recv
        batch = {"streams": S, "ms_per_step": round(dtb * 1e3, 3), "ms_per_stream_second": round(dtb * 1e3 / S, 3), "value": round(S * sr / dtb / 1e6, 1), "unit": "Msamples/s", "steps": nb}
    # A/B: the 256 channels mixed out of the stream one by one
    sw = Scanner(sr, fq=[synth.snap_fq(ch.channel_freq(k) / sr, sr) for k in range(M)], iq_mode=BBIQ, dc=True, cont=True, max_chunk=2_000_000, device=D.local_rank)
    torch.cuda.synchronize()
    for _ in range(2):
        t0 = time.perf_counter()
        for part in range(5):
            sw.process_device(wb.data_ptr() + 4 * part * 2_000_000, 0, 2_000_000)
        sw.fetch()
        torch.cuda.synchronize()
        brute = time.perf_counter() - t0
    brute_k = {k: sw.kernel_ms(k) for k in ("front_end", "scan_if", "scan_corr")}
    sw.close()
    if D.rank == 0:
        out_json = {
            "metric": "wideband IQ Msamples/s channelized (256 ch polyphase) and scanned (dft_detect, 14 templates per channel)",
            "value": round(value, 1), "unit": "Msamples/s", "n_gpus": D.world, "steps": steps, "warmup": warmup,
            "ms_per_step": round(dt / steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "BASELINE configs[2]: one 10 Msps cs16 stream -> 256 x 50 kHz polyphase channels -> dft_detect scan, 1 s of stream per step"
                                   + ("" if serial else "; the two stages run one step apart on two streams (the scanner on the channels of the second before)"),
                       "stages": "serial" if serial else "pipelined",
                       "stream_rate": sr, "channels": M, "if_rate": if_sr, "realtime_factor": round(value * 1e6 / D.world / sr, 2),
                       "detections_last_step": sorted({(d["channel"], d["type"]) for d in det if d["printed"] or d["score"] != 0})[:24],
                       "rank_ms_per_step": [round(t / steps * 1e3, 3) for t in per],
                       "kernels_ms_per_launch": {"channelize": round(ch_ms, 4), **{k: round(v[0], 4) for k, v in kern.items()}},
                       "streams_batch": batch,
                       "brute_force": {"ms_per_stream_second": round(brute * 1e3, 2), "kernels_ms_per_launch": {k: round(v[0], 4) for k, v in brute_k.items()},
                                       "note": "256 per-channel mixer + FIR front ends reading the same stream (k_mix_decimate_wide, 5 calls of 0.2 s)"}},
            "roofline": {"bound": "mfma", "kernel": "k_scan_pre", "achieved": round(achieved, 2), "peak": 2500.0, "unit": "TFLOP/s",
                         "frac": round(achieved / 2500.0, 4), "traffic": None, "avg_launch_ms": round(pre_ms, 4),
                         "pairs_per_launch": round(pre_pairs, 1), "exact_pairs_per_launch": round(exact_pairs, 1),
                         "note": "dense f16 MFMA peak; useful multiply-adds only (FM low-pass + header correlation of every (window, template)); full Toeplitz "
                                 "fragments (32 taps per MFMA), one 16-byte LDS read per MFMA.  The kernel is bound by the vector instructions AROUND the "
                                 "MFMAs (conversion, prefix sums, scores, reductions: ~12 per MFMA), see DESIGN 4.6a.  Pairs within 0.03 "
                                 "of their threshold go on to the reference's own transform network (k_scan_corr: exact_pairs_per_launch)"},
        }
        if D.world == 1 and not args.no_cpu_baseline:
            from oracle import bind
            if bind.have_ref():
                ncores = max(1, min(os.cpu_count() or 1, 8))
                with tempfile.TemporaryDirectory() as td:
                    p = os.path.join(td, "wb.cs16")
                    x[:2 * 2_000_000].tofile(p)                 # 0.2 s of the stream per process pass
                    exe = os.path.join(bind.REFDIR, "dft_detect")
                    cmds = [[exe, "--IQ", repr(ch.channel_freq(10 * k + 3) / sr), "--dc", "-t", "1", "-", str(sr), "16"] for k in range(ncores)]
                    r = _time_reference(cmds, [p] * ncores, 2_000_000, "Msamples/s",
                                        "dft_detect --IQ fq processes, one channel each, over 0.2 s of the 10 Msps stream (channel-samples/s: x1)", getattr(args, "cpu_budget", 12.0))
                r["note"] = "channel-samples per second: one process handles ONE of the 256 channels; divide by 256 for stream samples/s"
                out_json["cpu_baseline"] = r
    sc.close(); ch.close()
    return out_json


def bench_fsk_mixed(args, D, short=False):
    torch = D.torch
    from tools import synth
    from radiosonde_auto_rx_amd.fsk import FskModem
    from bench import _time_reference
    C = args.channels or 1024
    steps = args.steps or (25 if short else 100)
    warmup = 2 if args.warmup is None else args.warmup
    # auto_rx's own argument sets (auto_rx/autorx/decode.py): RS41 :869-907 `-b -5000 -u 5000 --mask 5000 --nsym=300 -p 5`; DFM :1036-1067
    # `-b -5000 -u 5000` with fsk_demod's defaults P = 10 (utils/fsk_demod.c:71), nsym = 50 (fsk.h:46); M10 :1085-1122 `-b -10000 -u 10000 -p 5`
    groups = [("rs41", 48000, 4800, 5, 300, 5000, 5000), ("dfm", 50000, 2500, 10, 50, 0, 5000), ("m10", 48080, 9616, 5, 50, 0, 10000)]
    NB = 16

    def ref_args(P, nsym, mask, lim):
        return ["--cs16", "-b", str(-lim), "-u", str(lim), "-s"] + (["--mask", str(mask)] if mask else []) + ["--nsym=%d" % nsym, "-p", str(P)]
    engines = []
    total_samples = 0
    consumers = {}
    for gi, (kind, Fs, Rs, P, nsym, mask, lim) in enumerate(groups):
        n = C // 3 + (1 if gi < C % 3 else 0)
        caps = []
        for s in range(NB):                                   # NB unique captures per family: frame phase, carrier offset, noise and error count differ, so the channels of a launch do not move in lock step
            if kind == "rs41":
                # (most captures carry bit errors in the frame: the consumer's Reed-Solomon stage has symbols to repair)
                caps.append(synth.rs41_capture(sr=Fs, seconds=1.0, fq=0.0, n_frames=1, t_first=0.03 + 0.023 * s, noise_sigma=0.02 + 0.003 * (s % 4), seed=s, f_offset_hz=150.0 * (s % 4) - 40.0 * (s // 4),
                                               bit_errors=4 * (s % 4)))
            elif kind == "dfm":
                caps.append(synth.dfm_capture(sr=Fs, seconds=1.0, fq=0.0, noise_sigma=0.02 + 0.004 * (s % 3), seed=10 + s, t_first=0.1 + 0.0119 * s))
            else:
                caps.append(synth.m10_capture(sr=Fs, seconds=1.0, fq=0.0, noise_sigma=0.02 + 0.004 * (s % 3), seed=20 + s, baud=float(Rs), dev_hz=Rs / 2.0,     # tones Rs apart, as fsk_demod's estimator assumes
                                              t_first=0.35 + 0.017 * s,
                                              frame_fn=lambda k, s=s: synth.m10_frame(k, rng=np.random.default_rng(900 + 10 * s + k))))          # real frames: the checksum stage has something to accept
        L = min(len(c) for c in caps)
        X = torch.from_numpy(np.stack([caps[c % NB][:L] for c in range(n)])).to(D.dev)
        md = FskModem(Fs, Rs, n_channels=n, P=P, nsym=nsym, mask=mask, lower=-lim, upper=lim, max_chunk=Fs, device=D.local_rank)
        engines.append((kind, Fs, Rs, n, X, md, caps[0], ref_args(P, nsym, mask, lim)))
        # the consumers of auto_rx's pipes on the device (sonde_softin_dev_*): decode.py:901-909 `fsk_demod ... | rs41mod --softin -i` (header search, bit loop, rs41_ecc --ecc2),
        # :1067 `... | dfm09mod --ecc --auto --softin` (two symbols per bit, eight frames per hit, Hamming(8,4)), :1120 `... | m10mod --softin -i` (differential code, checksum)
        from radiosonde_auto_rx_amd.fsk import SoftinDev
        consumers[kind] = dict(sf=SoftinDev(n, ecc=2, inv=True) if kind == "rs41" else SoftinDev(n, kind="dfm", ecc=1, inv=False, auto=True) if kind == "dfm" else SoftinDev(n, kind="m10", ecc=0, inv=True),
                               caps=caps, binary={"rs41": "rs41mod", "dfm": "dfm09mod", "m10": "m10mod"}[kind],
                               args={"rs41": ["--softin", "-i", "-r", "--ecc2"], "dfm": ["--softin", "-r", "--ecc", "--auto"], "m10": ["--softin", "-i", "-r", "-v"]}[kind],
                               fetch={"rs41": "fetch", "dfm": "fetch_dfm", "m10": "fetch_m10"}[kind], ok=0, checked=0)
        total_samples += n * (L // 2)

    # untimed, before anything else: the first second of every channel against the compiled reference modem (oracle/_ref/fsk_demod, test infrastructure) —
    # channels fed the same capture must give the same soft decisions bit for bit, and each capture's must equal the reference's stdout
    verified, checked, vnote = 0, 0, "compiled reference not present"
    try:
        from oracle import bind
        have_ref = bind.have_ref()
    except Exception:
        have_ref = False
    fnote = "compiled reference not present"
    for kind, Fs, Rs, n, X, md, _cap, rargs in engines:
        md.process_device(X.data_ptr(), X.shape[1] // 2, X.shape[1] // 2)
        sds = [md.fetch(c)[0] for c in range(n)]
        refs = {}
        if have_ref:
            import subprocess
            exe = os.path.join(bind.REFDIR, "fsk_demod")
            for b in range(min(NB, n)):
                argv = [exe] + rargs + ["2", str(Fs), str(Rs), "-", "-"]
                r = subprocess.run(argv, input=X[b].cpu().numpy().tobytes(), capture_output=True, timeout=120)
                refs[b] = np.frombuffer(r.stdout, np.float32)
            vnote = "first second of every channel: soft decisions equal to channel (c mod %d) bit for bit, and that channel's to oracle/_ref/fsk_demod -s within 1e-6 of the RMS, same signs" % NB
        for c in range(n):
            checked += 1
            a0 = sds[c % NB].ravel(); ac = sds[c].ravel()
            ok = ac.shape == a0.shape and np.array_equal(ac, a0)
            if ok and have_ref:
                w = refs[c % NB][:len(ac)]
                rms = float(np.sqrt(np.mean(w.astype(np.float64) ** 2))) or 1.0
                ok = len(w) == len(ac) and len(ac) > 0 and float(np.sqrt(np.mean((ac.astype(np.float64) - w) ** 2))) < 1e-6 * rms and np.array_equal(ac < 0, w < 0)
            verified += int(ok and have_ref)
        cons = consumers.get(kind)
        if cons is not None:
            # the frames the device consumer completes in the first THREE seconds (the capture three times) against the reference's own pipe on the same samples
            sf = cons["sf"]
            sf.push_fsk(md)
            for _ in range(2):
                md.process_device(X.data_ptr(), X.shape[1] // 2, X.shape[1] // 2)
                sf.push_fsk(md)
            got = {}
            for f in getattr(sf, cons["fetch"])(16 * n):
                got.setdefault(f["channel"], []).append(f["line"].rstrip())
            want = {}
            if have_ref:
                import subprocess
                for b in range(min(NB, n)):
                    p1 = subprocess.run([os.path.join(bind.REFDIR, "fsk_demod")] + rargs + ["2", str(Fs), str(Rs), "-", "-"], input=cons["caps"][b][:X.shape[1]].tobytes() * 3, capture_output=True, timeout=120)
                    p2 = subprocess.run([os.path.join(bind.REFDIR, cons["binary"])] + cons["args"], input=p1.stdout, capture_output=True, timeout=120)
                    want[b] = [l.rstrip() for l in p2.stdout.decode().splitlines()]
                fnote = ("first three seconds of every channel: the frames of the device consumers equal `oracle/_ref/fsk_demod ... | oracle/_ref/{rs41mod --softin -i -r --ecc2, "
                         "dfm09mod --softin -r --ecc --auto, m10mod --softin -i -r -v}` on the same capture, line for line (the frame in progress at the end is the next call's)")
            for c in range(n):
                cons["checked"] += 1
                g = got.get(c, [])
                w = want.get(c % NB, [])
                # every frame the reference prints, in order — only the frame in progress at the end of the third second may still be missing (it is the next call's)
                cons["ok"] += int(have_ref and len(g) >= max(1, len(w) - 1) and g == w[:len(g)])

    # The three modem configurations are three engines with a stream each, driven by one host thread through the two-halves calls.  Per family and second k:
    #   sonde_fsk_wait (k - 1)              the modem's launch of the second before is through (its channel records on the host)
    #   sonde_softin_dev_collect (k - 2)    the frames of the consumer call that ran beside it
    #   sonde_softin_dev_submit_fsk (k - 1) the consumer over launch k - 1's soft decisions, on the consumer's own stream: soft decisions -> frames -> block codes, all in
    #                                       device memory; only the frames come back
    #   sonde_fsk_submit_device (k)         ring copy, launch, the channel records' way back — nothing waits; it runs beside the consumer of k - 1 (the modem keeps the
    #                                       soft decisions of two launches)
    # The families are independent receivers: none waits for another's second.  A step = one second of all channels submitted; everything in flight — the last modem
    # launches and both consumer calls behind them — is completed inside the timed region (`drain`).  One workgroup per channel (three or four waves, 17-41 KB of LDS).
    # (a host thread per family was tried and is slower — 2.17 against 2.03 ms at 1024 channels: the HIP calls of the threads serialise — profiles/r5g_fsk_mixed_host_loop.txt;
    # submission order, profiles/r5f_fsk_mixed_order.txt: up to ~2000 channels the launches do not fill the GPU; beyond, the CUs' LDS is what is contended and the
    # largest footprint (RS41, 40 KB a channel) is best placed first)
    _ord = os.environ.get("SONDE_BENCH_ORDER", "m10,rs41,dfm" if C <= 2048 else "rs41,m10,dfm").split(",")
    order = sorted(engines, key=lambda e: _ord.index(e[0]))
    barrier_every_step = bool(os.environ.get("SONDE_BENCH_FSK_BARRIER"))          # A/B: everything of a step completed before the next one starts
    modem_first = not os.environ.get("SONDE_BENCH_FSK_DECODER_FIRST")             # A/B: round 5's order (decoder of k - 1 submitted before the modem's second k)

    cnt0 = {k: c["sf"].counts() for k, c in consumers.items()}
    launched, consuming = set(), set()

    def drain():
        for kind, Fs, Rs, n, X, md, _, _ in order:
            sf = consumers[kind]["sf"]
            if kind in launched:
                md.wait()
            if kind in consuming:
                sf.collect()
            if kind in launched:
                sf.submit_fsk(md)
                sf.collect()
        launched.clear(); consuming.clear()
        torch.cuda.synchronize()

    def step():
        for kind, Fs, Rs, n, X, md, _, _ in order:
            sf = consumers[kind]["sf"]
            was = kind in launched
            if was:
                md.wait()
            if modem_first:                                   # the modem's next second first: its stream does not wait for the decoder's bookkeeping on the host
                md.submit_device(X.data_ptr(), X.shape[1] // 2, X.shape[1] // 2)
            if kind in consuming:
                sf.collect()
            if was:
                (sf.submit_fsk_behind if modem_first else sf.submit_fsk)(md)
                consuming.add(kind)
            if not modem_first:
                md.submit_device(X.data_ptr(), X.shape[1] // 2, X.shape[1] // 2)
            launched.add(kind)
        if barrier_every_step:
            drain()

    dt, per, steps = _timed_steps(D, step, steps, warmup, 1.15 if not args.steps else 0.0, drain=drain)
    value = D.world * total_samples * steps / dt / 1e6
    kern = {kind: md.kernel_ms() for kind, _, _, _, _, md, _, _ in engines}
    cnt1 = {k: c["sf"].counts() for k, c in consumers.items()}
    for k, c in consumers.items():
        getattr(c["sf"], c["fetch"])(1 << 20)                 # (drop the queued records)
    # dominant kernel k_fsk_stream: algorithmic bytes = 4 B per complex cs16 input sample (soft decisions out: 4 B per symbol)
    # the three launches overlap: the rate follows from the step time, not from the sum of the kernels' own durations
    achieved = total_samples * 4 / (dt / steps) / 1e9
    # HBM bytes of the three launches of a step from the committed counter passes of this command (tools/profile_round.sh), when taken on these launch geometries
    from bench import _traffic
    parts = [_traffic("fsk_" + kind, n * (X.shape[1] // 2) * 4) for kind, Fs, Rs, n, X, md, _, _ in engines]
    traffic = round(sum(p[0] for p in parts), 4) if all(p[0] is not None for p in parts) else None
    traffic_note = ("GB per step over the three launches (4 B per lane loads: FETCH_SIZE taken x 2 as for a wide stream — uncalibrated for this width, an upper bound; the raw "
                    "counters are in profiles/%s_fsk_{rs41,dfm,m10}_traffic.json): the input is read once, the soft decisions written once" % __import__("bench").PROFILE_TAG) if traffic is not None else None
    out = None
    if D.rank == 0:
        out = {
            "metric": "IF-rate IQ Msamples/s through the 2-FSK modem (fsk_demod path), mixed RS41 / DFM09 / M10 channels",
            "value": round(value, 1), "unit": "Msamples/s", "n_gpus": D.world, "steps": steps, "warmup": warmup,
            "ms_per_step": round(dt / steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "BASELINE configs[3]: %d channels per GPU, RS41 48000/4800, DFM09 50000/2500, M10 48080/9616 in equal parts, "
                                   "fsk_demod --cs16 -s with auto_rx's argument sets (decode.py:901 RS41 `-b -5000 -u 5000 --mask 5000 --nsym=300 -p 5`; :1048 DFM "
                                   "`-b -5000 -u 5000`, defaults P 10 / nsym 50; :1120 M10 `-b -10000 -u 10000 -p 5`, nsym 50), 1 s per channel per step" % C,
                       "fsk_demod_args": {g[0]: " ".join(ref_args(*g[3:])) for g in groups},
                       "channels_per_gpu": C, "realtime_channels": round(value * 1e6 / D.world / (total_samples / C), 1) if total_samples else 0,
                       "rank_ms_per_step": [round(t / steps * 1e3, 3) for t in per],
                       "kernel_ms_per_launch": {k: round(v[0], 4) for k, v in kern.items()},
                       "verified_channels": verified, "checked_channels": checked, "verify_note": vnote,
                       "consumers": {
                           "what": "the decoders behind the modem on the device, inside the timed step (sonde_softin_dev_*): rs41mod --softin -i --ecc2 (header search, bit loop, rs41_ecc), "
                                   "dfm09mod --softin --ecc --auto (two symbols per bit, eight frames per hit, Hamming(8,4)), m10mod --softin -i (differential code, checkM10); "
                                   "frames_ok = accepted by the block code / checksum",
                           **{k: {"frames_decoded": cnt1[k]["frames"] - cnt0[k]["frames"], "frames_ok": cnt1[k]["ecc_ok"] - cnt0[k]["ecc_ok"],
                                  "frames_repaired": cnt1[k]["repaired"] - cnt0[k]["repaired"], "symbols_or_codewords_repaired": cnt1[k]["symbols"] - cnt0[k]["symbols"],
                                  "frames_dropped": cnt1[k]["dropped"] - cnt0[k]["dropped"], "verified_channels": consumers[k]["ok"], "checked_channels": consumers[k]["checked"]} for k in consumers},
                           "verify_note": fnote},
                       "step": ("one second of all channels submitted; the three families are independent receivers — a family's consumer call over second k - 1 runs beside its "
                                "modem launch of second k (own stream; the modem keeps two launches' soft decisions), no family waits for another's; all work in flight is "
                                "completed inside the timed region" if not barrier_every_step else
                                "one second of all channels, every family's modem and consumer completed before the next step starts (SONDE_BENCH_FSK_BARRIER)"),
                       "soft_decisions": "stay in device memory (copied to the host only when sonde_fsk_fetch asks for them): the consumers read them there"},
            "roofline": {"bound": "hbm", "kernel": "k_fsk_wave", "achieved": round(achieved, 2), "peak": 8000.0, "unit": "GB/s", "frac": round(achieved / 8000.0, 5),
                         "traffic": traffic, "traffic_note": traffic_note, "note": "4 B per complex input sample over the three (overlapping) launches; one workgroup per channel: a walker wave on the serial "
                                                  "oscillator recurrence (one dependent complex multiply per sample, as in the reference: ~31 cycles per sample, 0.6 ms per second of "
                                                  "signal whatever the channel count), worker / estimator / finisher waves beside it, one barrier per 128-sample piece: bound by that "
                                                  "chain and by the waves' own instruction latency, not by memory — see DESIGN.md 4.7 and profiles/r5*"},
        }
        if D.world == 1 and not args.no_cpu_baseline:
            from oracle import bind
            if bind.have_ref():
                ncores = max(1, min(os.cpu_count() or 1, 8))
                with tempfile.TemporaryDirectory() as td:
                    cmds, inputs, units = [], [], 0
                    exe = os.path.join(bind.REFDIR, "fsk_demod")
                    for k in range(ncores):
                        kind, Fs, Rs, n, X, md, cap, rargs = engines[k % 3]
                        p = os.path.join(td, f"{kind}{k}.cs16")
                        with open(p, "wb") as f:
                            for _ in range(20):
                                f.write(cap.tobytes())
                        cmds.append([exe] + rargs + ["2", str(Fs), str(Rs), "-", "-"])
                        inputs.append(p); units += 20 * (len(cap) // 2)
                    r = _time_reference(cmds, inputs, units / ncores, "Msamples/s", "fsk_demod processes (RS41 / DFM / M10 settings in turn) over 20 s of IF-rate cs16", getattr(args, "cpu_budget", 12.0))
                out["cpu_baseline"] = r
    for c in consumers.values():
        c["sf"].close()
    for e in engines:
        e[5].close()
    return out


MIX_PATTERN = ("rs41", "dfm", "rs41", "m10", "rs41", "dfm", "rs41", "m10", "dfm", "rs41")      # 50 % RS41, 30 % DFM09, 20 % M10, interleaved: the type is a property of the channel
MIX_BANK = 16                # unique captures per family (carrier, frame phase, carrier offset, noise and error count differ: channels of a launch do not move in lock step)
MIX_REF = {"rs41": ("rs41mod", ["-r", "--ecc2"]), "dfm": ("dfm09mod", ["-r", "--ecc"]), "m10": ("m10mod", ["-r", "-v"])}


def mixed_bank(SR=2_400_000, n=MIX_BANK):
    """-> {kind: (fqs, captures)}: n one-second captures per family at 2.4 Msps, seeded"""
    from concurrent.futures import ThreadPoolExecutor
    from tools import synth
    rng = np.random.default_rng(4242)
    jobs = []
    for kind in ("rs41", "dfm", "m10"):
        for b in range(n):
            fq = synth.snap_fq(float(rng.uniform(-0.4, 0.4)), SR)
            jobs.append((kind, b, fq))

    def make(job):
        kind, b, fq = job
        if kind == "rs41":
            return synth.rs41_capture(sr=SR, seconds=1.0, fq=fq, n_frames=1, t_first=0.05 + 0.021 * b, seed=300 + b, noise_sigma=0.01 + 0.004 * (b % 5),
                                      bit_errors=(0, 0, 6, 14, 0, 3, 30, 0)[b % 8], f_offset_hz=60.0 * (b % 7 - 3))
        if kind == "dfm":
            return synth.dfm_capture(sr=SR, seconds=1.0, fq=fq, noise_sigma=0.02 + 0.01 * (b % 4), seed=310 + b, bit_errors_per_frame=b % 3, t_first=0.02 + 0.0137 * b)
        return synth.m10_capture(sr=SR, seconds=1.0, fq=fq, noise_sigma=0.02 + 0.01 * (b % 4), seed=320 + b, t_first=0.1 + 0.027 * b, f_offset_hz=80.0 * (b % 5 - 2),
                                 frame_fn=lambda k, b=b: synth.m10_frame(k, rng=np.random.default_rng(500 + 10 * b + k), good_checksum=(k + b) % 4 != 3))

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        caps = list(ex.map(make, jobs))
    out = {}
    for (kind, b, fq), cap in zip(jobs, caps):
        out.setdefault(kind, ([], []))
        out[kind][0].append(fq); out[kind][1].append(cap)
    return out


def _dfm_undecodable(line):
    """a `dfm09mod -r --ecc` line whose three blocks all failed the Hamming check"""
    return line.count("[NO]") == 3 and "[OK]" not in line and "[KO]" not in line


def cpu_baseline_mixed(bank, shares, SR, budget_s=9.0):
    """The reference decoders on this host's cores at the bench's type mix: every type timed by itself on all cores (N concurrent processes over the same
    captures), combined for the mix — a second of the mix costs sum(share_t / rate_t) seconds of the cores."""
    from bench import _time_reference
    from oracle import bind
    if not bind.have_ref():
        return None
    ncores = max(1, min(os.cpu_count() or 1, 8))
    secs = 6
    rates, samples = {}, []
    with tempfile.TemporaryDirectory() as td:
        for kind, (fqs, caps) in bank.items():
            paths = []
            for b in range(min(len(caps), ncores)):
                p = os.path.join(td, "%s%d.cs16" % (kind, b))
                with open(p, "wb") as f:
                    for _ in range(secs):
                        f.write(caps[b].tobytes())
                paths.append(p)
            exe, a = MIX_REF[kind]
            cmds = [[os.path.join(bind.REFDIR, exe)] + a + ["--IQ", repr(fqs[k % len(paths)]), "--lpIQ", "-", str(SR), "16"] for k in range(ncores)]
            r = _time_reference(cmds, [paths[k % len(paths)] for k in range(ncores)], secs * SR, "Msamples/s", "%s processes" % exe, budget_s / 3)
            rates[kind] = r["value"]; samples.append(r["sample"])
            for p in paths:
                os.remove(p)
    mix = 1.0 / sum(shares[k] / rates[k] for k in rates)
    return dict(value=round(mix, 1), unit="Msamples/s", cores=ncores, kind="reference", per_type={k: round(v, 1) for k, v in rates.items()},
                sample="%d concurrent oracle/_ref processes per type over %d s of the bench's own 2.4 Msps captures (%s); combined at the channel shares %s"
                       % (ncores, secs, "; ".join(samples), {k: round(v, 3) for k, v in shares.items()}))


def bench_mixed_2400k(args, D, short=False):
    """BASELINE configs[4] at the sonde types of configs[3]: channels at the base rate (2.4 Msps IQ each), half of them RS41 (Reed-Solomon (255,231) x 2), 30 % DFM09
    (Hamming(8,4), eight frames per hit), 20 % M10 (differential code, checksum), interleaved, on ONE mixed-type engine (sonde_engine_create_mixed): one decimator launch
    per step over all channels, the IF-rate stages per type on their own streams, every block code on the device, frames fetched one step behind.  A step = one second
    of every channel.  Ranks own contiguous channel blocks; the 32-byte detection summaries are all_gathered from device memory once per step.
    Untimed, first: two seconds of every channel against the compiled reference decoders on the same samples (oracle/_ref, test infrastructure), line for line.
    Extra objects on one GPU: `detect_in_step` (the dft_detect scanner re-scanning a rotating 1/16 of the channels inside every step), `host_decode_ab` (block codes on the
    host inside the fetch), `three_engines_ab` (one engine per type: the round-5 arrangement, three decimator launches per step)."""
    torch = D.torch
    import subprocess
    from radiosonde_auto_rx_amd.engine import Engine, MixedEngine
    from radiosonde_auto_rx_amd import shard
    from bench import _traffic, _stream_probe, _device_clocks, detect_in_step_extra
    SR = 2_400_000
    C = args.channels or 512
    kinds = [MIX_PATTERN[(c + D.rank) % len(MIX_PATTERN)] for c in range(C)]
    bank = mixed_bank(SR)
    seen = {k: 0 for k in bank}
    ch_bank = []
    for kd in kinds:                                                   # the b-th channel of a family decodes capture (b + rank) mod 16
        ch_bank.append((seen[kd] + D.rank) % MIX_BANK); seen[kd] += 1
    ch_fq = [bank[kd][0][b] for kd, b in zip(kinds, ch_bank)]
    n_of = {k: kinds.count(k) for k in bank}
    # resident input [C][2 * SR] int16, rows in the caller's channel order
    order = {"rs41": 0, "dfm": 1, "m10": 2}
    all_caps = torch.from_numpy(np.stack([cap for k in ("rs41", "dfm", "m10") for cap in bank[k][1]])).to(D.dev)
    X = all_caps.index_select(0, torch.tensor([order[kd] * MIX_BANK + b for kd, b in zip(kinds, ch_bank)], device=D.dev)).contiguous()
    del all_caps
    torch.cuda.synchronize()

    def make():
        return MixedEngine(ch_fq, kinds, SR, device=D.local_rank, lp_iq=True, ecc={"rs41": 2, "dfm": 1, "m10": 0}, max_chunk=SR, max_frames=8 * C)

    def lines_of(eng, fin):
        got = {}
        for f in eng.fetch_frames(finish=fin) + eng.fetch_dfm(finish=fin) + eng.fetch_mxx(finish=fin):
            got.setdefault(f["channel"], []).append(f["line"].rstrip())
        return got

    # ---- untimed: two seconds of every channel against the reference decoders
    try:
        from oracle import bind
        have_ref = bind.have_ref()
    except Exception:
        have_ref = False
    verified = {k: 0 for k in bank}
    exact = {k: 0 for k in bank}
    vnote = "compiled reference not present"
    if not getattr(args, "no_verify", False):
        eng = make()
        got = {}
        for sec in range(2):
            eng.process_device(X.data_ptr(), SR, SR)
            for c, ls in lines_of(eng, sec == 1).items():
                got.setdefault(c, []).extend(ls)
        eng.close()
        if have_ref:
            want = {}
            for kind, (fqs, caps) in bank.items():
                exe, a = MIX_REF[kind]
                for b in range(MIX_BANK):
                    r = subprocess.run([os.path.join(bind.REFDIR, exe)] + a + ["--IQ", repr(fqs[b]), "--lpIQ", "-", str(SR), "16"], input=caps[b].tobytes() * 2,
                                       capture_output=True, timeout=300)
                    want[kind, b] = [ln.rstrip() for ln in r.stdout.decode().splitlines()]
            for c, (kd, b) in enumerate(zip(kinds, ch_bank)):
                w, g = want[kd, b], got.get(c, [])
                exact[kd] += int(len(w) >= 1 and g == w)
                verified[kd] += int(len(w) >= 1 and len(g) == len(w) and all(a == q or (kd == "dfm" and _dfm_undecodable(a) and _dfm_undecodable(q)) for a, q in zip(w, g)))
            vnote = ("2 s of every channel + end of input: our text lines == stdout of oracle/_ref/{rs41mod -r --ecc2, dfm09mod -r --ecc, m10mod -r -v} --IQ fq --lpIQ - 2400000 16; "
                     "exact_channels: every line equal; verified_channels: every line equal except DFM lines BOTH sides print with all three blocks [NO] — slices of the gap "
                     "between two transmissions of the 1 s loop (a DFM hit is eight frames = 1.79 s), noise only, where a soft bit at the float noise floor decides a nibble")
        verified = dict(zip(verified, D.sum_ints(*verified.values())))
        exact = dict(zip(exact, D.sum_ints(*exact.values())))

    # ---- timed
    eng = make()
    summary = shard.summary_buffer(C, D.dev)
    eng.set_summary(summary.data_ptr(), D.rank * C)
    snaps = shard.summary_buffer(2 * C, D.dev).view(2, C, shard.SUMMARY_BYTES) if D.dist else None
    snap_next = eng.set_summary_snapshots(snaps.data_ptr()) if snaps is not None else 0
    gathered = [torch.empty_like(summary) for _ in range(D.world)] if D.dist else None
    while eng.samples_to_dc_boundary() < SR:                           # untimed lead-in: from here on every 1 s step is one IQ-DC segment = one decimator launch
        eng.process_device(X.data_ptr(), SR, eng.samples_to_dc_boundary())
    tallies = {k: [0, 0] for k in bank}
    dfm_dt = np.dtype([("h", "<i4", (2,)), ("ecc", "<i4", (3,)), ("rest", "u1", (88,))])
    m10_dt = np.dtype([("h", "<i4", (3,)), ("cs_ok", "<i4"), ("rest", "u1", (136,))])
    state = {"count": False, "calls": 0}

    def fetch(lag):
        fr = eng.fetch_frames_np(lag=lag)
        buf_d, n_d = eng.fetch_dfm_raw(lag=lag)
        buf_m, n_m = eng.fetch_m10_raw(lag=lag)
        if state["count"]:
            tallies["rs41"][0] += len(fr); tallies["rs41"][1] += int((fr["ecc"] >= 0).sum())
            if n_d:
                a = np.frombuffer(buf_d, dfm_dt, n_d)
                tallies["dfm"][0] += n_d; tallies["dfm"][1] += int((a["ecc"] >= 0).all(axis=1).sum())
            if n_m:
                a = np.frombuffer(buf_m, m10_dt, n_m)
                tallies["m10"][0] += n_m; tallies["m10"][1] += int((a["cs_ok"] != 0).sum())
        return fr

    # frames are fetched one step behind, like the headline's (two steps behind is slower with the groups' stages in shared launches, faster with a stream per
    # group: profiles/r6a_mixed_lag_ab.txt; and the engine keeps two summary snapshot halves, so ranks that gather them cannot go further back than one)
    LAG = int(os.environ.get("SONDE_MIXED_LAG", "1"))

    def step():
        eng.process_device(X.data_ptr(), SR, SR)
        state["calls"] += 1
        fr = fetch(LAG)
        if D.dist and state["calls"] >= 2:                             # 32 B per channel over RCCL, device to device: the snapshot call k-1 left while call k runs
            shard.gather_summaries(D.dist, snaps[(snap_next + state["calls"] - 2) & 1], D.world, gathered)
        return fr

    def drain():
        fetch(0)
        eng.sync()
        torch.cuda.synchronize()

    steps0 = args.steps or 8
    warm = 3 if args.warmup is None else args.warmup
    for _ in range(warm):
        step()
    drain()
    stream_gbps = _stream_probe(X.data_ptr(), int(X.numel()) * X.element_size())
    clocks0 = _device_clocks()
    eng.profile(1)                                                     # HIP events around the decimator only (2 per step), on the stream it runs on
    min_s = 1.15 if not args.steps else 0.0
    if min_s:                                                          # probe (untimed, uncounted): how many steps make a second
        D.barrier(); t0 = time.perf_counter()
        for _ in range(3):
            step()
        drain(); D.barrier()
        probe, _ = D.finish_times(time.perf_counter() - t0)
        steps0 = max(steps0, int(min_s / max(probe / 3, 1e-6)) + 1)
    state["count"] = True
    dt, per_rank, nsteps = _timed_steps(D, step, steps0, 0, 0.0, drain=drain)
    state["count"] = False
    clocks1 = _device_clocks()
    per = dt / nsteps
    md_ms, md_n = eng.kernel_ms("mix_decimate")
    eng.profile(0)
    counts = {k: (v[0] / nsteps, v[1] / nsteps) for k, v in tallies.items()}
    rec = shard.decode_summaries(summary)

    extras = {}
    if D.world == 1 and not getattr(args, "no_extras", False):
        # per-kernel table (untimed, events around every kernel)
        eng.profile(2)
        for _ in range(10):
            step()
        drain()
        kern = {}
        for k in ("mix_decimate", "if_chain", "header_corr", "framesync", "rs_ecc"):
            ms, n = eng.kernel_ms(k)
            kern[k] = dict(ms_per_step=round(ms * n / 10, 4), launches_per_step=n / 10)
        eng.profile(0)
        extras["kernels"] = kern

        def eng_step():
            eng.process_device(X.data_ptr(), SR, SR)
            return fetch(LAG)
        extras["detect_in_step"] = detect_in_step_extra(D, None, X, ch_fq, C, SR, 1, groups=16, engine_step=eng_step, engine_drain=drain)
        # A/B: the block codes on the host inside the fetch
        drain()
        eng.set_device_ecc(False)
        for _ in range(3):
            step()
        drain()
        dth, _, nh = _timed_steps(D, step, 8, 0, 0.5 if not args.steps else 0.0, drain=drain)
        extras["host_decode_ab"] = {"ms_per_step": round(dth / nh * 1e3, 3), "steps": nh}
        eng.set_device_ecc(True)
    eng.set_summary(0)
    eng.close()
    if D.world == 1 and not getattr(args, "no_extras", False):
        # A/B: one engine per type (round 5): three decimator launches per step
        idx = {k: [c for c, kd in enumerate(kinds) if kd == k] for k in bank}
        Xs = {k: X.index_select(0, torch.tensor(v, device=D.dev)).contiguous() for k, v in idx.items()}
        torch.cuda.synchronize()
        e3 = {k: Engine([ch_fq[c] for c in idx[k]], SR, device=D.local_rank, lp_iq=True, sonde=k, ecc={"rs41": 2, "dfm": 1, "m10": 0}[k], max_chunk=SR, max_frames=8 * len(idx[k]))
              for k in bank}

        def step3():
            for k in ("rs41", "dfm", "m10"):
                e3[k].process_device(Xs[k].data_ptr(), SR, SR)
            e3["rs41"].fetch_frames_np(); e3["dfm"].fetch_dfm_raw(); e3["m10"].fetch_m10_raw()

        def drain3():
            for e in e3.values():
                e.sync()
            torch.cuda.synchronize()
        for _ in range(3):
            step3()
        drain3()
        dt3, _, n3 = _timed_steps(D, step3, 8, 0, 0.5 if not args.steps else 0.0, drain=drain3)
        extras["three_engines_ab"] = {"ms_per_step": round(dt3 / n3 * 1e3, 3), "steps": n3}
        for e in e3.values():
            e.close()
        del Xs
    total = C * SR
    achieved = (total * 4 * md_n) / (md_ms * md_n / 1e3) / 1e9 if md_ms > 0 and md_n > 0 else 0.0
    traffic, traffic_src = _traffic("mix_decimate", total * 4)
    out = None
    if D.rank == 0:
        out = {
            "metric": "IQ Msamples/s demodulated + block-decoded, mixed RS41 / DFM09 / M10 channels at the base rate", "value": round(D.world * total / per / 1e6, 1), "unit": "Msamples/s",
            "n_gpus": D.world, "steps": nsteps, "ms_per_step": round(per * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "BASELINE configs[4] at configs[3]'s type mix: %d channels x 2.4 Msps cs16 IQ per GPU on ONE mixed-type engine — %d RS41 (rs41mod --ecc2), %d DFM09 "
                                   "(dfm09mod --ecc), %d M10, interleaved — one decimator launch per step, IF-rate stages per type, block codes on the device; 1 s per channel per step"
                                   % (C, n_of["rs41"], n_of["dfm"], n_of["m10"]),
                       "channels": n_of, "unique_captures_per_family": MIX_BANK, "realtime_channels": round(D.world * total / per / SR, 1), "timed_seconds": round(dt, 3), "frame_fetch_lag": LAG,
                       "rank_ms_per_step": [round(t / nsteps * 1e3, 3) for t in per_rank],
                       "frames_per_step": {k: round(v[0], 1) for k, v in counts.items()},
                       "frames_ok_per_step": {k: round(v[1], 1) for k, v in counts.items()},
                       "frames_ok_means": "rs41: rs41_ecc() >= 0; dfm: hamming() >= 0 in all three blocks; m10: checksum equal",
                       "summary_records": {"channels_with_frames": int((rec["frames"] > 0).sum())},
                       "verified_channels": verified, "exact_channels": exact, "checked_channels": {k: D.world * v for k, v in n_of.items()}, "verify_note": vnote},
            "roofline": {"bound": "hbm", "kernel": "k_mix_decimate50", "achieved": round(achieved, 1), "peak": 8000.0, "unit": "GB/s", "frac": round(achieved / 8000.0, 4),
                         "measured_stream_GBps": round(stream_gbps, 1) if stream_gbps else None, "frac_of_measured": round(achieved / stream_gbps, 4) if stream_gbps else None,
                         "traffic": traffic, "traffic_note": traffic_src, "algorithmic_gb_per_launch": round(total * 4 / 1e9, 3), "avg_launch_ms": round(md_ms, 4), "launches": md_n,
                         "step_frac": round(total * 4 / per / 8e12, 4), "clocks_mhz": {"before": clocks0, "after": clocks1},
                         "note": "ONE k_mix_decimate50 launch per step over all channels of all types (the same kernel and launch geometry as the headline's); achieved = 4 B x complex "
                                 "samples of the timed launches / their HIP-event time on the stream they ran on; step_frac = the same bytes over the whole step"},
        }
        out.update(extras)
    if D.world == 1 and not getattr(args, "no_cpu_baseline", False):
        cb = cpu_baseline_mixed(bank, {k: n_of[k] / C for k in n_of}, SR, getattr(args, "cpu_budget", None) or 9.0)
        if cb:
            out["cpu_baseline"] = cb
    del X
    torch.cuda.empty_cache()
    return out


def side_paths(D, caps, fqs, C=64, steps=12):
    """What the input forms and options beside the headline's cost (verdict round 5, weak #6): the same RS41 step over C channels x 1 s with float32 samples (k_mix_f32 /
    k_decimate_f32), unsigned 8-bit samples (k_u8_to_s16 in front of the cs16 kernels), --dc (AFC feedback: the host synchronises once per repair round) and with the C
    channels mixed out of ONE 10 Msps stream (channel stride 0, k_mix_decimate_wide, D = 200) — each in ms per channel-second beside the cs16 path at the same C."""
    torch = D.torch
    from tools import synth
    from radiosonde_auto_rx_amd.engine import Engine
    SR = 2_400_000
    nb = len(caps)
    x16 = torch.from_numpy(np.stack([caps[c % nb] for c in range(C)])).to(D.dev)
    ch_fq = [fqs[c % nb] for c in range(C)]
    out = {"channels": C}

    def timed(eng, ptr, stride, n):
        for _ in range(3):
            eng.process_device(ptr, stride, n); eng.fetch_frames_np()
        eng.sync(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = 0
        for _ in range(steps):
            eng.process_device(ptr, stride, n); got += len(eng.fetch_frames_np())
        eng.sync(); torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        eng.close()
        return dt, got / steps

    def entry(dt, frames, seconds=1.0):
        return {"ms_per_channel_second": round(dt * 1e3 / (C * seconds), 5), "ms_per_step": round(dt * 1e3, 3), "frames_per_step": round(frames, 1)}
    base, fr = timed(Engine(ch_fq, SR, device=D.local_rank, lp_iq=True, ecc=2, max_chunk=SR, max_frames=4 * C), x16.data_ptr(), SR, SR)
    out["cs16"] = entry(base, fr)
    xf = (x16.to(torch.float32) / 32768.0).contiguous()
    dt, fr = timed(Engine(ch_fq, SR, device=D.local_rank, lp_iq=True, ecc=2, max_chunk=SR, max_frames=4 * C, bits=32), xf.data_ptr(), SR, SR)
    out["f32"] = entry(dt, fr); del xf
    x8 = ((x16.to(torch.int32) >> 8) + 128).to(torch.uint8).contiguous()
    dt, fr = timed(Engine(ch_fq, SR, device=D.local_rank, lp_iq=True, ecc=2, max_chunk=SR, max_frames=4 * C, bits=8), x8.data_ptr(), SR, SR)
    out["u8"] = entry(dt, fr); del x8
    dt, fr = timed(Engine(ch_fq, SR, device=D.local_rank, lp_iq=True, ecc=2, max_chunk=SR, max_frames=4 * C, opt_dc=True), x16.data_ptr(), SR, SR)
    out["dc"] = entry(dt, fr)
    del x16
    wsr = 10_000_000
    sig = [dict(kind="rs41", fq=(-0.3 + 0.6 * i / 11), t_first=0.03 + 0.02 * i, amp=0.05) for i in range(12)]
    wb = torch.from_numpy(synth.wideband_capture(wsr, 1.0, sig, noise_sigma=0.01, seed=5)).to(D.dev)
    wfq = [synth.snap_fq(sig[c % 12]["fq"], wsr) for c in range(C)]
    dt, fr = timed(Engine(wfq, wsr, device=D.local_rank, lp_iq=True, ecc=2, max_chunk=2_000_000, max_frames=4 * C), wb.data_ptr(), 0, 2_000_000)
    out["wide_d200"] = entry(dt, fr, seconds=0.2); out["wide_d200"]["what"] = "%d channels out of ONE 10 Msps stream, 0.2 s per step" % C
    for k in ("f32", "u8", "dc", "wide_d200"):
        out[k]["x_cs16"] = round(out[k]["ms_per_channel_second"] / out["cs16"]["ms_per_channel_second"], 2)
    del wb
    torch.cuda.empty_cache()
    return out


def run(args, D, short=False):
    """short: the reduced runs the `bench.py --full` line carries as its `scan_wide` / `fsk_mixed` objects"""
    if args.config == "mixed_2400k":
        return bench_mixed_2400k(args, D, short)
    return bench_scan_wide(args, D, short) if args.config == "scan_wide" else bench_fsk_mixed(args, D, short)
