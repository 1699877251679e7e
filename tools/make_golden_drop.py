"""Writes tests/golden/drop_*.npz: stdout, stderr and exit code of the reference's dropsonde/rd94rd41drop.c on the captures of
tests/drop_cases.py, behind the reference's iq_dec / fsk_demod where the case has a front program (oracle/_ref/iq_dec,
oracle/_ref/fsk_demod as build() made them).

The decoder is compiled with its Makefile's flags (-O3 -w) and -DVER_JSN_STR="oracle" into a temporary directory that is removed
afterwards; only data is kept: case name, generator parameters, argument lists, stdout, stderr, exit codes, the front program's stderr,
and for the soft-bit cases the sign (-1 / 0 / +1) of every soft bit the reference modem wrote — the decoder looks at nothing else.  A
second build with -O2 runs every argument list too; a case on which the two builds print different text is reported and not written.
A clean case (drop_cases.CLEAN) that gives fewer JSON lines than frames put in (soft cases: than all but the first) is not written
either.  The run time of `iq_dec | rd94rd41drop` per second of signal is printed (one run, one core of the machine that makes the
goldens, not a benchmark).

    python tools/make_golden_drop.py path/to/reference/checkout [case ...]
"""
from __future__ import annotations

import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import drop_cases as cases  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")


def front_end(case, data):
    """what the decoder reads on stdin, the front program's stderr, and its run time"""
    if case["front"] is None:
        return data, b"", 0.0
    exe = os.path.join(REF, "fsk_demod" if case["gen"].get("form") == "soft" else "iq_dec")
    t0 = time.perf_counter()
    r = subprocess.run([exe] + list(case["front"]), input=data, capture_output=True, timeout=600)
    assert r.returncode == 0, (exe, r.stderr[-300:])
    return r.stdout, r.stderr, time.perf_counter() - t0


def main(ref_root: str, only=()) -> None:
    src = os.path.join(ref_root, "dropsonde", "rd94rd41drop.c")
    tmp = tempfile.mkdtemp(prefix="dropref_")
    try:
        exe = os.path.join(tmp, "rd94rd41drop")
        subprocess.check_call(["gcc", "-O3", "-w", '-DVER_JSN_STR="oracle"', "-o", exe, src, "-lm"])
        exe_o2 = os.path.join(tmp, "rd94rd41drop_o2")
        subprocess.check_call(["gcc", "-O2", "-w", '-DVER_JSN_STR="oracle"', "-o", exe_o2, src, "-lm"])
        for name, case in cases.CASES.items():
            if only and name not in only:
                continue
            data = cases.capture(case)
            mid, front_err, t_front = front_end(case, data)
            outs, errs, rcs, secs = [], [], [], []
            for argv in case["argv"]:
                t0 = time.perf_counter()
                r = subprocess.run([exe] + list(argv), input=mid, capture_output=True, timeout=600)
                secs.append(time.perf_counter() - t0)
                assert r.returncode == case.get("rc", 0), (name, argv, r.returncode, r.stderr[-300:])
                r2 = subprocess.run([exe_o2] + list(argv), input=mid, capture_output=True, timeout=600)
                if r2.stdout != r.stdout:
                    print("!!", name, argv, "the -O3 and the -O2 build disagree: not written", flush=True)
                    break
                outs.append(r.stdout)
                errs.append(r.stderr)
                rcs.append(r.returncode)
            else:
                g = case["gen"]
                soft = g.get("form") == "soft"
                if name in cases.CLEAN:
                    want = g.get("n_frames", cases.N_FRAMES) - (1 if soft else 0)
                    got = outs[cases.CLEAN[name]].count(b'"type"')
                    if got < want:
                        print("!!", name, "a clean case with %d of %d JSON lines: not written" % (got, want), flush=True)
                        continue
                extra = {}
                if soft:
                    extra["soft_sign"] = np.sign(np.frombuffer(mid[:len(mid) // 4 * 4], "<f4")).astype(np.int8)
                sig_s = len(data) / (2.0 * (1 if g.get("form") == "cu8" else 2)) / g.get("sr", 48000) if case["front"] else 0.0
                dst = os.path.join(ROOT, "tests", "golden", "drop_%s.npz" % name)
                np.savez_compressed(dst, **extra, params=np.array(json.dumps(case["gen"])), argv=np.array([json.dumps(a) for a in case["argv"]]),
                                    front=np.array(json.dumps(case["front"])), front_stderr=np.frombuffer(front_err, np.uint8),
                                    stdout=np.frombuffer(b"".join(outs), np.uint8), lengths=np.array([len(o) for o in outs], np.int64),
                                    stderr=np.frombuffer(b"".join(errs), np.uint8), err_lengths=np.array([len(o) for o in errs], np.int64),
                                    rc=np.array(rcs, np.int64))
                print(name, "lines", [o.count(b"\n") for o in outs], "json", [o.count(b'"type"') for o in outs],
                      "front %.3fs decoder %.3fs" % (t_front, secs[0]),
                      ("= %.4f s per signal-second" % ((t_front + secs[0]) / sig_s)) if sig_s else "", "%d bytes" % os.path.getsize(dst), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2:])
