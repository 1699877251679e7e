"""Writes tests/golden/dropf32_*.npz: stdout, stderr and exit code of the reference's dropsonde/rd94rd41drop.c behind the reference's iq_dec
(oracle/_ref/iq_dec as build() made it) on the float32 captures of tests/dropf32_cases.py:

    iq_dec --FM --lpFM --wav --bo 16 --iq <fq> - <sr> 32 | rd94rd41drop <argv>

The decoder is compiled with its Makefile's flags (-O3 -w) and -DVER_JSN_STR="oracle" into a temporary directory that is removed afterwards;
only data is kept: generator parameters, --iq, argument lists, stdout, stderr, exit codes.  A second build with -O2 runs every argument list
too; a case on which the two builds print different text is reported and not written.  dropf32_emu.npz holds iq_dec's int16 output on the
capture of tests/test_fm_front_emu.py.  The captures themselves are regenerated from their seeds by tools/synth.py.

    python tools/make_golden_drop_f32.py path/to/reference/checkout [case ...]
"""
from __future__ import annotations

import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import dropf32_cases as cases  # noqa: E402

IQ_DEC = os.path.join(ROOT, "oracle", "_ref", "iq_dec")


def iq_dec(data: bytes, sr: int, fq: float) -> bytes:
    r = subprocess.run([IQ_DEC] + cases.iq_dec_args(sr, fq), input=data, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-300:]
    return r.stdout


def main(ref_root: str, only=()) -> None:
    src = os.path.join(ref_root, "dropsonde", "rd94rd41drop.c")
    tmp = tempfile.mkdtemp(prefix="dropf32ref_")
    try:
        exe = os.path.join(tmp, "rd94rd41drop")
        subprocess.check_call(["gcc", "-O3", "-w", '-DVER_JSN_STR="oracle"', "-o", exe, src, "-lm"])
        exe_o2 = os.path.join(tmp, "rd94rd41drop_o2")
        subprocess.check_call(["gcc", "-O2", "-w", '-DVER_JSN_STR="oracle"', "-o", exe_o2, src, "-lm"])
        for name, case in list(cases.CASES.items()) + list(cases.WIDE.items()):
            if only and name not in only:
                continue
            mid = iq_dec(cases.samples(case["gen"]).astype("<f4").tobytes(), case["gen"]["sr"], case["fq"])
            outs, errs, rcs = [], [], []
            for argv in case["argv"]:
                r = subprocess.run([exe] + list(argv), input=mid, capture_output=True, timeout=600)
                assert r.returncode == 0, (name, argv, r.returncode, r.stderr[-300:])
                r2 = subprocess.run([exe_o2] + list(argv), input=mid, capture_output=True, timeout=600)
                if r2.stdout != r.stdout:
                    print("!!", name, argv, "the -O3 and the -O2 build disagree: not written", flush=True)
                    break
                outs.append(r.stdout)
                errs.append(r.stderr)
                rcs.append(r.returncode)
            else:
                dst = os.path.join(ROOT, "tests", "golden", "dropf32_%s.npz" % name)
                np.savez_compressed(dst, params=np.array(json.dumps(case["gen"])), fq=np.array(float(case["fq"])),
                                    argv=np.array([json.dumps(a) for a in case["argv"]]),
                                    stdout=np.frombuffer(b"".join(outs), np.uint8), lengths=np.array([len(o) for o in outs], np.int64),
                                    stderr=np.frombuffer(b"".join(errs), np.uint8), err_lengths=np.array([len(o) for o in errs], np.int64),
                                    rc=np.array(rcs, np.int64))
                print(name, "lines", [o.count(b"\n") for o in outs], "json", [o.count(b'"type"') for o in outs], "%d bytes" % os.path.getsize(dst), flush=True)
        if not only or "emu" in only:
            case = cases.CASES[cases.EMU_CASE]
            data = cases.samples(case["gen"])[:2 * cases.EMU_N].astype("<f4").tobytes()
            fm = {}
            for i, fq in enumerate(cases.EMU_FQ):
                wav = iq_dec(data, case["gen"]["sr"], fq)
                fm["fm_%d" % i] = np.frombuffer(wav[44:], "<i2").copy()                 # behind --wav's 44-byte header
                assert len(fm["fm_%d" % i]) == cases.EMU_N, len(fm["fm_%d" % i])
            dst = os.path.join(ROOT, "tests", "golden", "dropf32_emu.npz")
            np.savez_compressed(dst, fq=np.array(cases.EMU_FQ, np.float64), **fm)
            print("emu", "%d bytes" % os.path.getsize(dst), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2:])
