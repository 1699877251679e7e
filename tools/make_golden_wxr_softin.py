"""Writes tests/golden/wxr_softin_*.npz: stdout of the reference's weathex/weathex301d.c `--softin` on the synthetic soft-bit streams of tests/wxr_softin_cases.py.

The decoder is compiled as tools/make_golden_wxr.py compiles it — its Makefile's flags (-O3 -w -Ofast) and -DVER_JSN_STR="oracle", into a temporary directory that
is removed afterwards — and a second time with -O2 alone; a case on which the two builds print different text is reported and not written.  Only data is kept: the
stream the decoder read (int8 signs where it is +-1.0 alone, float32 otherwise: exact zeros of both signs, NaNs and soft values of any size), the argument lists and
the stdout of each.

    python tools/make_golden_wxr_softin.py path/to/reference/checkout [case ...]
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
from tests import wxr_softin_cases as cases  # noqa: E402


def main(ref_root: str, only=()) -> int:
    src = os.path.join(ref_root, "weathex", "weathex301d.c")
    tmp = tempfile.mkdtemp(prefix="wxrsoftref_")
    bad = 0
    try:
        exe = os.path.join(tmp, "weathex301d")
        subprocess.check_call(["gcc", "-O3", "-w", "-Ofast", '-DVER_JSN_STR="%s"' % cases.VERSION, "-o", exe, src, "-lm"])
        exe_o2 = os.path.join(tmp, "weathex301d_o2")
        subprocess.check_call(["gcc", "-O2", "-w", '-DVER_JSN_STR="%s"' % cases.VERSION, "-o", exe_o2, src, "-lm"])
        all_cases = cases.cases()
        for name in cases.GOLDEN_CASES:
            if only and name not in only:
                continue
            case = all_cases[name]
            s = np.ascontiguousarray(case["s"], np.float32)
            data = s.astype("<f4").tobytes()
            outs, argvs = [], []
            for argv in case["argv"]:
                argv = ["--softin"] + list(argv)
                r = subprocess.run([exe] + argv, input=data, capture_output=True, timeout=600)
                assert r.returncode == 0, (name, argv, r.stderr[-300:])
                r2 = subprocess.run([exe_o2] + argv, input=data, capture_output=True, timeout=600)
                if r2.returncode != 0 or r2.stdout != r.stdout:
                    print("!!", name, argv, "the -Ofast and the -O2 build disagree: not written", flush=True)
                    bad += 1
                    break
                outs.append(r.stdout); argvs.append(argv)
            else:
                plain = bool(np.all(np.abs(s) == 1.0))
                stream = np.sign(s).astype(np.int8) if plain else s
                dst = cases.golden_path(name)
                np.savez_compressed(dst, soft=stream, argv=np.array([json.dumps(a) for a in argvs]), stdout=np.frombuffer(b"".join(outs), np.uint8),
                                    lengths=np.array([len(o) for o in outs], np.int64))
                print(name, len(s), "bits", stream.dtype, [o.count(b"[OK]") for o in outs], [o.count(b"[NO]") for o in outs], [o.count(b'"type"') for o in outs],
                      "%d bytes" % os.path.getsize(dst), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return bad


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    sys.exit(1 if main(sys.argv[1], sys.argv[2:]) else 0)
