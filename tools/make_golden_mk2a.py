"""Writes tests/golden/mk2a_*.npz: stdout and stderr of the reference's mk2a/mk2a1680mod.c on the captures of tests/mk2a_cases.py.

The reference is compiled with its Makefiles' flags (-O3 -w -Ofast, -lm) and -DVER_JSN_STR="oracle" into a temporary directory that is
removed afterwards; only the data (case name, generator parameters, argv, stdout, stderr) is kept.  For the case whose Df field is left
out of the comparison (mk2a_cases.RELAXED) a second build of the reference with -O2 alone runs the first argv too, and its stdout is kept
as stdout_o2: the two builds print different Df digits, which is why that field cannot be compared.  The run time of the reference on each
capture is printed (one run on one core of the machine that makes the goldens; tools/bench_mk2a.py quotes it).

    python tools/make_golden_mk2a.py path/to/reference/checkout
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
from tests import mk2a_cases as cases  # noqa: E402


def main(ref_root: str) -> None:
    src = os.path.join(ref_root, "mk2a", "mk2a1680mod.c")
    tmp = tempfile.mkdtemp(prefix="mk2aref_")
    try:
        exe = os.path.join(tmp, "mk2a1680mod")
        subprocess.check_call(["gcc", "-O3", "-w", "-Wno-unused-variable", "-Ofast", '-DVER_JSN_STR="oracle"', "-o", exe, src, "-lm"])
        exe_o2 = os.path.join(tmp, "mk2a1680mod_o2")
        subprocess.check_call(["gcc", "-O2", "-w", '-DVER_JSN_STR="oracle"', "-o", exe_o2, src, "-lm"])
        for name, case in cases.CASES.items():
            data = cases.capture(case)
            outs, errs, secs = [], [], []
            for argv in case["argv"]:
                t0 = time.perf_counter()
                r = subprocess.run([exe] + list(argv), input=data, capture_output=True, timeout=600)
                secs.append(time.perf_counter() - t0)
                assert r.returncode == 0, (name, argv, r.stderr[-300:])
                outs.append(r.stdout)
                errs.append(r.stderr)
            extra = {}
            if name == cases.RELAXED:
                r = subprocess.run([exe_o2] + list(case["argv"][0]), input=data, capture_output=True, timeout=600)
                assert r.returncode == 0
                extra["stdout_o2"] = np.frombuffer(r.stdout, np.uint8)
            dst = os.path.join(ROOT, "tests", "golden", "mk2a_%s.npz" % name)
            np.savez_compressed(dst, **extra, params=np.array(json.dumps(case["gen"])), argv=np.array([json.dumps(a) for a in case["argv"]]),
                                stdout=np.frombuffer(b"".join(outs), np.uint8), lengths=np.array([len(o) for o in outs], np.int64),
                                stderr=np.frombuffer(b"".join(errs), np.uint8), err_lengths=np.array([len(o) for o in errs], np.int64))
            print(name, [o.count(b"[OK]") for o in outs], [o.count(b"[NO]") for o in outs], [o.count(b'"type"') for o in outs],
                  ["%.2fs" % s for s in secs], flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
