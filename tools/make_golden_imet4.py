"""Writes tests/golden/imet4_*.npz: stdout of the reference's imet/imet4iq.c on the captures of tests/imet4_cases.py.

The reference is compiled with its Makefile's flags (-O3 -w -Ofast, -lm) and -DVER_JSN_STR="oracle" into a temporary directory that is
removed afterwards; only the data (case name, generator parameters, argv, stdout) is kept.

    python tools/make_golden_imet4.py path/to/reference/checkout
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
from tests import imet4_cases as cases  # noqa: E402


def main(ref_root: str) -> None:
    src = os.path.join(ref_root, "imet", "imet4iq.c")
    tmp = tempfile.mkdtemp(prefix="imet4ref_")
    try:
        exe = os.path.join(tmp, "imet4iq")
        subprocess.check_call(["gcc", "-O3", "-w", "-Ofast", '-DVER_JSN_STR="oracle"', "-o", exe, src, "-lm"])
        for name, case in cases.CASES.items():
            data, wav = cases.capture(case)
            outs = []
            for argv in case["argv"]:
                args = list(argv)
                if wav is not None:
                    p = os.path.join(tmp, "in.wav")
                    with open(p, "wb") as f:
                        f.write(wav)
                    args = [p if a == "{wav}" else a for a in args]
                r = subprocess.run([exe] + args, input=data, capture_output=True, timeout=600)
                assert r.returncode == 0, (name, argv, r.stderr[-300:])
                outs.append(r.stdout)
            dst = os.path.join(ROOT, "tests", "golden", "imet4_%s.npz" % name)
            np.savez_compressed(dst, params=np.array(json.dumps(case["gen"])), argv=np.array([json.dumps(a) for a in case["argv"]]),
                                stdout=np.frombuffer(b"".join(outs), np.uint8),
                                lengths=np.array([len(o) for o in outs], np.int64))
            print(name, [o.count(b"\n") for o in outs])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
