"""Writes tests/golden/imet4f32_*.npz: stdout of the compiled reference imet4iq (oracle/_ref/imet4iq, built by `make -C oracle ref`) on the
float32 captures of tests/imet4_f32_cases.py.  Only the data (generator parameters, argv, stdout) is kept, in the layout of imet4_*.npz.

    python tools/make_golden_imet4_f32.py [path/to/imet4iq]
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
from tests import imet4_f32_cases as cases  # noqa: E402


def main(exe: str) -> None:
    tmp = tempfile.mkdtemp(prefix="imet4f32_")
    try:
        for name, case in cases.CASES.items():
            _, data, wav = cases.capture(case)
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
            dst = os.path.join(ROOT, "tests", "golden", "imet4f32_%s.npz" % name)
            np.savez_compressed(dst, params=np.array(json.dumps(case["gen"])), argv=np.array([json.dumps(a) for a in case["argv"]]),
                                stdout=np.frombuffer(b"".join(outs), np.uint8),
                                lengths=np.array([len(o) for o in outs], np.int64))
            print(name, [o.count(b"\n\n") for o in outs])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) > 2:
        sys.exit(__doc__)
    main(sys.argv[1] if len(sys.argv) == 2 else os.path.join(ROOT, "oracle", "_ref", "imet4iq"))
