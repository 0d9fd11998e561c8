"""Writes tests/golden/window_quench.json: the local quench of tests/window_helpers.quench on the host stand-in backend
(tests/cpu_backend.CpuComplexBackend).  Run from the repository root:  python tests/golden/make_window_quench.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from cpu_backend import CpuBackend, CpuComplexBackend  # noqa: E402
from window_helpers import quench  # noqa: E402

if __name__ == "__main__":
    overlaps, tots = quench(CpuComplexBackend(), gs_be=CpuBackend())
    out = {"model": "Heisenberg S=1/2, VUMPS D=16, window L=8, S+ at site 4, TDVP dt=0.05, 5 steps",
           "abs_overlap": overlaps, "tot": tots}
    with open(os.path.join(HERE, "window_quench.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))
