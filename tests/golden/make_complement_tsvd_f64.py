"""Writes tests/golden/complement_tsvd_f64.npz: the output of the fp64 mpsk_complement_tsvd on the planted case of
tests/native_changebonds_cases.f64_golden_case, on the device.  It was run on the commit before the entry learnt MPSK_C128;
tests/test_gpu_native_changebonds.py holds the entry to these bits.  Usage: python tests/golden/make_complement_tsvd_f64.py [out]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(out):
    import native_changebonds_cases as cs
    u, s, vt = cs.f64_golden_run()
    u2, s2, vt2 = cs.f64_golden_run()
    assert np.array_equal(u, u2) and np.array_equal(s, s2) and np.array_equal(vt, vt2), "the entry is not reproducible run to run"
    np.savez(out, U=u, S=s, Vt=vt)
    print(f"wrote {out}: S[0] = {s[0]:.17g}, S[-1] = {s[-1]:.17g}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "complement_tsvd_f64.npz"))
