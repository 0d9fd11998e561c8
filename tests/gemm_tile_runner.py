"""Child-process runner of the GEMM tile matrix (not a test file): `python gemm_tile_runner.py tiles|streamk`.

MPSK_SPLITK, MPSK_XCDGRID, MPSK_SPLITK_F and MPSK_STREAMK are read once when libmpsk.so is loaded, so each setting needs
a process of its own: tests/test_gpu_gemm_tiles.py starts this module with the environment extended by one knob.  It runs
the case list of tests/exact_inputs.py through mpsk_gemm and prints ONE JSON line
    {"set": ..., "cases": n, "mismatches": [...], "wall_s": ...}
exit status 0 when every case passed, 1 on mismatches."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(which):
    t0 = time.time()
    import exact_inputs as ei
    import mpskit_jl_amd as mk
    cases = {"tiles": ei.gemm_cases, "streamk": ei.streamk_cases}[which]()
    be = mk.Backend(0)
    try:
        bad = ei.run_gemm_cases(be, cases)
    finally:
        be.close()
    print(json.dumps({"set": which, "cases": len(cases), "mismatches": bad[:20], "n_mismatches": len(bad),
                      "wall_s": round(time.time() - t0, 2)}), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else "tiles"))
