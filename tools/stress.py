"""Randomised parity sweep (the long form; a 200-draw seeded slice runs under pytest -m gpu as
test_stress_slice).  For N random (sensor shape, input order, hyper-parameter) draws: HIP path vs the CPU oracle,
everything assert_scan_equal checks.  Run on the GPU box:
    python tools/stress.py [N] [seed]
    python tools/stress.py --batches [N] [seed]     batches of 3 .. 64 scans, three calls each, every position compared
                                                    (tests/stress_cases.py draw_batch; the slice: test_stress_slice_batches)"""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from anywhere: the repo root holds the packages
from tests.stress_cases import run_batch_cases, run_cases  # noqa: E402

args = [a for a in sys.argv[1:] if a != "--batches"]
batches = "--batches" in sys.argv[1:]
n_cases = int(args[0]) if len(args) > 0 else 200
seed = int(args[1]) if len(args) > 1 else 7
t0 = time.time()
seen = (run_batch_cases if batches else run_cases)(n_cases, seed, report_every=20)
print("all %d %scases ok in %.0f s (seed %d; input orders drawn: %s)" % (n_cases, "batch " if batches else "", time.time() - t0, seed, seen))
