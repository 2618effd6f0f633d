"""Randomised sweep of lfx_voxel_downsample: batches of random clouds drawn over the generators of tests/downsample_cases.py
(Gaussian, far from the origin, a given number of cells, lattices on and one ulp off the leaf's multiples, non-finite points
inserted anywhere, long lines with large keys), sizes on both sides of the small form's 12 288 points; every cloud's status,
count and centroid bytes against the oracle, and nothing written past the centroids.  On the GPU box:
    python tools/stress_downsample.py [N] [seed]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from lidar_feature_extraction_amd import FeatureExtraction
    from tests import downsample_cases as D
    from tests.test_downsample_gpu import _check_against_oracle, _run
    n_batches = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    rng = np.random.default_rng(seed)
    fx = FeatureExtraction(device=0, max_points_per_scan=1024, max_batch=1)
    t0 = time.time()
    clouds_seen = 0
    for batch in range(n_batches):
        leaf = float(np.float32(10.0 ** rng.uniform(-2.5, 0.7)))
        clouds = [D.draw(rng)[0] for _ in range(int(rng.integers(1, 12)))]
        _check_against_oracle(range(len(clouds)), clouds, leaf, *_run(fx, clouds, leaf))
        clouds_seen += len(clouds)
        if (batch + 1) % 10 == 0:
            print("%d batches ok, %.0f s" % (batch + 1, time.time() - t0), flush=True)
    fx.close()
    print("all %d batches (%d clouds) ok in %.0f s (seed %d)" % (n_batches, clouds_seen, time.time() - t0, seed))


if __name__ == "__main__":
    main()
