#!/usr/bin/env python3
"""tools/stress_long.py [--draws N] [--seed S] [--workers W] [--log PATH] -- randomised parity of LONG rings (more than
LFX_MAX_RING_POINTS points: the long-ring kernel) against the CPU oracle.  A draw is one scan of 1-8 rings of 4 609 -
70 000 points (rings of one scan differ in length), in a random input order (sorted, rotated, reversed, shuffled, ragged),
under one of a set of random hyper-parameter sets; draws of one set run in batches of up to four on one context of ring
capacity 70 016.  The oracle runs in worker processes (spawned before the GPU is touched).  Exit 1 on the first
difference."""
import argparse
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ORDERS = ["sorted", "rotated", "reversed", "shuffled", "ragged"]
CAP = 70000


def make_params(rng):
    return dict(padding=int(rng.choice([1, 2, 3, 5, 5, 5, 8, 15, 20])), n_blocks=int(rng.choice([1, 2, 6, 6, 6, 17, 40, 64])),
                neighbor_degree_threshold=float(rng.uniform(0.5, 6.0)), distance_diff_threshold=float(rng.uniform(0.05, 1.0)),
                parallel_beam_min_range_ratio=float(rng.uniform(0.005, 0.2)),
                edge_threshold=float(rng.choice([0.01, 0.05, 0.1, 0.5])), surface_threshold=float(rng.choice([0.001, 0.01, 0.1])),
                min_range=float(rng.uniform(0.05, 1.0)), max_range=float(rng.choice([50.0, 100.0, 1000.0])))


def make_draw(seed):
    """(cloud, description) of draw `seed`: deterministic."""
    from lidar_feature_extraction_amd import make_scan, synth
    rng = np.random.default_rng(seed)
    n_rings = int(rng.integers(1, 9))
    order = str(rng.choice(ORDERS))
    parts = []
    for r in range(n_rings):
        cols = int(rng.integers(4609, CAP + 1)) if rng.integers(0, 4) else int(rng.integers(4609, 9000))
        kw = {}
        if order == "rotated":
            kw["start_col"] = int(rng.integers(1, cols))
        if order == "reversed":
            kw["reverse"] = True
        if order == "ragged":
            kw["drop_fraction"] = 0.05       # (a ring may end below 4 609 points: still compared, through the LDS kernels)
        p = make_scan(1, cols, seed=seed * 16 + r, sigma=float(rng.choice([0.0, 0.01, 0.03])), **kw)
        p["ring"] = r
        parts.append(p)
    c = synth.concat(parts)
    if order == "shuffled":
        c = c[rng.permutation(len(c))]
    return np.ascontiguousarray(c), "%d rings (%s) %s" % (n_rings, ",".join(str(int((c["ring"] == r).sum())) for r in range(n_rings)), order)


def oracle_job(args):
    seed, prm = args
    from oracle import binding as OB
    c, _ = make_draw(seed)
    p = OB.Params(prm["padding"], prm["neighbor_degree_threshold"], prm["distance_diff_threshold"],
                  prm["parallel_beam_min_range_ratio"], prm["edge_threshold"], prm["surface_threshold"], prm["min_range"],
                  prm["max_range"], prm["n_blocks"])
    return OB.extract(c, params=p, canonical_ties=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--sets", type=int, default=40, help="hyper-parameter sets (one context each)")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    pool = mp.get_context("spawn").Pool(a.workers)          # before the GPU is touched
    from lidar_feature_extraction_amd import FeatureExtraction, HyperParameters
    from tests.parity import assert_scan_equal
    log = open(a.log, "w") if a.log else sys.stdout
    prng = np.random.default_rng(a.seed)
    sets = [make_params(prng) for _ in range(a.sets)]
    per_set = (a.draws + a.sets - 1) // a.sets
    t0, done, points = time.time(), 0, 0
    for k, prm in enumerate(sets):
        seeds = [a.seed * 1000003 + k * per_set + i for i in range(per_set) if done + i < a.draws]
        if not seeds:
            break
        wants = pool.map_async(oracle_job, [(s, prm) for s in seeds])
        f = FeatureExtraction(params=HyperParameters(**prm), device=0, max_points_per_scan=8 * CAP, max_batch=4,
                              max_points_per_ring=CAP, max_rings=8)
        draws = [make_draw(s) for s in seeds]
        got = []
        for b in range(0, len(draws), 4):
            got += f.extract_batch([c for c, _ in draws[b:b + 4]])
        f.close()
        for s, (c, what), g, w in zip(seeds, draws, got, wants.get()):
            ctx = "draw seed %d: %s P%d B%d" % (s, what, prm["padding"], prm["n_blocks"])
            try:
                assert_scan_equal(g, w, ctx)
            except AssertionError as e:
                print("FAIL %s\n  %s" % (ctx, e), file=log, flush=True)
                pool.terminate()
                return 1
            points += len(c)
        done += len(seeds)
        print("set %2d (P%d B%d): %d draws equal to the oracle (%d in all, %.1f M points, %.0f s)" % (
            k, prm["padding"], prm["n_blocks"], len(seeds), done, points / 1e6, time.time() - t0), file=log, flush=True)
    print("ALL EQUAL: %d draws, %.1f M points, %.0f s" % (done, points / 1e6, time.time() - t0), file=log, flush=True)
    pool.close()
    pool.join()
    return 0


if __name__ == "__main__":
    sys.exit(main())
