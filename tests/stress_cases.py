"""Randomised parity cases shared by tests/test_gpu_parity.py (a seeded slice under pytest -m gpu) and
tools/stress.py (the long sweep): random sensor shapes, input orders, sensor noise and all nine
hyper-parameters; every output of the HIP path against the CPU oracle (tests/parity.assert_scan_equal)."""
import time

import numpy as np

from lidar_feature_extraction_amd import FeatureExtraction, HyperParameters, make_scan
from oracle import binding as OB
from lidar_feature_extraction_amd import binding as LB
from tests.parity import assert_scan_equal, assert_filtered_equal

# ("zeros": a grid whose invalid returns are (0, 0, 0) records, zero filter on -- the holes form of the organised route)
ORDERS = ["sorted", "rotated", "reversed", "revrot", "shuffled", "ragged", "ragrot", "zeros", "zeros"]


def draw(rng):
    """One case: (rings, cols, HyperParameters, order, make_scan kwargs, seed, sigma, exact_cap)."""
    rings = int(rng.choice([4, 8, 16, 32, 64]))
    cols = int(rng.integers(150, 2600))
    if rng.integers(0, 6) == 0:                # long rings: the 12-chunk form of the unit kernels, or (few blocks) the workgroup-per-ring kernel
        cols = int(rng.integers(2600, 4609))        # (up to LFX_MAX_RING_POINTS)
        rings = min(rings, 16)
    P = int(rng.choice([1, 2, 3, 5, 5, 5, 8, 15, 20, 33]))      # (16 and up: beyond the windows, the workgroup-per-ring kernel for every ring)
    B = int(rng.choice([1, 2, 3, 6, 6, 6, 9, 17, 40]))
    hp = HyperParameters(padding=P, n_blocks=B,
                         neighbor_degree_threshold=float(rng.uniform(0.5, 6.0)),
                         distance_diff_threshold=float(rng.uniform(0.05, 1.0)),
                         parallel_beam_min_range_ratio=float(rng.uniform(0.005, 0.2)),
                         edge_threshold=float(rng.choice([0.01, 0.05, 0.1, 0.5])),
                         surface_threshold=float(rng.choice([0.001, 0.01, 0.1])),
                         min_range=float(rng.uniform(0.05, 1.0)), max_range=float(rng.choice([50.0, 100.0, 1000.0])))
    kw = {}
    order = str(rng.choice(ORDERS))
    if order in ("rotated", "revrot", "ragrot"):
        kw["start_col"] = int(rng.integers(1, cols))
    if order in ("reversed", "revrot"):
        kw["reverse"] = True
    if order == "shuffled":
        kw["shuffle"] = True
    if order in ("ragged", "ragrot"):
        kw["drop_fraction"] = float(rng.uniform(0.01, 0.4))
    if order == "zeros":
        # (share of the returns zeroed, a stretch of columns without a return, whether the context is told)
        kw["_zeros"] = (float(rng.choice([0.0, 0.01, 0.05, 0.05, 0.15, 0.3])), int(rng.integers(0, 3)) == 0, int(rng.integers(0, 2)) == 0)
    seed = int(rng.integers(1, 1 << 30))
    sigma = float(rng.choice([0.01, 0.002, 0.03]))
    exact_cap = bool(rng.integers(0, 2))
    return rings, cols, hp, order, kw, seed, sigma, exact_cap


def run_case(case, rng):
    import os
    rings, cols, hp, order, kw, seed, sigma, exact_cap = draw(rng)
    zeros = kw.pop("_zeros", None)
    clouds = [make_scan(rings, cols, seed=seed + i, sigma=sigma, **kw) for i in range(2)]
    if zeros is not None:
        return run_zeros_case(case, rng, rings, cols, hp, clouds, zeros, seed, exact_cap)
    # a third of the contexts that know the sensor look for rotated / reversed rings from the first batch on
    pin = bool(rng.integers(0, 3) == 0)
    if pin:
        os.environ["LFX_DEBUG_XFORM"] = "1"
    try:
        f = FeatureExtraction(hp, device=0, max_points_per_scan=rings * cols, max_batch=2,
                              max_points_per_ring=cols if exact_cap else 0, max_rings=rings if exact_cap else 0)
    finally:
        os.environ.pop("LFX_DEBUG_XFORM", None)
    op = OB.Params(hp.padding, hp.neighbor_degree_threshold, hp.distance_diff_threshold, hp.parallel_beam_min_range_ratio,
                   hp.edge_threshold, hp.surface_threshold, hp.min_range, hp.max_range, hp.n_blocks)
    want = []
    for c in clouds:
        w = OB.extract(c, op, canonical_ties=False)
        if w["angle_ties"] or w["curvature_ties"]:
            w = OB.extract(c, op, canonical_ties=True)
        want.append(w)
    try:
        for rep in range(2):                       # the second call may take another route (order pre-pass, path choice)
            # (the two clouds trade places between calls: no index sees the content it had in the batch before)
            which = [rep % 2, 1 - rep % 2]
            got = f.extract_batch([clouds[i] for i in which])
            for k, i in enumerate(which):
                assert_scan_equal(got[k], want[i], "case %d: %dx%d P%d B%d %s rep%d scan%d seed%d" % (
                    case, rings, cols, hp.padding, hp.n_blocks, order, rep, i, seed))
    finally:
        f.close()
    return order


def run_zeros_case(case, rng, rings, cols, hp, clouds, zeros, seed, exact_cap):
    """A grid with (0, 0, 0) records against the oracle on the filtered cloud (assert_filtered_equal)."""
    fraction, gap, hinted = zeros
    masks = []
    for i, c in enumerate(clouds):
        z = rng.uniform(0.0, 1.0, len(c)) < fraction
        if gap:
            lo = int(rng.integers(0, cols))
            width = int(rng.integers(1, max(2, cols // 3)))
            z |= (np.arange(len(c)) // rings >= lo) & (np.arange(len(c)) // rings < lo + width) & (rng.uniform(0.0, 1.0, len(c)) < 0.9)
        masks.append(z)
    # a third of the draws: one of the two clouds loses every return of a ring (the first, the last or any): a slot with
    # returns at one index in one batch and without them in the next
    gone = ""
    if rng.integers(0, 3) == 0:
        i = int(rng.integers(0, 2))
        pick = int(rng.integers(0, 3))
        r = 0 if pick == 0 else (rings - 1 if pick == 1 else int(rng.integers(0, rings)))
        masks[i] = masks[i] | (clouds[i]["ring"] == r)
        gone = " ring%d gone in scan%d" % (r, i)
    for c, z in zip(clouds, masks):
        for f in ("x", "y", "z"):
            c[f][z] = 0.0
    import os
    by_scan = bool(rng.integers(0, 2))             # the count pass of large batches (one workgroup per scan), pinned on for these two scans
    if by_scan:
        os.environ["LFX_DEBUG_SCAN_COUNT_FROM"] = "1"
    try:
        f = FeatureExtraction(hp, device=0, max_points_per_scan=rings * cols, max_batch=2, max_points_per_ring=cols if exact_cap else 0,
                              max_rings=rings, drop_zero_points=True, stream_hint=LB.STREAM_GRID_WITH_HOLES if hinted else 0)
    finally:
        os.environ.pop("LFX_DEBUG_SCAN_COUNT_FROM", None)
    op = OB.Params(hp.padding, hp.neighbor_degree_threshold, hp.distance_diff_threshold, hp.parallel_beam_min_range_ratio,
                   hp.edge_threshold, hp.surface_threshold, hp.min_range, hp.max_range, hp.n_blocks)
    keeps = [np.nonzero(~z)[0] for z in masks]
    want = []
    for c, keep in zip(clouds, keeps):
        w = OB.extract(np.ascontiguousarray(c[keep]), op, canonical_ties=False)
        if w["angle_ties"] or w["curvature_ties"]:
            w = OB.extract(np.ascontiguousarray(c[keep]), op, canonical_ties=True)
        want.append(w)
    try:
        for rep in range(3):                       # (the route follows the report: plain form, holes form, the bucketing route)
            which = [rep % 2, 1 - rep % 2]         # (the clouds trade places between calls, as in run_case)
            got = f.extract_batch([clouds[i] for i in which])
            for k, i in enumerate(which):
                assert_filtered_equal(got[k], want[i], keeps[i], masks[i], "case %d: %dx%d P%d B%d zeros %.2f%s%s%s rep%d scan%d seed%d[ties]" % (
                    case, rings, cols, hp.padding, hp.n_blocks, fraction, " gap" if gap else "", " hinted" if hinted else "", gone, rep, i, seed))
    finally:
        f.close()
    return "zeros"


def run_cases(n_cases, seed=7, report_every=0):
    rng = np.random.default_rng(seed)
    t0 = time.time()
    seen = {}
    for case in range(n_cases):
        o = run_case(case, rng)
        seen[o] = seen.get(o, 0) + 1
        if report_every and case % report_every == report_every - 1:
            print("%d cases ok, %.0f s" % (case + 1, time.time() - t0), flush=True)
    return seen


# ---------------------------------------------------------------------------------------------- batches
# The cases above run two scans at a time.  A BATCH case runs 3 .. 64 scans of a few distinct contents in a drawn arrangement,
# three calls with the arrangement redrawn, and compares every position of every call (tests/test_launch_scale_gpu.py
# test_stress_slice_batches runs a seeded slice, tools/stress.py --batches the long sweep).  draw / run_case / run_zeros_case /
# ORDERS above stay as they are: test_stress_slice depends on their seeded sequence.

def _order_kwargs(rng, order, cols):
    """make_scan keywords of one input order (as draw() chooses them); "zeros" -> {"_zeros": (fraction, gap)}."""
    kw = {}
    if order in ("rotated", "revrot", "ragrot"):
        kw["start_col"] = int(rng.integers(1, cols))
    if order in ("reversed", "revrot"):
        kw["reverse"] = True
    if order == "shuffled":
        kw["shuffle"] = True
    if order in ("ragged", "ragrot"):
        kw["drop_fraction"] = float(rng.uniform(0.01, 0.4))
    if order == "zeros":
        kw["_zeros"] = (float(rng.choice([0.0, 0.01, 0.05, 0.05, 0.15, 0.3])), int(rng.integers(0, 3)) == 0)
    return kw


def draw_batch(rng):
    """One batch case: sensor shape, batch size, number of distinct contents, the stream's order, the odd scans mixed in, all
    nine hyper-parameters (as draw() draws them), seed, noise."""
    rings = int(rng.choice([16, 32, 64, 128]))
    cols = int(rng.integers(150, 2601))
    batch = int(rng.integers(3, 65))
    n_distinct = int(rng.integers(2, 8))
    P = int(rng.choice([1, 2, 3, 5, 5, 5, 8, 15, 20, 33]))
    B = int(rng.choice([1, 2, 3, 6, 6, 6, 9, 17, 40]))
    hp = HyperParameters(padding=P, n_blocks=B,
                         neighbor_degree_threshold=float(rng.uniform(0.5, 6.0)),
                         distance_diff_threshold=float(rng.uniform(0.05, 1.0)),
                         parallel_beam_min_range_ratio=float(rng.uniform(0.005, 0.2)),
                         edge_threshold=float(rng.choice([0.01, 0.05, 0.1, 0.5])),
                         surface_threshold=float(rng.choice([0.001, 0.01, 0.1])),
                         min_range=float(rng.uniform(0.05, 1.0)), max_range=float(rng.choice([50.0, 100.0, 1000.0])))
    order = str(rng.choice(ORDERS))
    kw = _order_kwargs(rng, order, cols)
    others = []                                   # a third of the draws: one or two scans of another order mixed in
    if rng.integers(0, 3) == 0:
        for _ in range(int(rng.integers(1, 3))):
            o = str(rng.choice([x for x in ORDERS if x != order]))
            others.append((o, _order_kwargs(rng, o, cols)))
    return dict(rings=rings, cols=cols, batch=batch, n_distinct=n_distinct, hp=hp, order=order, kw=kw, others=others,
                seed=int(rng.integers(1, 1 << 30)), sigma=float(rng.choice([0.01, 0.002, 0.03])), exact_cap=bool(rng.integers(0, 2)),
                hinted=bool(rng.integers(0, 2)))


def _batch_scan(rng, d, kw, seed):
    """(cloud, keep): one scan of the case; keep = the indices a zero filter leaves."""
    kw = dict(kw)
    zeros = kw.pop("_zeros", None)
    c = make_scan(d["rings"], d["cols"], seed=seed, sigma=d["sigma"], **kw)
    if zeros is None:
        return c, np.arange(len(c))
    fraction, gap = zeros
    z = rng.uniform(0.0, 1.0, len(c)) < fraction
    if gap:
        lo = int(rng.integers(0, d["cols"]))
        width = int(rng.integers(1, max(2, d["cols"] // 3)))
        col = np.arange(len(c)) // d["rings"]
        z |= (col >= lo) & (col < lo + width) & (rng.uniform(0.0, 1.0, len(c)) < 0.9)
    for f in ("x", "y", "z"):
        c[f][z] = 0.0
    return c, np.nonzero(~z)[0]


def run_batch_case(case, rng):
    d = draw_batch(rng)
    hp = d["hp"]
    scans = [_batch_scan(rng, d, d["kw"], d["seed"] + i) for i in range(d["n_distinct"])]
    odd = [_batch_scan(rng, d, kw, d["seed"] + 100 + i) for i, (_, kw) in enumerate(d["others"])]
    drop_zero = d["order"] == "zeros" or any(o == "zeros" for o, _ in d["others"])
    op = OB.Params(hp.padding, hp.neighbor_degree_threshold, hp.distance_diff_threshold, hp.parallel_beam_min_range_ratio,
                   hp.edge_threshold, hp.surface_threshold, hp.min_range, hp.max_range, hp.n_blocks)
    want = []
    for c, keep in scans + odd:
        kept = c if not drop_zero else np.ascontiguousarray(c[keep])
        w = OB.extract(kept, op, canonical_ties=False)
        if w["angle_ties"] or w["curvature_ties"]:
            w = OB.extract(kept, op, canonical_ties=True)
        want.append(w)
    f = FeatureExtraction(hp, device=0, max_points_per_scan=d["rings"] * d["cols"], max_batch=d["batch"],
                          max_points_per_ring=d["cols"] if d["exact_cap"] else 0, max_rings=d["rings"], drop_zero_points=drop_zero,
                          stream_hint=LB.STREAM_GRID_WITH_HOLES if (d["order"] == "zeros" and d["hinted"]) else 0)
    what = "batch case %d: %dx%dx%d P%d B%d %s%s, %d distinct, seed%d" % (
        case, d["rings"], d["cols"], d["batch"], hp.padding, hp.n_blocks, d["order"],
        "".join(" +" + o for o, _ in d["others"]), d["n_distinct"], d["seed"])
    try:
        for rep in range(3):
            pick = rng.integers(0, len(scans), d["batch"])                  # (redrawn: no position keeps its content)
            for k, pos in enumerate(rng.choice(d["batch"], len(odd), replace=False)):
                pick[pos] = len(scans) + k
            clouds = [(scans + odd)[u][0] for u in pick]
            got = f.extract_batch(clouds)
            assert len(got) == d["batch"]
            for s, u in enumerate(pick):
                c, keep = (scans + odd)[u]
                ctx = "%s rep%d position%d content%d[ties]" % (what, rep, s, u)
                if drop_zero:
                    zero = np.ones(len(c), bool)
                    zero[keep] = False
                    assert_filtered_equal(got[s], want[u], keep, zero, ctx)
                else:
                    assert_scan_equal(got[s], want[u], ctx)
    finally:
        f.close()
    return d["order"]


def run_batch_cases(n_cases, seed=11, report_every=0):
    rng = np.random.default_rng(seed)
    t0 = time.time()
    seen = {}
    for case in range(n_cases):
        o = run_batch_case(case, rng)
        seen[o] = seen.get(o, 0) + 1
        if report_every and case % report_every == report_every - 1:
            print("%d batch cases ok, %.0f s" % (case + 1, time.time() - t0), flush=True)
    return seen
