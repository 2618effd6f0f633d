"""Stale device state between batches.  A context keeps its unit tables, the holes form's prefix rows and descriptors, the record
slots and two sets of accumulators from one batch to the next; lfx_create zeroes a named set of them and the rest must be
written before it is read, in every batch and on every route.  Here every batch index gets new content from one
batch to the next -- a ring slot that had returns and has none, a cluttered scan after a sparse one, an empty scan, a batch
of another size -- on contexts whose workspaces start poisoned (LFX_DEBUG_POISON, the test-hooks build), and every scan of
every batch is compared with the oracle.  Each route is pinned with the LFX_DEBUG_* switches and checked with scan_routes."""
import contextlib
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from lidar_feature_extraction_amd import FeatureExtraction, make_scan, POINT_DTYPE  # noqa: E402
from lidar_feature_extraction_amd import binding as LB  # noqa: E402
from lidar_feature_extraction_amd.synth import concat  # noqa: E402
from oracle import binding as OB  # noqa: E402
from tests.parity import assert_filtered_equal  # noqa: E402

# What a scan index holds in a batch: a full grid; the grid without returns in slot max_rings - 1 ("last"), in slot 0
# ("first"), in every slot but one ("one"), anywhere ("none"); no records at all ("empty"); many features ("clutter"), few
# ("sparse").  Index k of batch t holds KINDS[(t // 2 + k) % len(KINDS)]: every state lasts two batches (both sets of
# accumulators), and each index goes from a full grid to every other state and back.
KINDS = ["full", "last", "full", "first", "full", "one", "full", "none", "full", "empty", "full", "clutter", "sparse"]
NB = 8


@contextlib.contextmanager
def switches(**kv):
    """LFX_DEBUG_<name> set around the creation of a context (the test-hooks build reads them in lfx_create)."""
    names = {"LFX_DEBUG_" + k: str(v) for k, v in kv.items()}
    old = {k: os.environ.get(k) for k in names}
    os.environ.update(names)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def scan_of(kind, R, C, seed, holes, **kw):
    """(cloud, mask of its (0, 0, 0) records).  holes: rings go without returns as (0, 0, 0) records in the grid (the zero
    filter drops them), among 3 % of scattered ones; otherwise their records are left out of the scan."""
    if kind == "empty":
        return np.zeros(0, POINT_DTYPE), np.zeros(0, bool)
    if kind == "clutter":
        c = make_scan(R, C, seed=seed, n_pillars=40, sigma=0.03, **kw)
    elif kind == "sparse":
        c = make_scan(R, C, seed=seed, n_pillars=0, sigma=0.002, spikes=False, out_of_range=False, **kw)
    else:
        c = make_scan(R, C, seed=seed, **kw)
    gone = {"last": [R - 1], "first": [0], "one": [r for r in range(R) if r != R // 2], "none": list(range(R))}.get(kind, [])
    if holes:
        zero = np.random.default_rng(seed).uniform(0.0, 1.0, len(c)) < 0.03
        zero |= np.isin(c["ring"], gone)
        for f in ("x", "y", "z"):
            c[f][zero] = 0.0
        return c, zero
    c = np.ascontiguousarray(c[~np.isin(c["ring"], gone)])
    return c, np.zeros(len(c), bool)


def check(got, c, zero, ctx):
    keep = np.nonzero(~zero)[0]
    if len(keep) == 0:
        # nothing of the scan is left: no ring, no label, no feature (whatever an earlier batch left at this index)
        assert len(got.labels) == len(c) and not got.labels.any(), ctx + ": labels of a scan without a valid return"
        assert got.ring_count.tolist() == [] and len(got.sorted_index) == 0, ctx + ": rings of a scan without a valid return"
        assert len(got.edge_index) == 0 and len(got.surface_index) == 0, ctx + ": features of a scan without a valid return"
        assert len(got.edge_points) == 0 and len(got.surface_points) == 0, ctx + ": clouds of a scan without a valid return"
        return
    sub = np.ascontiguousarray(c[keep])
    want = OB.extract(sub, canonical_ties=False)
    if want["angle_ties"] or want["curvature_ties"]:
        want = OB.extract(sub, canonical_ties=True)
        ctx += "[ties]"
    assert_filtered_equal(got, want, keep, zero, ctx)


class Stream:
    """One context, batches of scans uploaded to the device and extracted with extract_batch_device; every scan checked."""

    def __init__(self, R, max_cols, route, holes=False, poison=True, max_batch=NB, ring_cap=None, **sw):
        import torch
        self.torch = torch
        self.R, self.route, self.holes = R, route, holes
        if poison:
            sw["POISON"] = 1
        with switches(**sw):
            self.f = FeatureExtraction(device=0, max_points_per_scan=R * max_cols, max_batch=max_batch,
                                       max_points_per_ring=ring_cap or max_cols, max_rings=R, drop_zero_points=holes,
                                       stream_hint=LB.STREAM_GRID_WITH_HOLES if holes else 0, test_hooks=poison or bool(sw))
        self.st = torch.cuda.current_stream().cuda_stream
        self.t = 0

    def run(self, scans, routes, ctx):
        """scans: [(cloud, zero mask)]; routes: the route each scan must have taken (None: not looked at)."""
        torch = self.torch
        pts = concat([c for c, _ in scans])
        # (a batch of empty scans still needs a valid address)
        d = torch.from_numpy(pts.view(np.uint8)).to("cuda:0") if len(pts) else torch.zeros(64, dtype=torch.uint8, device="cuda:0")
        n = np.array([len(c) for c, _ in scans], np.uint32)
        self.f.extract_batch_device(d.data_ptr(), n, self.st)
        got_routes = self.f.scan_routes(len(scans), self.st).tolist()
        for k, (c, z) in enumerate(scans):
            if routes[k] is not None:
                assert got_routes[k] == routes[k], "%s batch %d scan %d: route %d, pinned %d (%s)" % (ctx, self.t, k, got_routes[k], routes[k], got_routes)
            check(self.f.download(k, self.st), c, z, "%s batch %d scan %d" % (ctx, self.t, k))
        self.t += 1

    def close(self):
        self.f.close()


def route_of(kind, holes, route, long_cols=False):
    """The route a scan of `kind` takes on a context pinned to `route`: a scan whose rings were left out is no grid (the
    organised routes hand it to the bucketing route in the same call); rings longer than the LDS holds are bucketed too."""
    if kind == "empty":
        return None
    if route == 0 or long_cols or (not holes and kind in ("last", "first", "one", "none")):
        return 0
    return route


def run_schedule(s, C_of, kw_of, ctx, kinds=KINDS):
    """The KINDS schedule at NB scans a batch, then a batch of 2 and one of NB again, then two batches of empty scans and two
    normal ones: new content at every index of every batch."""
    seed = [zlib.crc32(ctx.encode()) % 100000]

    def batch(kinds_b, t):
        out, routes = [], []
        for k, kind in enumerate(kinds_b):
            C = C_of(t, k)
            seed[0] += 1
            c, z = scan_of(kind, s.R, C, seed[0], s.holes, **kw_of(t, k))
            out.append((c, z))
            routes.append(route_of(kind, s.holes, s.route, C > LB.MAX_RING_POINTS) if len(c) else None)
        return out, routes

    T = 2 * len(kinds)
    plan = [[kinds[(t // 2 + k) % len(kinds)] for k in range(NB)] for t in range(T)]
    plan += [["last", "full"], ["clutter", "first"]]                               # 8 -> 2 -> 8
    plan += [[kinds[(k + 5) % len(kinds)] for k in range(NB)]]
    plan += [["empty"] * NB, ["empty"] * NB, ["full"] * NB, ["sparse"] * NB]     # an all-empty batch (no kernel runs), then scans
    for t, kinds_b in enumerate(plan):
        scans, routes = batch(kinds_b, t)
        s.run(scans, routes, ctx)


ROUTES = {
    # name: (rings, columns, route scan_routes reports for a full grid, holes, switches, make_scan keywords of index k in batch t)
    "holes16": (16, 900, 3, True, {"FUSED": 1, "HOLES": 1}, lambda t, k: {}),
    "holes64": (64, 1800, 3, True, {"FUSED": 1, "HOLES": 1}, lambda t, k: {}),
    "holes_count_by_scan": (32, 1200, 3, True, {"FUSED": 1, "HOLES": 1, "SCAN_COUNT_FROM": 1}, lambda t, k: {}),
    "organised": (16, 900, 1, False, {"FUSED": 1}, lambda t, k: {}),
    "organised_totals_kernel": (16, 900, 1, False, {"FUSED": 1, "TOTALS_KERNEL": 1}, lambda t, k: {}),
    "bucketing": (16, 900, 0, False, {"FUSED": 0}, lambda t, k: {"shuffle": True}),
    "ring_transforms": (16, 900, 2, False, {"FUSED": 1, "XFORM": 1}, lambda t, k: {"start_col": 37 + 101 * ((t + k) % 7)}),
}


@pytest.mark.parametrize("name", list(ROUTES))
def test_changing_content_on_one_context(name):
    R, C, route, holes, sw, kw_of = ROUTES[name]
    s = Stream(R, C, route, holes=holes, **sw)
    try:
        run_schedule(s, lambda t, k: C, kw_of, name)
    finally:
        s.close()


@pytest.mark.parametrize("holes", [True, False])
def test_one_ring_context_whose_ring_goes_empty(holes):
    """max_rings = 1: the only slot is the last one and the first.  (Without the zero filter a ring left out is an empty scan.)"""
    s = Stream(1, 900, 3 if holes else 1, holes=holes, FUSED=1, **({"HOLES": 1} if holes else {}))
    try:
        run_schedule(s, lambda t, k: 900, lambda t, k: {}, "one ring" + (" holes" if holes else ""),
                     kinds=["full", "last", "full", "clutter", "sparse", "empty"])
    finally:
        s.close()


def test_long_ring_context_switching_between_long_and_short_rings():
    """A context of capacity 6 000 (above LFX_MAX_RING_POINTS: ring_long_kernel and its HBM workspace): every index switches
    between rings of 5 000 points (bucketed, then the long-ring kernel) and of 1 200 (the organised route) every two batches."""
    s = Stream(4, 5000, 1, ring_cap=6000, FUSED=1)
    try:
        run_schedule(s, lambda t, k: 5000 if (t // 2 + k) % 2 == 0 else 1200, lambda t, k: {}, "long rings")
    finally:
        s.close()


def test_empty_last_ring_after_one_with_returns():
    """Regression: the holes form, a scan whose slot max_rings - 1 has returns, then at the same index one where it has none.
    The dead units of that slot write nothing; the compaction summed the slot's unit tables into the scan's totals anyway,
    and the scan published the edge and surface counts the previous batch left there.  No poison: the shipped library."""
    R, C = 16, 900
    s = Stream(R, C, 3, holes=True, poison=False, max_batch=2)
    try:
        for t, kinds in enumerate([["full", "full"], ["last", "full"], ["last", "last"], ["full", "last"]]):
            s.run([scan_of(kind, R, C, 9000 + 10 * t + k, True) for k, kind in enumerate(kinds)], [3, 3], "empty last ring")
    finally:
        s.close()
