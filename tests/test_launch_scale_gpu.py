"""Batches of launch scale against the CPU oracle, EVERY position of every call (tests/launch_scale.py has the comparison).

Each case is one context and several consecutive calls.  A call's batch is an arrangement of a few distinct scans drawn from a
seeded generator (position -> distinct[pick[position]], redrawn per call, so a position's content changes from call to call
and is not position mod U), sizes [B, B - 24, B]: a last generation that is not full, then a larger batch over a smaller
one's leftovers; consecutive calls alternate between the two sets of accumulators (lfx_api.hip, c->parity / par_dirty) and
every call after the first is routed by the report of the large batch before it (choose_route).  After every call the routes
of all scans are asserted, then the device view's arrays are compared for all positions; once per case the packed payloads
(pack_features, pack_xyz12) and download() at 18 positions spread over the batch go the same way.

`python -m tests.test_launch_scale_gpu` prepares every case without a device (scans, oracle, expectations, tie checks)."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lidar_feature_extraction_amd import FeatureExtraction, HyperParameters, make_scan, synth  # noqa: E402
from lidar_feature_extraction_amd import binding as LB  # noqa: E402
from oracle import binding as OB  # noqa: E402
from tests import launch_scale as LS  # noqa: E402
from tests.parity import assert_scan_equal, assert_filtered_equal  # noqa: E402

pytestmark = pytest.mark.gpu


@dataclasses.dataclass
class Distinct:
    cloud: np.ndarray                  # the records the device is given
    kind: str                          # what decides its route
    keep: np.ndarray = None            # a grid with (0, 0, 0) records: the indices the zero filter keeps
    want: dict = None                  # the oracle on the (filtered) cloud

    @property
    def zero(self):
        z = np.ones(len(self.cloud), bool)
        z[self.keep] = False
        return z


@dataclasses.dataclass
class Case:
    name: str
    rings: int
    cols: int
    sizes: list                        # batch size of each call
    distinct: object                   # () -> [Distinct]
    route: object                      # (call, kind) -> expected lfx_scan_routes value
    hp: HyperParameters = dataclasses.field(default_factory=HyperParameters)
    outputs: int = 0
    drop_zero: bool = False
    hint: int = 0
    arrange: object = None             # (rng, call, batch, kinds) -> pick; None: any distinct scan anywhere
    launches: tuple = ()               # kernels whose launch count must be non-zero at the end (kernel_times)
    seed: int = 1

    @property
    def curvature(self):
        return self.outputs == 0 or bool(self.outputs & LB.OUT_CURVATURE)


def oracle_params(hp):
    return OB.Params(hp.padding, hp.neighbor_degree_threshold, hp.distance_diff_threshold, hp.parallel_beam_min_range_ratio,
                     hp.edge_threshold, hp.surface_threshold, hp.min_range, hp.max_range, hp.n_blocks)


def grids(rings, cols, seeds, kind="grid", **kw):
    return lambda: [Distinct(make_scan(rings, cols, seed=s, **kw), kind) for s in seeds]


def zeroed(cloud, fraction, seed, columns=None, rings=None):
    """`cloud` with a share of its returns written as (0, 0, 0) records (and whole columns / rings of them) -> (cloud, keep)."""
    c = cloud.copy()
    zero = np.random.default_rng(seed).uniform(0, 1, len(c)) < fraction
    n_rings = int(c["ring"].max()) + 1
    if columns is not None:
        zero |= np.isin(np.arange(len(c)) // n_rings, columns)
    if rings is not None:
        zero |= np.isin(c["ring"], rings)
    for f in ("x", "y", "z"):
        c[f][zero] = 0.0
    return c, np.nonzero(~zero)[0]


def holes_scans(rings, cols, seeds, clean_seeds=()):
    """Grids with 5 % of the records zeroed.  The first four: the LAST ring all zero, ring 0 all zero, no zero record at all,
    200 columns without a return.  clean_seeds: further scans without a zero record."""
    def make():
        out = []
        for i, s in enumerate(seeds):
            base = make_scan(rings, cols, seed=s)
            if i == 0:
                c, keep = zeroed(base, 0.05, s, rings=[rings - 1])
                out.append(Distinct(c, "holes", keep))
            elif i == 1:
                c, keep = zeroed(base, 0.05, s, rings=[0])
                out.append(Distinct(c, "holes", keep))
            elif i == 2:
                out.append(Distinct(base, "clean", np.arange(len(base))))
            elif i == 3:
                c, keep = zeroed(base, 0.05, s, columns=np.arange(cols // 3, cols // 3 + 200))
                out.append(Distinct(c, "gap", keep))
            else:
                c, keep = zeroed(base, 0.05, s)
                out.append(Distinct(c, "holes", keep))
        for s in clean_seeds:
            base = make_scan(rings, cols, seed=s)
            out.append(Distinct(base, "clean", np.arange(len(base))))
        return out
    return make


def turned_scans(rings, cols, seeds):
    def make():
        rng = np.random.default_rng(77)
        return [Distinct(make_scan(rings, cols, seed=s, start_col=int(rng.integers(1, cols)), reverse=bool(i % 2)), "turned")
                for i, s in enumerate(seeds)]
    return make


ODD_KINDS = ("shuffled", "ragged", "empty", "ring of 4", "rotated")


def odd_scans(rings, cols, seeds, odd_seed):
    """Organised scans, and after them one of each odd kind (ODD_KINDS)."""
    def make():
        out = grids(rings, cols, seeds)()
        out.append(Distinct(make_scan(rings, cols, seed=odd_seed, shuffle=True), "shuffled"))
        out.append(Distinct(make_scan(rings, cols, seed=odd_seed + 1, drop_fraction=0.05), "ragged"))
        out.append(Distinct(make_scan(rings, cols, seed=odd_seed + 2)[:0], "empty"))
        c = make_scan(rings, cols, seed=odd_seed + 3)
        few = c["ring"] == 7
        out.append(Distinct(synth.concat([c[~few], c[few][:4]]), "ring of 4"))
        out.append(Distinct(make_scan(rings, cols, seed=odd_seed + 4, start_col=cols // 3), "rotated"))
        return out
    return make


def odd_arrangement(rng, call, batch, kinds):
    """Organised scans everywhere -- from the second call on with an odd scan at positions 0, 1, 511, B-2, B-1 and ten seeded
    others, the five kinds in turn."""
    plain = np.nonzero(np.asarray(kinds) == "grid")[0]
    pick = plain[rng.integers(0, len(plain), batch)]
    if call >= 1:
        fixed = [0, 1, 511, batch - 2, batch - 1]
        free = np.setdiff1d(np.arange(2, batch - 2), fixed)
        others = rng.choice(free, 10, replace=False)
        for i, pos in enumerate(fixed + sorted(int(p) for p in others)):
            pick[pos] = list(kinds).index(ODD_KINDS[i % len(ODD_KINDS)])
    return pick


def clean_tail(n_calls_mixed):
    """Call 0: scans with zero records only (every one of them falls back); then the whole mixture; then calls of zero-free
    scans only."""
    def arrange(rng, call, batch, kinds):
        if call == 0:
            holed = np.nonzero(np.asarray(kinds) != "clean")[0]
            return holed[rng.integers(0, len(holed), batch)]
        if call < n_calls_mixed:
            return rng.integers(0, len(kinds), batch)
        clean = np.nonzero(np.asarray(kinds) == "clean")[0]
        return clean[rng.integers(0, len(clean), batch)]
    return arrange


STRESS_BATCH_DRAWS = 24             # (test_stress_slice_batches; how it was sized: its docstring)
NO_CURVATURE = LB.OUT_FEATURES | LB.OUT_LABELS | LB.OUT_SORTED_INDEX
B1K, B512 = [1024, 1000, 1024], [512, 488, 512]


def _holes_route(call, kind):
    # the holes form reads a grid in place (3) unless a block's positions span more columns than a workgroup loads
    # (grid_count_kernel / scan_count_kernel: piece_hi - piece_lo + 1 > max_pieces = 4 (chunks + 2) pieces of 16 columns; a
    # block of a 64 x 1 800 scan with 5 % holes is ~250 positions in ~265 columns, 4 chunks: 384 columns at most, and the
    # 200 empty columns make it ~465): that scan is the bucketing route's (0)
    return 0 if kind == "gap" else 3


def _found_holes_route(call, kind):
    # call 0 runs the plain organised form, which refuses a scan for its first zero record; the report (zero_fell) moves the
    # stream to the holes form; the first call of zero-free scans only (call 3) still runs it and reports no zero group
    # (choose_route: holes_ran && 50 zero_groups < of), so the next one is back on the plain form
    if call == 0:
        return 1 if kind == "clean" else 0
    return 1 if call == 4 else _holes_route(call, kind)


CASES = [
    # the launch the metric is quoted on; route 1 everywhere.  From the second call on the stream has not been falling back
    # (choose_route: short_tail = was_fused && of && fell == 0), so the tail is fallback_tail_kernel's one launch
    Case("headline", 64, 1800, B1K, grids(64, 1800, range(9000, 9048)), lambda call, kind: 1,
         launches=("ring_unit_org_kernel", "feature_compact_kernel", "fallback_tail_kernel")),
    # unit variant 1 at scale
    Case("launch-file parameters", 64, 1800, B512, grids(64, 1800, range(9100, 9113)), lambda call, kind: 1, hp=HyperParameters.launch_yaml()),
    # the other template of the unit kernel: curvature_sorted is NULL, the features still carry theirs
    Case("no curvature", 64, 1800, B512, grids(64, 1800, range(9200, 9213)), lambda call, kind: 1, outputs=NO_CURVATURE),
    # 16 384 ring slots, compaction with a hundred records per scan
    Case("many short scans 16x900", 16, 900, B1K, grids(16, 900, range(9300, 9313)), lambda call, kind: 1),
    Case("many short scans 16x1800", 16, 1800, B1K, grids(16, 1800, range(9400, 9413)), lambda call, kind: 1),
    # all 32 positions against the oracle, content moving between calls
    Case("OS1-128", 128, 2048, [32, 8, 32, 32, 32], grids(128, 2048, range(9500, 9511), vfov_deg=22.5), lambda call, kind: 1),
    # the long form of the unit kernel at scale
    Case("wide rings", 64, 3600, [256, 232, 256], grids(64, 3600, range(9600, 9607)), lambda call, kind: 1),
    # scan_count_kernel: lfx_api.hip run_batch takes it for `batch >= c->scan_count_from` (256, lfx_internal.hpp) where its
    # LDS fits (64 rings x 117 words + 192 words = 30 KB <= 144 KB); all three batch sizes are above 256
    Case("holes, hinted", 64, 1800, B1K, holes_scans(64, 1800, range(9700, 9712)), _holes_route, drop_zero=True,
         hint=LB.STREAM_GRID_WITH_HOLES, launches=("grid_count_kernel",)),
    # call 0 holds scans with zero records only: all 1 024 fall back behind a launch sized for 8 list entries (choose_route:
    # fb_grid = guess = 8 without a report; ring_scatter_kernel and the unit kernel loop over the list)
    Case("holes, found", 64, 1800, B1K + [1024, 1024], holes_scans(64, 1800, range(9700, 9712), range(9720, 9725)), _found_holes_route,
         drop_zero=True, arrange=clean_tail(3), launches=("grid_count_kernel", "ring_scatter_kernel")),
    # call 0 falls back whole (angle order); the report (order_fell) switches ring_cut_kernel on: route 2 from then on
    Case("turned rings, found", 64, 1800, B512, turned_scans(64, 1800, range(9800, 9813)), lambda call, kind: 0 if call == 0 else 2,
         launches=("ring_cut_kernel",)),
    # the bucketing route for every scan.  Call 0 is fused with fb_grid = 8 and a list of 512; its report (4 fell > of) sets
    # bucket_all, so later calls are not fused and 512 x 64 = 32 768 rings > 8 192 take ring_totals_kernel (run_batch:
    # self_totals = fused || batch * max_rings <= 8192)
    Case("records missing", 64, 1800, B512, grids(64, 1800, range(9900, 9913), kind="ragged", drop_fraction=0.05), lambda call, kind: 0,
         launches=("ring_scatter_kernel", "ring_totals_kernel")),
    # a short fall-back list inside a large organised batch.  Call 0 has no odd scan, so call 1 is on the short tail
    # (choose_route: short_tail needs fell == 0 in the report) and its 15 odd scans are redone by fallback_tail_kernel, whose
    # grid has (1024 + kTailMaxTurns - 1) / kTailMaxTurns = 8 rows; calls 2 and 3 follow a report with fell = 15 and take the
    # five-launch route behind a list sized 2 fell + 8 = 38
    Case("odd scans out", 64, 1800, [1024, 1024, 1000, 1024], odd_scans(64, 1800, range(10000, 10013), 10050),
         lambda call, kind: 1 if kind == "grid" else 0, arrange=odd_arrangement, launches=("fallback_tail_kernel", "ring_extract_kernel")),
]

_prepared = {}


def prepare(case):
    """Everything a case needs before its first device call: the distinct scans, the oracle on each (tie-free, asserted), the
    expectations in the view's layout."""
    if case.name not in _prepared:
        distinct = case.distinct()
        cap = (case.cols + 63) // 64 * 64
        per_scan = []
        for u, d in enumerate(distinct):
            kept = d.cloud if d.keep is None else np.ascontiguousarray(d.cloud[d.keep])
            d.want = OB.extract(kept, oracle_params(case.hp), canonical_ties=False)
            LS.require_tie_free(d.want, "%s: distinct scan %d (%s)" % (case.name, u, d.kind))
            per_scan.append(LS.expected_ring_major(d.want, case.rings, cap, d.keep))
        U = len(distinct)
        assert all(b % U for b in case.sizes), "%s: %d distinct scans divide a batch size" % (case.name, U)
        _prepared[case.name] = (distinct, LS.Expected(per_scan, [len(d.cloud) for d in distinct]))
    return _prepared[case.name]


def check_download(case, got, d, ctx):
    """download(i) against the oracle with the suite's own checkers; a context without the per-point curvature brings none back
    and is compared on everything else."""
    if not case.curvature:
        assert len(got.curvature) == 0, ctx + ": curvature without LFX_OUT_CURVATURE"
        full = np.zeros(len(d.cloud), np.float64)
        full[np.arange(len(d.cloud)) if d.keep is None else d.keep] = d.want["curvature"]
        got = dataclasses.replace(got, curvature=full)
    if d.keep is None:
        assert_scan_equal(got, d.want, ctx)
    else:
        assert_filtered_equal(got, d.want, d.keep, d.zero, ctx)


@pytest.mark.parametrize("case", CASES, ids=[c.name.replace(" ", "_").replace(",", "") for c in CASES])
def test_launch_scale(case):
    """One context, consecutive calls, every position of every call against the oracle: routes, the device view's arrays, and
    once per case the packed payloads and download() at 18 positions.

    The thresholds the cases rely on, as the code has them (each case's comment in CASES says which it crosses):
      lfx_internal.hpp  `scan_count_from = 256`, and lfx_api.hip run_batch `batch >= c->scan_count_from && count_lds <= 144u * 1024u`:
                        the holes form's count pass is scan_count_kernel for the 1 024 / 1 000-scan batches of the holes cases;
      lfx_api.hip choose_route  `guess = (was_fused ? 2u * fell : 0u) + 8u; ch.fb_grid = guess < batch && ... ? guess : batch`:
                        the first call of an unhinted context sizes the bucketing launches for 8 list entries ("holes, found",
                        "turned rings, found" and "records missing" put their whole first batch on that list);
      choose_route      `ch.short_tail = was_fused && of && fell == 0 ...` and run_batch `lazy = fused && short_tail && !choice.xform`:
                        fallback_tail_kernel is the tail from the second call of a stream that has not been falling back;
      lfx_kernels_extract.hpp  `kTailMaxTurns = 128`, run_batch `turns = (batch + kTailMaxTurns - 1) / kTailMaxTurns`: 8 rows
                        of that kernel's grid at 1 024 scans ("odd scans out", call 1: 15 list entries);
      run_batch         `self_totals = (fused || (uint64_t)batch * c->max_rings <= 8192u) && ...`: ring_totals_kernel runs for a
                        batch that is not fused and has more than 8 192 rings ("records missing" from its second call on:
                        512 x 64 = 32 768).
    Where the kernel table can tell (kernel_times: launch counts, not times), the case asserts the launch happened."""
    import torch
    distinct, exp = prepare(case)
    kinds = [d.kind for d in distinct]
    f = FeatureExtraction(case.hp, device=0, max_points_per_scan=case.rings * case.cols, max_batch=max(case.sizes),
                          max_points_per_ring=case.cols, max_rings=case.rings, drop_zero_points=case.drop_zero, outputs=case.outputs,
                          stream_hint=case.hint)
    try:
        if case.launches:
            f.set_profiling(True)
        dev = [torch.from_numpy(d.cloud.view(np.uint8).copy()).to("cuda:0") for d in distinct]
        st = torch.cuda.current_stream().cuda_stream
        rng = np.random.default_rng(case.seed)
        for call, B in enumerate(case.sizes):
            ctx = "%s, call %d of %d scans" % (case.name, call, B)
            pick = np.asarray(rng.integers(0, len(distinct), B) if case.arrange is None else case.arrange(rng, call, B, kinds), np.int64)
            batch = torch.cat([dev[u] for u in pick])
            f.extract_batch_device(batch.data_ptr(), exp.n_points[pick].astype(np.uint32), st)
            routes = f.scan_routes(B, st)
            f.batch_status(st)
            want_routes = np.array([case.route(call, kinds[u]) for u in pick], np.uint8)
            bad = np.nonzero(routes != want_routes)[0]
            assert bad.size == 0, "%s: %d scans on another route than expected, first position %d (distinct scan %d, %s): %d, expected %d" % (
                ctx, bad.size, bad[0], pick[bad[0]], kinds[pick[bad[0]]], routes[bad[0]], want_routes[bad[0]])
            n = LS.assert_batch_equal(f, pick, exp, ctx, curvature=case.curvature)
            assert n == B, "%s: %d of %d positions compared" % (ctx, n, B)
            print("%s: %d positions equal, routes %s" % (ctx, n, {int(r): int(k) for r, k in zip(*np.unique(routes, return_counts=True))}))
            if call == len(case.sizes) - 1 or (case.name == "odd scans out" and call == 1):
                LS.assert_packed_equal(f, pick, exp, ctx)
                for s in sorted(set(int(p) for p in np.linspace(0, B - 1, 18))):
                    check_download(case, f.download(s, st), distinct[pick[s]], "%s, download(%d)" % (ctx, s))
            del batch
        if case.launches:
            times = f.kernel_times()
            for name in case.launches:
                assert times[name][1] > 0, "%s: %s was never launched: %s" % (case.name, name, {k: v[1] for k, v in times.items()})
    finally:
        f.close()


def test_host_api_at_512_scans():
    """16 x 1 800 x 512 through extract_batch from pageable memory: staging, fetch plans and pinned result blocks at 512 scans,
    every scan of three calls with assert_scan_equal."""
    rings, cols, U = 16, 1800, 13
    clouds = [make_scan(rings, cols, seed=10100 + i) for i in range(U)]
    want = [OB.extract(c, canonical_ties=False) for c in clouds]
    for u, w in enumerate(want):
        LS.require_tie_free(w, "host API: distinct scan %d" % u)
    f = FeatureExtraction(device=0, max_points_per_scan=rings * cols, max_batch=512, max_points_per_ring=cols, max_rings=rings)
    try:
        rng = np.random.default_rng(3)
        for call, B in enumerate(B512):
            pick = rng.integers(0, U, B)
            got = f.extract_batch([clouds[u] for u in pick])
            assert len(got) == B
            for s, u in enumerate(pick):
                assert_scan_equal(got[s], want[u], "host API, call %d, position %d (distinct scan %d)" % (call, s, u))
    finally:
        f.close()


@pytest.mark.timeout(900)
def test_stress_slice_batches():
    """A seeded slice of the randomised BATCH cases (tests/stress_cases.py draw_batch; the long sweep is tools/stress.py
    --batches): 3 .. 64 scans of 2 .. 7 distinct contents in a drawn arrangement, three calls, every position against the
    oracle.  The draw count has to fit into a tenth of the rest of the -m gpu suite's wall time: 24 draws took 3.1 s where
    the rest of the suite took 104 s."""
    from tests.stress_cases import run_batch_cases
    seen = run_batch_cases(STRESS_BATCH_DRAWS, seed=20261016)
    assert sum(seen.values()) == STRESS_BATCH_DRAWS, seen



if __name__ == "__main__":
    import time
    for case in CASES:
        t0 = time.time()
        distinct, exp = prepare(case)
        print("%-28s %3d distinct scans, tie-free, %5.1f s; edge %s surface %s" % (
            case.name, len(distinct), time.time() - t0, exp.n_edge.tolist()[:4], exp.n_surface.tolist()[:4]), flush=True)
