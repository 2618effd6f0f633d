"""Cases and restatement for the alignment loop BEYOND its first iteration (tests/test_align_iterations_expect.py,
tests/test_align_iterations_gpu.py).  Seeded, no GPU, nothing read from outside the repository.

tests/align_step_restatement.restate_step restates one call of the optimizer with max_iter = 1.  restate_iteration puts the
stopping tests of iteration m around it (optimizer.hpp:97-108 and the three ends of the loop), so that a chain of them, each
fed with the rows at the pose the one before left and with ITS error and scale as prev_error and prev_scale, restates
Optimizer::Run(max_iter = m) one iteration at a time.  What the device's warm-started map searches must then reproduce is
every single step of the chain to restate_step's derived bound -- a search that loses one true neighbour of one query moves
the step by orders more (tests/test_align_iterations_expect.py asserts that) while the converged pose hardly notices.

Clouds: 160 edge and 320 surface points spread over the scans of align_step_cases.mixed_scene(), against its maps, drawn
anew for every (start, n_neighbors).  Start poses from centimetres to metres off, one turned by 8 degrees, one 300 m away (every query outside the grid), so that the
bound a warm search starts from -- (distance of the 16th neighbour at the search before + the query's movement since) / cell
size -- falls into every class the search kernel treats differently (coverage())."""
import ctypes as C

import numpy as np

from tests import align_step_cases as AC
from tests.align_step_restatement import (CONVERGED, DBL_MAX, EMPTY, LARGER_ERROR, LARGER_SCALE, MAX_ITERATION, NO_PLANE, U,
                                          pose_of, restate_step)
from tests.report_restatement import quaternion_of

CONTINUES = -1                                           # the code of an iteration after which the loop goes on
NEIGHBOURS = (15, 5, 16)
CELL_PAIRS = ((1.0, 2.0), (0.4, 0.8), (0.0, 0.0))        # (edge map's cell, surface map's); 0: no grid, no warm start -- the control
MAX_ITERS = (1, 2, 3, 4, 5)
N_EDGE, N_SURFACE = 160, 320
LIST_LENGTH = 16                                         # the searches keep 16 neighbours whatever n_neighbors is: reach[] is the 16th's distance
MIN_GAP = 1e-6                                           # metres between the k-th and the (k + 1)-th neighbour's distances
BANDS = ("x <= 1", "1.5 < x <= 2", "2.5 < x <= 3", "x > 3.5")
PD, PF = AC.PD, AC.PF


def start_poses():
    """(name, 3 x 4 pose) of the starts; the scans were taken where the maps were, so each is how far off the start is."""
    turn = np.deg2rad(8.0) * np.array([0.2, -0.3, 0.9327379053088815])
    far = np.array([0.05, -0.03, 0.1])
    return [("3 cm", AC.translation((1 / 32, -1 / 64, 1 / 128))),
            ("1.2 m", AC.translation((0.75, -0.875, 0.3125))),
            ("2.5 m", AC.translation((2.25, 1.0, -0.5))),
            ("6 m", AC.translation((-4.5, 3.75, 1.25))),
            ("8 degrees", np.ascontiguousarray(np.hstack([AC._rotation(turn), np.array([[0.25], [-0.125], [0.0625]])]))),
            # (along one axis: from a diagonal every query sees the same corner of the map and the problem is degenerate)
            ("300 m", np.ascontiguousarray(np.hstack([AC._rotation(far), np.array([[300.0], [0.0], [0.0]])]))),
            # (near enough for a step below the convergence threshold within five iterations: its draws are those that end so)
            ("1.6 cm", AC.translation((1 / 64, 1 / 128, -1 / 256)))]


# Which draw of a (start, n_neighbors)'s clouds is used: the first one for which, at every pose its restated chain passes
# through, every query's k-th and (k + 1)-th nearest map points differ in distance by more than MIN_GAP -- otherwise which of
# them is the neighbour would hang on the pose's last bits.  (A few queries in ten thousand sit that close, so a chain of
# six poses and 480 queries is clear of them about one time in three, and far less often from 300 m, where all distances
# crowd together.)  The draw also has no iteration that restate_step would exclude or that ties with the error or scale
# before it, and no residual at the Huber threshold at a returned pose.  Found with the oracle's rows and cKDTree;
# tests/test_align_iterations_expect.py asserts gap and exclusions for the draws named here.  (The 1.6 cm start takes the first such draw whose chain ends CONVERGED after at least one full iteration: noise
# ends most runs from nearby with LARGER_ERROR or LARGER_SCALE.)
DRAW = {("3 cm", 15): 4, ("1.2 m", 15): 0, ("2.5 m", 15): 10, ("6 m", 15): 8, ("8 degrees", 15): 1, ("300 m", 15): 4,
        ("3 cm", 5): 0, ("1.2 m", 5): 1, ("2.5 m", 5): 8, ("6 m", 5): 3, ("8 degrees", 5): 1, ("300 m", 5): 8, ("small maps", 5): 0,
        ("3 cm", 16): 2, ("1.2 m", 16): 12, ("2.5 m", 16): 6, ("6 m", 16): 5, ("8 degrees", 16): 1, ("300 m", 16): 26,
        ("1.6 cm", 15): 7, ("1.6 cm", 5): 6, ("1.6 cm", 16): 10}
NAMES = ("3 cm", "1.2 m", "2.5 m", "6 m", "8 degrees", "300 m", "small maps", "1.6 cm")


def clouds_of(s, name, k):
    """The edge and the surface cloud of a (start, k): N_EDGE and N_SURFACE points spread over the scene's clouds."""
    rng = np.random.default_rng([2027, NAMES.index(name), k, DRAW.get((name, k), 0)])
    return (np.ascontiguousarray(s["edge"][rng.permutation(len(s["edge"]))[:N_EDGE]]),
            np.ascontiguousarray(s["surface"][rng.permutation(len(s["surface"]))[:N_SURFACE]]))


def scene():
    """align_step_cases.mixed_scene() with the maps of the small-map case."""
    s = AC.mixed_scene()
    # fewer than 16 map points: the 16th list entry stays infinite, the bound "none" at every iteration.  The points of a
    # small patch of each map (a dozen scattered points would span no line and no plane worth the name)
    e_at, s_at = s["edge_map"][1000, :3], s["surface_map"][2000, :3]
    s["small_edge_map"] = np.ascontiguousarray(s["edge_map"][np.argsort(np.linalg.norm(s["edge_map"][:, :3] - e_at, axis=1))[:12]])
    s["small_surface_map"] = np.ascontiguousarray(s["surface_map"][np.argsort(np.linalg.norm(s["surface_map"][:, :3] - s_at, axis=1))[:14]])
    return s


def cases(s, k):
    """The scans of one n_neighbors: dict(name, edge, surface, pose, maps) with maps "scene" (the scene's edge and surface map)
    or "small" (the maps of fewer than 16 points, k = 5 only)."""
    out = []
    for name, pose in start_poses():
        e, f = clouds_of(s, name, k)
        out.append(dict(name=name, edge=e, surface=f, pose=pose, maps="scene"))
    if k == 5:
        e, f = clouds_of(s, "small maps", k)
        out.append(dict(name="small maps", edge=e[:40], surface=f[:80], pose=AC.translation((0.125, -0.0625, 0.03125)), maps="small"))
    return out


def maps_of(s, case):
    return (s["edge_map"], s["surface_map"]) if case["maps"] == "scene" else (s["small_edge_map"], s["small_surface_map"])


def empty_case():
    none = np.zeros((0, 4), np.float32)
    return dict(name="empty", edge=none, surface=none, pose=AC.translation((0.25, 0.0, -4.0)), maps="any")


def no_plane_case(s):
    """Against scene["coincident_map"]: surface points well inside the half whose map points come in clusters of 16 coincident
    ones (the k <= 16 nearest of such a point are one cluster: no plane, the zero row) -- every surface row is the zero row."""
    surf = s["surface"]
    pts = np.ascontiguousarray(surf[surf[:, 1] > 2.5][:120], np.float32)
    return dict(name="no plane", edge=np.ascontiguousarray(s["edge"][:37], np.float32), surface=pts, pose=AC.translation((1 / 64, 1 / 128, -1 / 128)),
                maps="coincident")


# ---- the restatement of iteration m ----------------------------------------------------------------------------------------

def restate_iteration(pose_before, rows, prev_error, prev_scale, last, m=1):
    """Iteration m (1-based) of Optimizer::Run from `pose_before` on `rows` = (r3, J3, r1, J1) at that pose, with the error and
    the scale of iteration m - 1 (numeric_limits::max() for m = 1), in the optimizer's order: error > prev_error ends it with
    LARGER_ERROR, else scale > prev_scale with LARGER_SCALE -- both at iteration m - 1 with the pose as it was --, else the
    step is taken and ends it with CONVERGED at m - 1 if it was short, with MAX_ITERATION at m if `last`; otherwise the loop
    goes on (code CONTINUES).  restate_step's dict with these fields replaced, its `excluded` flags carried, and near_stop: the
    error or the scale within 1e-7 (relative) of the one before -- which stopping test fires is then a matter of rounding."""
    want = restate_step(pose_before, *rows)
    P = np.asarray(pose_before, np.float64).reshape(3, 4)
    unmoved = pose_of(quaternion_of(P[:, :3]), P[:, 3].copy())
    want.update(near_stop=False, no_step=True)
    if want["code"] in (EMPTY, NO_PLANE):
        want["iteration"] = m - 1
        return want
    error, scale = want["error"], want["error_scale"]
    want["near_stop"] = bool(abs(error - prev_error) <= 1e-7 * abs(error) or abs(scale - prev_scale) <= 1e-7 * abs(scale))
    stopped = LARGER_ERROR if error > prev_error else (LARGER_SCALE if scale > prev_scale else None)
    if stopped is not None:
        want.update(code=stopped, iteration=m - 1, pose=unmoved, bound=0.0, dx_norm=0.0, no_step=True,
                    pose_bound=16 * U * (1.0 + np.abs(unmoved).max()))
        return want
    want["no_step"] = bool(want["degenerate"])
    if want["code"] == CONVERGED:
        want["iteration"] = m - 1
    elif last:
        want.update(code=MAX_ITERATION, iteration=m)
    else:
        want.update(code=CONTINUES, iteration=m)
    return want


def oracle_rows_at(maps, case, pose, k):
    r3, J3 = AC.oracle_rows(maps[0], 0, pose, case["edge"], k)
    r1, J1 = AC.oracle_rows(maps[1], 1, pose, case["surface"], k)
    return r3, J3, r1, J1


def chain(rows_at, start, max_m=5):
    """The restated loop from `start`: steps[j] is iteration j + 1 restated with last = False on rows_at(pose before it), up
    to the first one that stops or to `max_m`.  rows_at: pose -> (r3, J3, r1, J1)."""
    steps, pose, prev_error, prev_scale = [], np.ascontiguousarray(start, np.float64), DBL_MAX, DBL_MAX
    for m in range(1, max_m + 1):
        want = restate_iteration(pose, rows_at(pose), prev_error, prev_scale, False, m)
        want["pose_before"] = pose
        steps.append(want)
        if want["code"] != CONTINUES:
            break
        pose, prev_error, prev_scale = np.ascontiguousarray(want["pose"]), want["error"], want["error_scale"]
    return steps



def result_of(steps, m):
    """What a call with max_iter = m returns, from chain(): (the step that ends it as restate_iteration(..., last = True)
    gives it, its index in steps)."""
    j = min(m, len(steps)) - 1
    want = dict(steps[j])
    if want["code"] == CONTINUES:                          # j = m - 1: the limit ends it
        want.update(code=MAX_ITERATION, iteration=m)
    return want, j


def oracle_loop(maps, case, k, max_iter):
    """orc_loc_optimize_scan(start, max_iter)."""
    from oracle import binding as OB
    em, sm, e, f = (np.ascontiguousarray(a, np.float32) for a in (maps[0], maps[1], case["edge"], case["surface"]))
    pose = np.ascontiguousarray(case["pose"], np.float64)
    out, err, scale, it, code = np.zeros(12), C.c_double(), C.c_double(), C.c_int(), C.c_int()
    ok = OB.lib().orc_loc_optimize_scan(OB.ptr(em, PF), len(em), OB.ptr(sm, PF), len(sm), k, OB.ptr(e, PF), len(e), OB.ptr(f, PF), len(f),
                                        OB.ptr(pose, PD), max_iter, OB.ptr(out, PD), C.byref(err), C.byref(scale), C.byref(it), C.byref(code))
    return dict(pose=out.reshape(3, 4), error=err.value, error_scale=scale.value, iteration=it.value, code=code.value, success=bool(ok))


# ---- preconditions and coverage, from the reference side only --------------------------------------------------------------

_TREES = {}


def _tree(map_points):
    from scipy.spatial import cKDTree
    key = (id(map_points), len(map_points))
    if key not in _TREES:
        _TREES[key] = (cKDTree(np.asarray(map_points, np.float64)[:, :3]), map_points)       # (the array kept: its id stays its own)
    return _TREES[key][0]


def moved(pose, points):
    P = np.asarray(pose, np.float64).reshape(3, 4)
    return np.asarray(points, np.float64)[:, :3] @ P[:, :3].T + P[:, 3]


def nearest_distances(map_points, pose, points, count):
    """[n][count] ascending distances of the points at `pose` to their nearest map points (infinity beyond the map's size)."""
    if not len(points):
        return np.zeros((0, count))
    d, _ = _tree(map_points).query(moved(pose, points), k=count)
    return np.asarray(d, np.float64).reshape(len(points), count)


def smallest_gap(maps, case, pose, k):
    """The smallest difference between the k-th and the (k + 1)-th nearest map distance over the scan's queries at `pose`."""
    gaps = [np.inf]
    for m, pts in ((maps[0], case["edge"]), (maps[1], case["surface"])):
        d = nearest_distances(m, pose, pts, k + 1)
        if len(d):
            with np.errstate(invalid="ignore"):
                g = d[:, k] - d[:, k - 1]
            gaps.append(float(np.nanmin(np.where(np.isfinite(d[:, k]), g, np.inf))))
    return min(gaps)


def warm_searches(steps, max_iters=MAX_ITERS):
    """The warm-started searches the calls with max_iter in `max_iters` run for one scan, from its chain(): a list of
    (where, pose of the search before, pose the kernel measures the movement from, pose searched at), `where` = "loop" or
    "report", each distinct search once.  In the loop: iteration j > 0 searches at the pose step j left, from reach[] and
    prev_m of the pose before.  The report searches at the returned pose: after a step (CONVERGED, MAX_ITERATION) reach[] and
    prev_m are of the pose the step started from; after LARGER_ERROR / LARGER_SCALE reach[] is of the returned pose itself and
    prev_m one pose behind it."""
    seen, out = set(), []
    for j in range(1, len(steps)):
        out.append(("loop", steps[j - 1]["pose_before"], steps[j - 1]["pose_before"], steps[j]["pose_before"]))
    for m in max_iters:
        want, j = result_of(steps, m)
        if want["code"] in (EMPTY, NO_PLANE) or (j, want["code"]) in seen:
            continue
        seen.add((j, want["code"]))
        if want["code"] in (LARGER_ERROR, LARGER_SCALE):
            out.append(("report", want["pose_before"], steps[j - 1]["pose_before"], want["pose_before"]))
        else:
            out.append(("report", want["pose_before"], want["pose_before"], want["pose"]))
    return out


def new_coverage():
    return {(where, kind): dict({b: 0 for b in BANDS}, outside=0) for where in ("loop", "report") for kind in ("edge", "surface")}


def count_coverage(total, maps, cells, case, steps):
    """Adds the queries of one scan's warm searches to `total`.  x = (d16 + move) / h with d16 the distance of the 16th
    nearest map point at the search before and move the distance the kernel adds for the query's movement.  The kernel
    enlarges its first cube to need = ceil(x - g0) cells, g0 in [0, 0.5] the query's distance to the nearest face of its
    cell: x <= 1 gives none, 1.5 < x <= 2 gives 2, 2.5 < x <= 3 gives 3 and x > 3.5 gives 4 or more (a bounded start at
    rho = 1) wherever the grid's origin lies.  Only queries inside the map's bounding box count for the bands (outside it the
    first cube is as large as the query is far); `outside`: queries more than one cell outside it."""
    for where, reach_pose, from_pose, at_pose in warm_searches(steps):
        for kind, m, h, pts in (("edge", maps[0], cells[0], case["edge"]), ("surface", maps[1], cells[1], case["surface"])):
            if h <= 0 or len(m) < LIST_LENGTH or not len(pts):
                continue
            d16 = nearest_distances(m, reach_pose, pts, LIST_LENGTH)[:, LIST_LENGTH - 1]
            q = moved(at_pose, pts)
            x = (d16 + np.linalg.norm(q - moved(from_pose, pts), axis=1)) / h
            lo, hi = np.asarray(m, np.float64)[:, :3].min(0), np.asarray(m, np.float64)[:, :3].max(0)
            out_by = np.maximum(np.maximum(lo - q, q - hi), 0.0).max(1)
            inside = out_by == 0.0
            t = total[(where, kind)]
            t["outside"] += int((out_by > h).sum())
            for b, sel in zip(BANDS, (x <= 1.0, (x > 1.5) & (x <= 2.0), (x > 2.5) & (x <= 3.0), x > 3.5)):
                t[b] += int((sel & inside).sum())
    return total


def coverage_ok(total):
    return all(t[b] >= 8 for t in total.values() for b in BANDS + ("outside",))


_CHAINS = {}


def oracle_chains(s, k):
    """[(case, maps, chain on the oracle's rows)] of one n_neighbors, computed once."""
    if k not in _CHAINS:
        out = []
        for case in cases(s, k):
            maps = maps_of(s, case)
            out.append((case, maps, chain(lambda pose, c=case, mp=maps: oracle_rows_at(mp, c, pose, k), case["pose"])))
        _CHAINS[k] = out
    return _CHAINS[k]


def stopping_iterations(steps_of_scans, m):
    """The iterations at which the scans of one call with max_iter = m stop, from their chains."""
    return sorted(set(result_of(steps, m)[0]["iteration"] for steps in steps_of_scans))


def without_neighbour(map_points, pose, point, rank):
    """The map without the `rank`-th nearest point (1-based) of the scan point at `pose`: its next one moves up."""
    d = np.linalg.norm(np.asarray(map_points, np.float64)[:, :3] - moved(pose, np.asarray(point).reshape(1, -1))[0], axis=1)
    return np.ascontiguousarray(np.delete(map_points, np.argsort(d, kind="stable")[rank - 1], axis=0))
