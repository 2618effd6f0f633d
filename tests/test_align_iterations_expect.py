"""The cases of the alignment loop's later iterations (tests/align_iteration_cases.py) and the chained restatement against
the CPU oracle alone, without a GPU: what tests/test_align_iterations_gpu.py holds the device to is itself held to
orc_loc_optimize_scan, and the conditions under which that comparison means something are asserted here from the reference
side only -- no near-tie between a k-th and a (k + 1)-th neighbour at any pose, next to no iteration excluded, every class
of warm-start bound met by enough queries, a batch whose scans stop at different iterations, and the test's power: one wrong
neighbour of one query moves a step by far more than the bound the device is held to."""
import numpy as np
import pytest

from tests import align_iteration_cases as IC
from tests.align_step_restatement import EMPTY, NO_PLANE, restate_step
from tests.report_restatement import restate


@pytest.fixture(scope="module")
def scene():
    return IC.scene()


@pytest.mark.parametrize("k", IC.NEIGHBOURS)
def test_the_chained_restatement_reproduces_the_oracle_s_loop(scene, k):
    """restate_iteration chained on the oracle's rows at the pose before, against orc_loc_optimize_scan(start, m) for m = 1..5:
    code and iteration equal, the pose within the restatement's pose_bound, error and scale to 1e-7.  No pose of a chain has a
    query whose k-th and (k + 1)-th neighbours are within 1e-6 m, and at most 1 in 16 iterations is excluded."""
    checked, excluded, near_stop, worst, gap = 0, 0, 0, (0.0, ""), (np.inf, "")
    for case, maps, steps in IC.oracle_chains(scene, k):
        for m in IC.MAX_ITERS:
            want, _ = IC.result_of(steps, m)
            what = "%s, k = %d, m = %d" % (case["name"], k, m)
            got = IC.oracle_loop(maps, case, k, m)
            checked += 1
            excluded += int(want["excluded"] or want["near_stop"])
            near_stop += int(want["near_stop"])
            for pose in (want["pose_before"], want["pose"]):
                gap = min(gap, (IC.smallest_gap(maps, case, pose, k), what))
            assert (got["code"], got["iteration"]) == (want["code"], want["iteration"]), (what, got, want["code"], want["iteration"])
            diff = float(np.abs(got["pose"] - want["pose"]).max())
            assert diff <= want["pose_bound"], (what, diff, want["pose_bound"])
            worst = max(worst, (diff / want["pose_bound"], what))
            assert abs(got["error"] - want["error"]) <= 1e-7 * abs(want["error"]) + 1e-18, what
            assert abs(got["error_scale"] - want["error_scale"]) <= 1e-7 * abs(want["error_scale"]) + 1e-18, what
    print("k = %d: %d (case, m) pairs, %d excluded (%d near a stopping tie); the oracle's worst |dP| / pose_bound %.3g (%s); "
          "the smallest gap %.3g m (%s)" % ((k, checked, excluded, near_stop) + worst + gap))
    assert gap[0] > IC.MIN_GAP, ("choose another input", gap)
    assert 16 * excluded <= checked, ("choose another input", excluded, checked)


def test_every_class_of_warm_start_bound_is_met(scene):
    """From the restated chains: the warm-started searches of the loop and those of the report each meet every class of
    (d16 + move) / cell size with at least 8 edge and 8 surface queries, and at least 8 of each lie more than a cell outside
    the map's bounding box; from m = 3 on the scans of a batch (the empty scan among them) stop at three or more different
    iterations; and the chains end in every way a loop can end after its first iteration."""
    total = IC.new_coverage()
    for cells in IC.CELL_PAIRS:
        for k in IC.NEIGHBOURS:
            for case, maps, steps in IC.oracle_chains(scene, k):
                if case["maps"] == "scene":
                    IC.count_coverage(total, maps, cells, case, steps)
    for key, counts in total.items():
        print("warm searches of the %s, %s queries:" % key, counts)
    assert IC.coverage_ok(total), ("choose another input", total)
    codes = set()
    for k in IC.NEIGHBOURS:
        chains = [steps for case, _, steps in IC.oracle_chains(scene, k) if case["maps"] == "scene"]
        codes |= set((steps[-1]["code"], len(steps) >= 2) for steps in chains)
        for m in IC.MAX_ITERS:
            stops = sorted(set(IC.stopping_iterations(chains, m) + [0]))         # (+ the empty scan: iteration 0)
            print("k = %d, max_iter = %d: the scans of the batch stop at iterations" % (k, m), stops)
            assert m < 3 or len(stops) >= 3, ("choose another input", k, m, stops)
    # every way the loop ends after its first iteration: CONVERGED, LARGER_ERROR, LARGER_SCALE, and the limit
    print("the chains end with (code, beyond the first iteration)", sorted(codes))
    assert codes >= {(0, True), (1, True), (2, True), (IC.CONTINUES, True)}, ("choose another input", codes)


def test_the_small_maps_the_empty_scan_and_the_scan_without_a_plane(scene):
    """The maps of the small-map case have fewer than 16 points and still carry steps; the empty scan is EMPTY; every surface
    row of the no-plane scan against the coincident map is the zero row for every n_neighbors, and the oracle's loop says
    NO_PLANE at iteration 0."""
    assert 5 <= len(scene["small_edge_map"]) < IC.LIST_LENGTH and 5 <= len(scene["small_surface_map"]) < IC.LIST_LENGTH
    small = [(c, steps) for c, _, steps in IC.oracle_chains(scene, 5) if c["maps"] == "small"]
    assert len(small) == 1 and len(small[0][1]) >= 3 and not small[0][1][0]["degenerate"], "the small maps carry no steps"
    empty = IC.empty_case()
    want = IC.restate_iteration(empty["pose"], (np.zeros((0, 3)), np.zeros((0, 21)), np.zeros(0), np.zeros((0, 7))), IC.DBL_MAX, IC.DBL_MAX, True)
    assert (want["code"], want["iteration"]) == (EMPTY, 0)
    case = IC.no_plane_case(scene)
    maps = (scene["edge_map"], scene["coincident_map"])
    assert len(case["surface"]) >= 100 and len(case["edge"]) > 0
    for k in IC.NEIGHBOURS:
        rows = IC.oracle_rows_at(maps, case, case["pose"], k)
        assert not rows[3].any() and not rows[2].any(), k
        want = IC.restate_iteration(case["pose"], rows, IC.DBL_MAX, IC.DBL_MAX, True)
        got = IC.oracle_loop(maps, case, k, 5)
        assert (want["code"], want["iteration"]) == (NO_PLANE, 0) == (got["code"], got["iteration"]), (k, got)


def test_one_wrong_neighbour_moves_a_step_by_far_more_than_its_bound(scene):
    """The power of the device test, not a tolerance: at the 2.5 m start, first step, k = 15, a query that takes its 16th
    nearest map point for its 15th moves the restated pose by more than 100 pose_bound and the information matrix by more
    than 100 x 1e-9 (the report test's bound) -- for each of eight edge and eight surface queries tried one at a time."""
    k = 15
    case, maps, _ = [c for c in IC.oracle_chains(scene, k) if c[0]["name"] == "2.5 m"][0]
    pose = case["pose"]
    rows = IC.oracle_rows_at(maps, case, pose, k)
    base, base_h = restate_step(pose, *rows), restate(pose, *rows)["information"]
    least = dict(pose=np.inf, information=np.inf)
    for kind, pts, at in ((0, case["edge"], 0), (1, case["surface"], 2)):
        for i in range(0, 8 * 20, 20):
            lesser = IC.without_neighbour(maps[kind], pose, pts[i], k)
            r, J = IC.AC.oracle_rows(lesser, kind, pose, pts[i:i + 1], k)
            wrong = [a.copy() for a in rows]
            assert wrong[at][i].tobytes() != r[0].tobytes(), (kind, i)
            wrong[at][i], wrong[at + 1][i] = r[0], J[0]
            moved = float(np.abs(restate_step(pose, *wrong)["pose"] - base["pose"]).max()) / base["pose_bound"]
            h = restate(pose, *wrong)["information"]
            moved_h = float(np.linalg.norm(h - base_h) / np.linalg.norm(base_h)) / 1e-9
            print("%s query %d with its 16th neighbour for its 15th: the pose moves by %.3g pose_bound, H by %.3g x 1e-9" % (
                ("edge", "surface")[kind], i, moved, moved_h))
            least = dict(pose=min(least["pose"], moved), information=min(least["information"], moved_h))
    assert least["pose"] > 100.0 and least["information"] > 100.0, least
