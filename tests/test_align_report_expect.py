"""lfx_align_report's cases and restatements on the host, before a GPU sees them (tests/align_report_cases.py,
tests/align_report_reference.py), on the rows the CPU oracle gives at every case's start pose.

Every case is what it claims: the ranks of the ladder, the two windows about the covariance's floor, the H that is diagonal
with repeated eigenvalues, the tie under the sign rule, the margins from the Huber threshold (at most 1 selection case in
16 excluded, 6 144 and 6 145 rows among the compared), from the floor and from IsDegenerate's 0.1, the condition's cap, the
tiny scans without a degree of freedom.  And the chain's first link: report_restatement.restate and
align_report_reference.algorithm / algorithm_d against the 50-digit reference within the constants the cases file records.
Every test prints its figures before it asserts."""
import math

import numpy as np
import pytest

from tests import align_report_cases as RC
from tests import align_report_reference as RR
from tests import align_step_cases as AC
from tests.report_restatement import restate

NAMES = RC.all_names()
HAND = list(RC.HAND)


def _ref(name):
    return RC.host_reference(name)[1]


@pytest.mark.parametrize("name", NAMES)
def test_restatements_against_the_reference(name):
    sums, eig, d_ratio, near = RC.measure()[name]
    rows, ref = RC.host_reference(name)
    case = [c for c in RC.selection_cases() + RC.hand_cases() if c["name"] == name][0]
    alg = RR.algorithm(ref["information"], ref["sigma2"])
    print(name, "rows", ref["n_edge"], ref["n_surface"], "sums", sums, "eigen", eig, "D %.3g" % d_ratio, "rank", ref["rank"],
          "Huber margin %.3g" % ref["huber_margin"], "floor margins", ref["floor_margin"], "gaps", ref["gaps"])
    for k, v in sums.items():
        assert v <= RC.C_SUM, (name, k, v)
    assert eig["eigenvalues"] <= RC.C_EIG and eig["vectors"] <= RC.C_EIG and d_ratio <= RC.C_EIG, (name, eig, d_ratio)
    assert eig.get("covariance", 0.0) <= RC.C_COV, (name, eig)
    assert alg["settled"] and RR.algorithm_d(ref["D"])[1]
    # IsDegenerate's decision is not a matter of rounding in any case
    assert abs(ref["min_eigenvalue_d"] - 0.1) > RC.d_bound(ref), (name, ref["min_eigenvalue_d"], RC.d_bound(ref))
    # what the algorithm promises of its own output, exactly
    lam, vec = alg["eigenvalues"], alg["eigenvectors"]
    assert np.all(np.diff(lam) >= 0) and np.abs(vec @ vec.T - np.eye(6)).max() <= 1e-14
    assert all(vec[k][int(np.argmax(np.abs(vec[k])))] > 0 for k in range(6))
    assert RR.same_bits(alg["covariance"], alg["covariance"].T)
    if min(ref["floor_margin"]) > 1e-3:
        assert alg["rank"] == ref["rank"], (name, lam)
    if not near:
        want = restate(case["pose"], *rows)
        assert (want["n_edge_inliers"], want["n_surface_inliers"], want["n_surface_no_plane"]) == \
            (ref["n_edge_inliers"], ref["n_surface_inliers"], ref["n_surface_no_plane"])
        assert math.isnan(want["sigma2"]) == math.isnan(ref["sigma2"]) == (not ref["dim"] > 0)


def test_the_recorded_constants_are_the_measured_ones():
    seen = RC.measure()
    c_sum = max(max(list(v[0].values()) + [0.0]) for v in seen.values())
    c_eig = max(max(v[1]["eigenvalues"], v[1]["vectors"], v[2]) for v in seen.values())
    c_cov = max(v[1].get("covariance", 0.0) for v in seen.values())
    print("measured C_SUM %.3g C_EIG %.3g C_COV %.3g; recorded %g %g %g" % (c_sum, c_eig, c_cov, RC.C_SUM, RC.C_EIG, RC.C_COV))
    for measured, recorded in ((c_sum, RC.C_SUM), (c_eig, RC.C_EIG), (c_cov, RC.C_COV)):
        assert measured <= recorded <= 1.25 * measured, "the record in align_report_cases.py is stale"


def test_the_selection_cases_keep_clear_of_the_huber_threshold():
    cases = [c for c in RC.selection_cases() if c["n3"] + c["n1"] > 0]
    near = [c["name"] for c in cases if _ref(c["name"])["huber_margin"] <= RC.HUBER_MARGIN]
    print("%d of %d selection cases within %g of 1.345^2: %s" % (len(near), len(cases), RC.HUBER_MARGIN, near))
    assert 16 * len(near) <= len(cases)
    assert [a + b for a, b in AC.SPLIT_COUNTS] == [6144, 6145]
    for n3, n1 in AC.SPLIT_COUNTS:
        assert "n3 = %d, n1 = %d" % (n3, n1) not in near
    zero = _ref([c["name"] for c in cases if c["name"].startswith("zero rows")][0])
    assert AC.bits(zero["error_scale"]) == AC.bits(0.0) and 2 * zero["n_surface_no_plane"] > zero["n_edge"] + zero["n_surface"]


def test_the_tiny_cases_without_a_degree_of_freedom():
    without, with_ = [], []
    for n3, n1 in AC.TINY_COUNTS:
        if n3 + n1 == 0:
            continue
        ref = _ref("n3 = %d, n1 = %d" % (n3, n1))
        (with_ if ref["dim"] > 0 else without).append((n3, n1, ref["dim"]))
        # exactly 0 only where every weight is 1: the sum is then one of small integers, exact in any order
        assert abs(ref["dim"]) > 1e-9 or (ref["dim"] == 0.0 and np.all(ref["weights"] == 1.0)), "sum w dim - 6 sits on 0 (choose another input)"
        assert math.isnan(ref["sigma2"]) == (not ref["dim"] > 0) and np.isnan(ref["covariance"]).all() == (not ref["dim"] > 0)
        assert np.isfinite(ref["information"]).all() and ref["eigenvalues"][5] > 0
    print("sum w dim - 6 <= 0:", without, "> 0:", with_)
    assert len(without) >= 8 and len(with_) >= 1
    assert all(3 * n3 + n1 > 6 for n3, n1, _ in with_)                      # (no scan of six rows or fewer has a degree of freedom left)


@pytest.mark.parametrize("name", HAND)
def test_a_hand_scene_is_what_it_claims(name):
    ref = _ref(name)
    case = [c for c in RC.hand_cases() if c["name"] == name][0]
    lam = ref["eigenvalues"]
    print(name, "rows", case["n3"], case["n1"], "map", len(case["edge_map"]), len(case["surface_map"]), "rank", ref["rank"], "eigenvalues", lam,
          "scale", ref["error_scale"], "inliers", ref["n_edge_inliers"], ref["n_surface_inliers"], "min eigenvalue of D", ref["min_eigenvalue_d"],
          "cond", ref["cond"], "Huber margin", ref["huber_margin"], "floor margins", ref["floor_margin"])
    assert ref["rank"] == case["rank"] == RC.HAND[name]
    assert case["n3"] + case["n1"] <= 1700 and ref["n_surface_no_plane"] == 0
    assert ref["huber_margin"] > RC.HUBER_MARGIN and min(ref["floor_margin"]) >= 0.5
    assert ref["cond"] <= RC.CAP and RC.C_COV * RC.MARGIN * RC.U * ref["cond"] <= 1e-5
    # the scale is one population's error, or every row is an inlier whatever the scale: never the noise within a population
    inliers = ref["n_edge_inliers"] + ref["n_surface_inliers"]
    assert ref["error_scale"] > 1e-3 or inliers == case["n3"] + case["n1"], ref["error_scale"]
    assert abs(ref["min_eigenvalue_d"] - 0.1) > RC.d_bound(ref)
    ratio = lam[0] / lam[5]
    if name in RC.WINDOW:
        lo, hi = RC.WINDOW[name]
        assert lo <= ratio <= hi, ratio
        assert abs(RC.solve_epsilon(name) - RC.EPSILON[name]) <= 1e-3 * RC.EPSILON[name], "the record of the tilt is stale"
    if name == "long_corridor":
        assert abs(ref["cond"] - RC.LONG_COND) <= 1e-2 * ref["cond"], "the record of cond_2 is stale"
        assert np.abs(case["surface"][:, 0]).max() >= 95.0
    if name.endswith("_rotated"):
        R = case["pose"][:, :3]
        assert R[0, 0] + R[1, 1] + R[2, 2] <= 0                    # Eigen::Quaterniond's other branch into M


def test_both_sides_of_the_floor():
    above, below = _ref("converging_above_floor"), _ref("converging_below_floor")
    floor = RR.FLOOR
    print("lambda_0 / lambda_5: %.3e (rank %d) and %.3e (rank %d)" % (above["eigenvalues"][0] / above["eigenvalues"][5], above["rank"],
                                                                   below["eigenvalues"][0] / below["eigenvalues"][5], below["rank"]))
    assert (above["rank"], below["rank"]) == (6, 5)
    # the covariance along the corridor: sigma2 / lambda_0 where it stands, sigma2 / floor where it is floored
    for ref, floored in ((above, False), (below, True)):
        lam, v = ref["eigenvalues"], ref["eigenvectors"][0]
        assert abs(v[3]) >= 0.999                                  # the translation along x
        along = ref["sigma2"] / (floor * lam[5] if floored else lam[0])
        assert abs(ref["covariance"][3, 3] - along) <= 1e-3 * along, (ref["covariance"][3, 3], along)


@pytest.mark.parametrize("name", ["box", "box_square"])
def test_the_boxes_have_a_diagonal_h_with_repeated_eigenvalues(name):
    rows, ref = RC.host_reference(name)
    case = [c for c in RC.hand_cases() if c["name"] == name][0]
    H = restate(case["pose"], *rows)["information"]
    off = np.abs(H - np.diag(np.diag(H))).max()
    lam = ref["eigenvalues"]
    equal = [k for k in range(5) if lam[k + 1] - lam[k] <= 1e-12 * lam[5]]
    print(name, "largest off-diagonal entry %.3g = %.3g ulp of the diagonal's largest" % (off, off / np.spacing(np.diag(H).max())), "eigenvalues", lam)
    assert off <= 64 * np.spacing(np.diag(H).max())
    assert len(equal) >= 2, lam                              # two pairs in either box (y and z faces alike; x and y faces alike)
    # mirror images: opposite faces carry equal counts and the same insets
    s = case["surface"][:, :3].astype(np.float64)
    for axis in range(3):
        m = s.copy()
        m[:, axis] = -m[:, axis]
        assert sorted(map(tuple, m)) == sorted(map(tuple, s))
    if name == "box_square":
        diag = np.diag(H)
        assert abs(diag[3] - diag[4]) <= 1e-12 * diag[3] and abs(diag[0] - diag[1]) <= 1e-12 * diag[0]     # lambda_x = lambda_y, lambda_rx = lambda_ry


def test_the_wall_at_45_degrees_ties_under_the_sign_rule():
    ref = _ref("wall_at_45")
    tied = []
    for k in range(6):
        a = np.sort(np.abs(ref["eigenvectors"][k]))[::-1]
        if a[0] - a[1] <= 1e-5 * a[0]:
            tied.append((k, a[0], a[1]))
    print("eigenvectors whose two largest components tie:", tied)
    assert tied
