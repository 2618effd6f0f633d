"""The covariances' algebra on the host, before a GPU sees it (tests/pose_graph_marginal_restatement.py; the graphs and the
tolerance's constants: tests/pose_graph_marginal_cases.py).

The float64 restatement of the device's algorithm against the 50-digit reference of the definition, every case; the 50-digit
evaluation of the algorithm against mpmath's dense inverse wherever both exist (that is what makes it a reference beyond);
relative_covariance, restated and the library's host routine, against central differences of the edge residual; and the
conditions the cases claim.  Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

from lidar_feature_extraction_amd import binding as B
from tests import pose_graph_cases as K
from tests import pose_graph_marginal_cases as MC
from tests import pose_graph_marginal_restatement as M
from tests import pose_graph_restatement as R

NAMES = [c["name"] for c in MC.cases()]


@pytest.mark.parametrize("name", NAMES)
def test_algorithm_restatement_against_the_reference(name):
    c = MC.case(name)
    ref = MC.start_reference(name)
    diag, cross = M.algorithm(MC.system_of(c), c["pairs"])
    ratio = MC.worst(diag, cross, ref)
    print("%s: kappa_2 %.3e, max |Sigma| %.3e, error %.3g eps kappa max|Sigma| (C of its class %.3g)" % (name, ref[2], ref[3], ratio, MC.c_of(name)))
    assert ratio <= MC.c_of(name)
    # the definition in float64 agrees as far as the condition allows (a wrong block would be off by its own size)
    d64, x64 = M.blocks(M.definition(MC.system_of(c)), len(c["poses"]), c["pairs"])
    assert MC.worst(d64, x64, ref) <= 16.0


@pytest.mark.parametrize("name", [c["name"] for c in MC.cases() if len(c["poses"]) <= MC.DENSE_REFERENCE_NODES])
def test_the_algorithm_at_50_digits_is_the_dense_inverse(name):
    c = MC.case(name)
    diag, cross, kappa, top = MC.start_reference(name)               # (mpmath's dense inverse for these)
    d50, x50 = M.algorithm(MC.system_of(c), c["pairs"], digits=M.DIGITS)
    err = max([np.abs(d50 - diag).max()] + [np.abs(x50[p] - cross[p]).max() for p in cross])
    tol = MC.bound(name, (diag, cross, kappa, top))
    print("%s: the algorithm at 50 digits - the dense inverse at 50 digits: %.3e of max |Sigma| %.3e, %.2g of the device's bound" % (
        name, err, top, err / tol))
    # Not equal to the last bit: the split adds lambda to a diagonal block before the edges' terms, the dense assembly after
    # them, so the two invert matrices one rounding of an addition apart -- as the device's own assembly is from either.
    # What matters is that this is small against the bound the reference is used for.
    assert err <= 0.05 * tol


def test_the_chain_solve_form_of_a_cross_block_agrees():
    c = MC.case("N65_L9")
    ref = MC.start_reference("N65_L9")
    diag, cross = M.algorithm(MC.system_of(c), c["pairs"], chain_solve=True)
    ratio = MC.worst(diag, cross, ref)
    print("P^-1 E_j in place of the product of the T_k: %.3g eps kappa max|Sigma|" % ratio)
    assert ratio <= MC.C_WHOLE


def test_conditions_the_cases_claim():
    seen = {}
    for c in MC.cases():
        s = MC.system_of(c)
        kappa = M.condition(s)
        seen[c["name"]] = kappa
        print("%-36s N %3d loops %2d fixed %s kappa_2 %.3e" % (c["name"], s["N"], len(R.split_edges(c["edges"], s["N"])[1]), sorted(s["fixed"]), kappa))
        assert kappa <= MC.CAP
        assert abs(kappa - MC.KAPPA[c["name"]]) <= 1e-2 * kappa, "the record of kappa_2 in pose_graph_marginal_cases.py is stale"
        assert MC.c_of(c["name"]) * MC.MARGIN * MC.EPS * kappa <= 1e-5
    loops = {n: len(R.split_edges(MC.case(n)["edges"], len(MC.case(n)["poses"]))[1]) for n in NAMES}
    # 6 L against the panel: none, one entry row, one panel exactly full, one over, two panels and a bit
    assert [6 * loops["N12_L%d" % L] for L in (0, 1, 8, 9, 17)] == [0, 6, MC.PANEL, MC.PANEL + 6, 2 * MC.PANEL + 6]
    assert loops["N64_L9"] == loops["N65_L9"] == 9 and loops["N257_L9_released"] == 9
    assert (6 * 64) % 64 == 0 and (6 * 65) % 64 != 0                  # the row tiles: exactly full, and a partial last one
    assert MC.system_of(MC.case("fixed_middle_and_end"))["fixed"] == {0, 12, 23}
    assert MC.system_of(MC.case("N257_L9_released"))["fixed"] == set()
    assert MC.system_of(MC.case("released_position_priors_lever"))["fixed"] == set()
    gap = MC.case("N65_chain_31_32_missing_bridged")
    assert R.split_edges(gap["edges"], 65)[0][31] < 0
    # the false loop is down-weighted, the others are not
    rob = MC.system_of(MC.case("robust_false_loop"))
    w = rob["lin"]["w"]
    assert (w < 0.1).sum() == 1 and (w[w >= 0.1] == 1.0).all()
    # the isolated node: Sigma = I / lambda, and nothing couples it
    iso = MC.case("isolated_last_node")
    diag, cross, _, _ = MC.start_reference("isolated_last_node")
    assert np.abs(diag[19] * iso["damping"] - np.eye(6)).max() <= 1e-12 and not cross[(19, 3)].any() and not cross[(18, 19)].any()
    # fixed nodes: zeros
    diag, cross, _, _ = MC.start_reference("fixed_middle_and_end")
    assert not diag[0].any() and not diag[12].any() and not diag[23].any() and not cross[(12, 13)].any() and cross[(11, 13)].any()
    # the distances the joint kernel's product is walked at
    d = sorted({abs(i - j) for i, j in MC.case("N257_L9_released")["pairs"]})
    assert {1, 2, 63, 64, 256} <= set(d)


def _numeric_jacobians(Ti, Tj, Z, h=1e-6):
    """dr / d delta_i, dr / d delta_j of the edge residual by central differences, delta = (a, b): R <- R Exp(a), t <- t + b"""
    def moved(T, d):
        out = np.array(T, np.float64)
        out[:, :3] = T[:, :3] @ R.exp_rotation(d[:3])
        out[:, 3] = T[:, 3] + d[3:]
        return out
    J = np.zeros((6, 12))
    for k in range(12):
        d = np.zeros(12)
        d[k] = h
        plus = M.edge_residual(moved(Ti, d[:6]), moved(Tj, d[6:]), Z)
        minus = M.edge_residual(moved(Ti, -d[:6]), moved(Tj, -d[6:]), Z)
        J[:, k] = (plus - minus) / (2.0 * h)
    return J


def test_relative_covariance_against_central_differences():
    L = B.load()
    c = MC.case("N12_L9")
    diag, cross, _, _ = MC.start_reference("N12_L9")
    for (i, j) in ((3, 9), (9, 3), (1, 2)):
        Ti, Tj = c["poses"][i], c["poses"][j]
        Z = K.between(Ti, Tj)
        joint = M.joint(diag, cross, i, j)
        J = _numeric_jacobians(Ti, Tj, Z)
        want = J @ joint @ J.T
        mine = M.relative_covariance(Ti, Tj, joint)
        lib = np.zeros(36)
        args = [np.ascontiguousarray(x, np.float64).reshape(-1) for x in (Ti, Tj, joint)]
        assert L.lfx_pose_graph_relative_covariance(*[C.c_void_p(a.ctypes.data) for a in args], C.c_void_p(lib.ctypes.data)) == 0
        lib = lib.reshape(6, 6)
        top = np.abs(want).max()
        print("(%d, %d): restated - differences %.3e, library - restated %.3e of %.3e" % (i, j, np.abs(mine - want).max(), np.abs(lib - mine).max(), top))
        # central differences with h = 1e-6: a relative error of h^2 in the Jacobians, and eps / h from the residual's rounding
        assert np.abs(mine - want).max() <= 1e-8 * top
        assert np.abs(lib - mine).max() <= 64 * np.spacing(top)
        assert lib.tobytes() == lib.T.copy().tobytes()
    assert L.lfx_pose_graph_relative_covariance(None, None, None, None) == B.ERR_INVALID_ARGUMENT


def test_relative_covariance_of_two_nodes_is_the_edge_information_inverted():
    """N = 2, node 0 fixed, lambda = 0: H is A_j^T Omega A_j, and the residual's covariance is Omega^-1 (exact algebra)"""
    c = MC.case("N2_L0")
    # at the optimum of a single edge the residual is 0, which is where relative_covariance takes its Jacobians
    poses = np.array([c["poses"][0], K.compose(c["poses"][0], np.reshape(c["edges"][0]["z"], (3, 4)))])
    s = M.system(poses, c["edges"], damping=0.0)
    diag, cross = M.blocks(M.definition(s), 2, [(0, 1)])
    rel = M.relative_covariance(poses[0], poses[1], M.joint(diag, cross, 0, 1))
    omega = np.reshape(c["edges"][0]["information"], (6, 6))
    omega_inv = np.linalg.inv(omega)
    err, top = np.abs(rel - omega_inv).max(), np.abs(omega_inv).max()
    print("relative covariance - Omega^-1: %.3e of %.3e, kappa_2(Omega) %.3e" % (err, top, np.linalg.cond(omega)))
    assert err <= 64.0 * MC.EPS * np.linalg.cond(omega) * top
