"""The restatement with priors (tests/pose_graph_prior_restatement.py) held to the old one (tests/pose_graph_restatement.py),
on the host.

* Pose priors and position priors without a lever: the new dense step equals R.dense_step on the anchored graph (the
  identity node first, the ids shifted, every prior an edge from the anchor; a released first node: only the anchor is
  fixed).  The two are two dense solves of the same system; their difference must lie below the whole-chain floor
  K.floors()[0].
* The lever arm's Jacobian against central differences, allowed 4 x what the same check gives for R.edge_terms' A_j at the
  same poses.
* The floor: for every shape of tests/pose_graph_prior_cases.py the new woodbury_step and the new dense step differ by
  less than K.floors()[0]: a condition on the shapes, which is what lets the device be held to the old tolerance.
* The drift case's seed: the restatement converges, down-weights exactly the outlier fix and ends with a smaller worst
  position error than it began with.

Measured here (K.floors()[0] = 1.3e-10):
  anchored - prior form, dense: 1.4e-17 .. 1.5e-15 over the shapes (prior_on_an_isolated_node the largest)
  woodbury - dense with priors: one_prior 5.8e-16, 64_priors 5.0e-16, 65_priors 3.7e-16, three_mixed_on_one_node 1.2e-16,
    on_fixed_first_and_last 2.5e-16, prior_on_an_isolated_node 4.8e-15, four_nodes_no_edge 1.4e-17, robust_priors 2.4e-16,
    position_levers 1.5e-15, N65_gap_prior_every_8th 2.8e-15, released_pose_prior_on_0 2.4e-15,
    released_positions_only 1.2e-14, released_257_a_fix_per_node 1.3e-14
    (prior_on_an_isolated_node with a position prior in place of the pose prior on node 17: 1.9e-7, the class of the gap
    shapes; the shape was changed, as the condition asks)
  central differences, h = 1e-6: the position prior's A within 1.14e-9, R.edge_terms' A_j within 1.17e-9
  drift_256: converged after 8 iterations, w < 1 at prior 9 alone (0.0060), worst position error 1.501 -> 0.136 m
Every test prints its figures before it asserts."""
import numpy as np
import pytest

from tests import pose_graph_cases as K
from tests import pose_graph_prior_cases as PK
from tests import pose_graph_prior_restatement as Q
from tests import pose_graph_restatement as R


@pytest.mark.parametrize("g", PK.step_shapes(), ids=lambda g: g["name"])
def test_dense_step_equals_the_anchored_graphs(g):
    h = PK.without_levers(g)
    new, lin = Q.dense_step(h["poses"], h["edges"], h["priors"], h["fixed"], h["released"], **PK.config_of(h))
    poses, edges, fixed = PK.anchored(h)
    old, olin = R.dense_step(poses, edges, fixed, **PK.config_of(h))
    diff = float(np.abs(old[1:] - new).max())
    P = len(h["priors"])
    pose_kind = (h["priors"]["flags"] & Q.PRIOR_POSITION) == 0
    print("%s: anchored - prior form %.3e (floor %.2e, max |delta| %.2e); chi2 %.9e vs %.9e" % (
        g["name"], diff, K.floors()[0], np.abs(new).max(), lin["chi2"], olin["chi2"]))
    assert np.abs(old[0]).max() == 0.0 and (g["released"] or np.abs(new[0]).max() == 0.0)
    assert diff <= K.floors()[0]
    # a pose prior's r, rho and w ARE the anchored edge's; a position prior's share too, the edge's phi aside
    assert np.array_equal(lin["p_r"][pose_kind], olin["r"][-P:][pose_kind])
    assert np.array_equal(lin["p_rho"][pose_kind], olin["rho"][-P:][pose_kind]) and np.array_equal(lin["p_w"][pose_kind], olin["w"][-P:][pose_kind])
    assert np.allclose(lin["p_rho"], olin["rho"][-P:], rtol=1e-12, atol=0.0) and np.array_equal(lin["p_w"] < 1.0, olin["w"][-P:] < 1.0)


def _numeric_jacobian(residual, T, h=1e-6):
    """central differences of residual(T) along the increment R <- R Exp(a), t <- t + b"""
    J = np.zeros((6, 6))
    for c in range(6):
        d = np.zeros((1, 6))
        d[0, c] = h
        plus = np.asarray(residual(Q.retract(T[None], d, set())[0]))
        minus = np.asarray(residual(Q.retract(T[None], -d, set())[0]))
        J[:, c] = (plus - minus) / (2.0 * h)
    return J


def test_the_lever_arms_jacobian_against_central_differences():
    rng = np.random.default_rng(5)
    worst_new, worst_old = 0.0, 0.0
    for _ in range(8):
        T = K.pose(rng.standard_normal(3), 5.0 * rng.standard_normal(3))
        Ti = K.pose(rng.standard_normal(3), 5.0 * rng.standard_normal(3))
        Z = K.perturb(K.between(Ti, T), rng, 0.3, 0.5)
        tz = T[:, 3] + rng.standard_normal(3)
        lever = np.array(PK.LEVER) * (1.0 + rng.standard_normal(3))
        ar = R.Arith()
        _r, A = Q.position_terms(T, tz, lever, ar)
        new = float(np.abs(_numeric_jacobian(lambda X: Q.position_terms(X, tz, lever, ar)[0], T) - np.array(A)).max())
        om = np.eye(6)
        Aj = np.array(R.edge_terms(Ti, T, Z, om, 0, 3.0)[4])
        old = float(np.abs(_numeric_jacobian(lambda X: R.edge_terms(Ti, X, Z, om, 0, 3.0)[0], T) - Aj).max())
        worst_new, worst_old = max(worst_new, new), max(worst_old, old)
    print("central differences (h = 1e-6): the position prior's A within %.3e, R.edge_terms' A_j within %.3e (allowed: 4 x the latter)" % (worst_new, worst_old))
    assert worst_new <= 4.0 * worst_old


def test_every_shape_lies_below_the_whole_chain_floor():
    seen, f = PK.differences(), K.floors()[0]
    for name, v in seen.items():
        print("%-32s woodbury - dense with priors %.3e (floor %.2e)" % (name, v, f))
    assert all(v <= f for v in seen.values()), {k: v for k, v in seen.items() if v > f}


def test_the_shapes_cover_what_they_claim():
    """the counts and the weights the shapes were built for"""
    shapes = {g["name"]: g for g in PK.step_shapes()}
    assert [len(shapes[n]["priors"]) for n in ("one_prior", "64_priors", "65_priors", "released_257_a_fix_per_node")] == [1, 64, 65, 257]
    assert len(shapes["four_nodes_no_edge"]["edges"]) == 0 and len(shapes["four_nodes_no_edge"]["poses"]) == 4
    lin = PK.dense_first_steps()["robust_priors"][1]
    s = np.sqrt(np.einsum("pi,pi->p", lin["p_r"], lin["p_q"] / lin["p_w"][:, None]))
    print("robust_priors: s = %s, w = %s" % (np.array2string(s, precision=3), np.array2string(lin["p_w"], precision=4)))
    assert lin["p_w"][PK.ROBUST_INSIDE] == 1.0 and 0.1 < lin["p_w"][PK.ROBUST_BEYOND] < 1.0 and lin["p_w"][PK.ROBUST_FAR] < 0.01
    assert abs(s[PK.ROBUST_FAR] - 25.0 / 0.05) < 0.5 * 25.0 / 0.05
    for name in shapes:
        _, res, _, _ = PK.one_iteration(name)
        print("%-32s one iteration: code %d, chi2 %.4e -> %.4e, %d edges and %d priors down-weighted" % (
            name, res["code"], res["chi2_initial"], res["chi2_final"], res["n_robust_downweighted"], res["n_prior_downweighted"]))
        assert res["code"] in (R.CONVERGED, R.MAX_ITERATIONS)
    # the isolated node and the edgeless graph move by their priors alone
    assert np.abs(PK.dense_first_steps()["prior_on_an_isolated_node"][0][10]).max() > 0.0
    assert np.abs(PK.dense_first_steps()["four_nodes_no_edge"][0][1:]).min(axis=1).max() > 0.0
    lin = Q.linearize(**{k: PK.linearisation_case()[k] for k in ("poses", "edges", "priors")})
    theta = np.linalg.norm(lin["p_r"][:5, :3], axis=1)
    print("linearisation case: residual rotations %s; robust w %s" % (np.array2string(theta, precision=6), np.array2string(lin["p_w"][5:9], precision=4)))
    assert theta[0] < 1e-12 and np.allclose(theta[1:], [1e-5, 1e-3, 1.0, 2.5], rtol=1e-6)
    assert lin["p_w"][5] == 1.0 and lin["p_w"][6] < 0.5 and lin["p_w"][7] < 0.01 and lin["p_w"][8] == 1.0


def test_the_drift_cases_seed():
    g = PK.drift_case()
    poses, res, _edges, (rho, w) = PK.drift_result()
    before, after = K.worst_error(g["poses"], g["truth"]), K.worst_error(poses, g["truth"])
    print("drift_256: code %d after %d iterations, chi2 %.6e -> %.6e (priors %.6e); w < 1 at priors %s (smallest %.5f); worst position error %.3f -> %.3f m" % (
        res["code"], res["iterations"], res["chi2_initial"], res["chi2_final"], res["chi2_priors"], np.flatnonzero(w < 1.0).tolist(), w.min(), before, after))
    assert res["code"] == R.CONVERGED
    assert np.flatnonzero(w < 1.0).tolist() == [PK.DRIFT_OUTLIER] and res["n_prior_downweighted"] == 1 and res["n_robust_downweighted"] == 0
    assert after < before
