"""The pose-graph problem on the host (include/lfx.h, the pose graph section): the restatement's Jacobians against central
differences, hand cases, the host helper lfx_pose_graph_edge_information, the measured floor between the solver's statement
and the dense step, and the conditions the seeds of the device's convergence and robust cases were chosen by.  No device: but for the
edge_information case these tests hold the restatement, which the device is then held to in tests/test_pose_graph_gpu.py.

Measured here (python, float64): the floor f over the shapes with a whole chain is 1.3e-10 (circle_256_40; 1e-17 .. 1.6e-13
at the one-step shapes, 8e-12 at 257 nodes and at circle_256_5); the shape whose chain edge 31 -> 32 is missing has 1.7e-7:
there P is held by lambda = 1e-6 alone along six directions, so P^-1 carries 1e6 and the two ways to the step part at
1e6 x 1e-16 x the step's size x the loops' weight.  The device is therefore held to 16 f of the shape's class
(tests/pose_graph_cases.py floors()), both no larger than the one figure over all shapes."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import pose_graph_cases as K
from tests import pose_graph_restatement as R


def _numeric_jacobians(Ti, Tj, Z, h=1e-6):
    def res(a, b):
        return np.array(R.edge_terms(a, b, Z, np.eye(6), 0, 3.0)[0])
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    for c in range(6):
        d = np.zeros(6)
        d[c] = h
        step = lambda T, s: R.retract(np.array([np.zeros((3, 4)), T]), np.array([np.zeros(6), s * d]))[1]      # noqa: E731  (node 1 moves)
        Ji[:, c] = (res(step(Ti, 1), Tj) - res(step(Ti, -1), Tj)) / (2 * h)
        Jj[:, c] = (res(Ti, step(Tj, 1)) - res(Ti, step(Tj, -1))) / (2 * h)
    return Ji, Jj


@pytest.mark.parametrize("angle", [0.0, 1e-5, 1e-3, 1.0, 2.5])
def test_jacobians_agree_with_central_differences(angle):
    """Random poses whose residual rotation is `angle`: A_i and A_j against central differences with h = 1e-6, 1e-8 or
    better (measured: 1.0e-9 .. 2.1e-9 over these poses, whose translations are metres apart)."""
    rng = np.random.default_rng(int(angle * 1e6) + 5)
    worst = 0.0
    for _ in range(4):
        Ti = K.pose(rng.standard_normal(3), 5 * rng.standard_normal(3))
        Tj = K.pose(rng.standard_normal(3), 5 * rng.standard_normal(3))
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        # Z with R_E = R_Z^T R_i^T R_j = Exp(angle axis) and a residual translation of a few metres
        Z = K.between(Ti, Tj)
        Z[:, :3] = Z[:, :3] @ R.exp_rotation(angle * axis).T
        Z[:, 3] += rng.standard_normal(3)
        r, _w, _rho, Ai, Aj, _q = R.edge_terms(Ti, Tj, Z, np.eye(6), 0, 3.0)
        assert abs(np.linalg.norm(r[:3]) - angle) < 1e-9
        Ni, Nj = _numeric_jacobians(Ti, Tj, Z)
        worst = max(worst, np.abs(np.array(Ai) - Ni).max(), np.abs(np.array(Aj) - Nj).max())
    print("angle %g: Jacobians within %.2e of central differences" % (angle, worst))
    assert worst <= 1e-8


def test_two_nodes_and_one_edge():
    """After one iteration node 1 is T0 Z to 1e-12 and chi^2 is 0.  (damping 0: lambda = 1e-6 against an information of
    1e4 holds the step back by 1e-10 of its length, 3e-11 m here.)"""
    rng = np.random.default_rng(3)
    T0 = K.pose(rng.standard_normal(3), rng.standard_normal(3))
    Z = K.pose([0.1, -0.2, 0.3], [1.0, 2.0, -0.5])
    start = np.array([T0, K.perturb(K.compose(T0, Z), rng, 0.01, 0.05)])
    edges = K.edges_of([(0, 1, Z, K.information(rng, 0.002, 0.01), 0)])
    # (one edge, its Jacobian A_j square and invertible: delta = -A_j^-1 r is exact, the rotation too, since J_r(phi) phi = phi)
    poses, res, _ = R.optimize(start, edges, max_iter=1, damping=0.0)
    assert np.abs(poses[1] - K.compose(T0, Z)).max() < 1e-12 and res["chi2_final"] < 1e-18 and res["iterations"] == 1
    exact = np.array([T0, K.compose(T0, Z)])
    exact[1, :, 3] += [0.3, -0.2, 0.1]             # a translation alone IS linear: one step
    poses, res, _ = R.optimize(exact, edges, max_iter=1, damping=0.0)
    assert np.abs(poses[1] - K.compose(T0, Z)).max() < 1e-12 and res["chi2_final"] < 1e-18 and res["iterations"] == 1
    assert np.array_equal(poses[0], T0)


def square_loop():
    side = K.pose([0.0, 0.0, math.pi / 2], [2.0, 0.0, 0.0])
    poses = [K.pose([0.0, 0.0, 0.3], [1.0, 1.0, 0.0])]
    for _ in range(3):
        poses.append(K.compose(poses[-1], side))
    om = np.diag([100.0] * 3 + [25.0] * 3)
    return np.array(poses), K.edges_of([(k, (k + 1) % 4, side, om, 0) for k in range(4)])


def test_a_consistent_square_loop_stays():
    poses, edges = square_loop()
    got, res, (rho, w) = R.optimize(poses, edges)
    assert res["chi2_initial"] < 1e-24 and res["chi2_final"] < 1e-24 and np.abs(got - poses).max() < 1e-12
    assert res["n_chain"] == 3 and res["n_loop"] == 1 and np.all(w == 1.0) and rho.max() < 1e-24


def test_edge_information_on_a_quarter_turn():
    """R = Rz(90 deg): R^T maps world x to -y' ... written out: with H's translation block [[4, .5, 0], [.5, 5, 0], [0, 0, 6]]
    the block becomes [[5, -.5, 0], [-.5, 4, 0], [0, 0, 6]]; the rotation block stays; the cross block's columns follow."""
    from lidar_feature_extraction_amd import edge_information
    H = np.diag([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    H[3, 4] = H[4, 3] = 0.5
    H[0, 3] = H[3, 0] = 0.25                      # rotation x with translation x
    T = np.array([[0.0, -1.0, 0.0, 7.0], [1.0, 0.0, 0.0, 8.0], [0.0, 0.0, 1.0, 9.0]])
    want = np.diag([1.0, 2.0, 3.0, 5.0, 4.0, 6.0])
    want[3, 4] = want[4, 3] = -0.5
    want[0, 4] = want[4, 0] = -0.25               # world x is the scan's -y
    got = edge_information(T, H)
    assert np.array_equal(got, want) and np.array_equal(R.edge_information(T, H), want)
    rng = np.random.default_rng(4)
    T = K.pose(rng.standard_normal(3), rng.standard_normal(3))
    m = rng.standard_normal((6, 6))
    H = m @ m.T
    assert np.abs(edge_information(T, H) - R.edge_information(T, H)).max() < 1e-14 * np.abs(H).max() * 8
    # in place, and refusals
    from lidar_feature_extraction_amd import binding as B
    buf = np.ascontiguousarray(H).reshape(36).copy()
    p = np.ascontiguousarray(T).reshape(12)
    assert B.load().lfx_pose_graph_edge_information(C.c_void_p(p.ctypes.data), C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data)) == 0
    assert np.array_equal(buf.reshape(6, 6), edge_information(T, H))
    assert B.load().lfx_pose_graph_edge_information(None, C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data)) == -1


def test_hubers_weight_at_the_threshold():
    """s = delta exactly and one float either side: w = 1 at and below, delta / s above; rho is continuous there."""
    delta = 3.0
    Ti = K.pose([0, 0, 0], [0, 0, 0])
    Z = K.pose([0, 0, 0], [0, 0, 0])
    for s, above in ((delta, False), (np.nextafter(delta, 0.0), False), (np.nextafter(delta, 10.0), True)):
        Tj = K.pose([0, 0, 0], [float(s), 0, 0])            # r = (0, 0, 0, s, 0, 0) and Omega = I: sqrt(r^T Omega r) = s
        r, w, rho, *_ = R.edge_terms(Ti, Tj, Z, np.eye(6), R.ROBUST, delta)
        assert r[3] == s and math.sqrt(s * s) == s
        assert (w < 1.0) == above and (w == 1.0 or w == delta / s)
        assert abs(rho - s * s) <= 4 * np.spacing(9.0)
        assert R.edge_terms(Ti, Tj, Z, np.eye(6), 0, delta)[1:3] == (1.0, s * s)


def test_the_solvers_statement_against_the_dense_step():
    f, seen = K.floor()
    for name, v in seen.items():
        print("%-36s woodbury - dense %.2e, max |delta| %.2e" % (name, v, np.abs(K.dense_first_steps()[name][0]).max()))
    whole, gap = K.floors()
    print("floor over all shapes %.2e; whole chains %.2e; the missing chain edge %.2e" % (f, whole, gap))
    assert whole < 1e-9 and gap < 1e-5 and f == max(whole, gap)
    # the split is the one the statement names
    g = [s for s in K.step_shapes() if s["name"] == "two_edges_on_one_pair"][0]
    chain, loops = R.split_edges(g["edges"], 16)
    assert (chain >= 0).sum() == 15 and len(loops) == 4 and chain[3] == 3 and loops[0] == 15


def test_the_circles_meet_the_conditions_their_seed_was_chosen_by():
    for g in K.circles():
        poses, res, _ = R.optimize(g["poses"], g["edges"])
        before, after = K.worst_error(g["poses"], g["truth"]), K.worst_error(poses, g["truth"])
        print(g["name"], res["iterations"], "iterations, worst position error %.3f -> %.3f m" % (before, after), res["steps"])
        assert res["code"] == R.CONVERGED and res["iterations"] <= 8 and res["max_step"] < 1e-9
        assert after <= 0.5 * before
        assert np.abs(np.einsum("kij,kil->kjl", poses[:, :, :3], poses[:, :, :3]) - np.eye(3)).max() <= 1e-12


def test_a_false_loop_with_and_without_the_robust_flag():
    robust, plain, clean = K.false_loop_cases()
    errs = {}
    for name, g in (("robust", robust), ("plain", plain), ("clean", clean)):
        poses, res, (rho, w) = R.optimize(g["poses"], g["edges"], max_iter=20, huber_delta=3.0)
        errs[name] = K.worst_error(poses, g["truth"])
        print(name, res["code"], res["iterations"], "worst %.3f m" % errs[name], "smallest w %.4f at edge %d" % (w.min(), int(w.argmin())))
        if name == "robust":
            assert int(w.argmin()) == 255 + 2 and res["n_robust_downweighted"] >= 1
    assert errs["robust"] <= 2.0 * errs["clean"] < errs["plain"]
