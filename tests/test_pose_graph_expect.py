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
import os

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


def _tolerance(name, want):
    """what the device's one-step test allows a shape: 16 x the floor of its class, or 1e-12 of the step"""
    return max(16.0 * K.floor_of(name), 1e-12 * float(np.abs(want).max()))


def test_the_extra_shapes_lie_below_the_floor_they_are_held_to():
    """Each extra shape's own woodbury - dense difference, under its own config, is no larger than the floor of the class it
    is held to on the device (all of them the whole-chain class: K.floor_of knows no other name of theirs), so the
    restatement alone cannot eat the margin.  The last node of dangling_last_node has no edge: P's last block is lambda I,
    well conditioned, and the shape is in the whole-chain class BECAUSE its difference says so (the missing edge 31 -> 32
    of the gap class splits a chain that loops then hold together through lambda alone).
    Measured here: 5.1e-15, 3.6e-15 and 1.8e-14 at the robust shapes, 3.4e-14, 1.1e-13 and 5.9e-14 at damping 0, 1e-2
    and 10, 2.2e-15 at the dangling node; the floors are 1.3e-10 and 1.7e-7 as before."""
    whole, gap = K.floors()
    print("floors: whole chains %.2e; the missing chain edge %.2e" % (whole, gap))
    assert whole < 1e-9 and gap < 1e-5                                # (as test_the_solvers_statement_against_the_dense_step holds them)
    assert not set(K.extra_differences()) & set(g["name"] for g in K.step_shapes() + K.circles())
    for g in K.extra_step_shapes():
        diff, want = K.extra_differences()[g["name"]], K.extra_first_steps()[g["name"]][0]
        _, res, _ = K.one_iteration(g["name"])
        print("%-28s woodbury - dense %.2e, max |delta| %.5f, damping %g, huber_delta %g; one iteration: code %d, %d down-weighted" % (
            g["name"], diff, np.abs(want).max(), g["damping"], g["huber_delta"], res["code"], res["n_robust_downweighted"]))
        assert K.floor_of(g["name"]) == whole and diff <= whole
        assert res["code"] == R.MAX_ITERATIONS                       # (not DIVERGED: the device's step would be taken back)
    g = K.all_step_shapes()["dangling_last_node"]
    want = K.extra_first_steps()["dangling_last_node"][0]
    chain, loops = R.split_edges(g["edges"], 20)
    assert chain[18] < 0 and not any(19 in (int(g["edges"][e]["i"]), int(g["edges"][e]["j"])) for e in range(len(g["edges"])))
    assert not np.any(want[19]) and np.abs(want[18]).max() > 1e-3
    assert K.one_iteration("dangling_last_node")[0][19].tobytes() == g["poses"][19].tobytes()


def test_the_robust_shapes_have_the_weights_they_are_there_for():
    """robust_chain_pair: the adjacent chain edges 7 and 8 and loop edge 23 start with w < 0.1, the robust chain edge 12 with
    w == 1; beside the fixed node 9 the down-weighted edge 8 ends at it; under huber_delta = 0.5 edge 16 has 0.5 < s <= 3,
    so the two thresholds give different weights.  No robust edge's s lies within 1e-9 (relative) of its huber_delta, at
    the start or where a count is taken, so that rounding cannot flip a reported n_robust_downweighted."""
    for g in K.extra_step_shapes()[:3]:
        lin = K.extra_first_steps()[g["name"]][1]
        chain, loops = R.split_edges(g["edges"], 24)
        robust = np.flatnonzero(g["edges"]["flags"] & R.ROBUST)
        print("%-26s huber_delta %g: w of the robust edges %s = %s" % (g["name"], g["huber_delta"], robust.tolist(), np.round(lin["w"][robust], 5).tolist()))
        assert robust.tolist() == sorted(K.ROBUST_OUTLIERS + (K.ROBUST_INLIER, K.ROBUST_BETWEEN))
        assert all(chain[e] == e for e in (7, 8, 12, 16)) and 23 in loops
        assert (lin["w"][list(K.ROBUST_OUTLIERS)] < 0.1).all() and lin["w"][K.ROBUST_INLIER] == 1.0
        assert (lin["w"][g["edges"]["flags"] == 0] == 1.0).all()
    pair, beside, half = K.extra_step_shapes()[:3]
    assert beside["fixed"] == (9,) and int(beside["edges"][8]["j"]) == 9 and beside["edges"].tobytes() == pair["edges"].tobytes()
    s = K.robust_s(half["edges"], *(K.extra_first_steps()["huber_half"][1][k] for k in ("rho", "w")), 0.5)
    w3, w05 = (K.extra_first_steps()[n][1]["w"] for n in ("robust_chain_pair", "huber_half"))
    print("huber_half: s of the robust edges %s; w at 3.0 %s, at 0.5 %s" % (np.round(s, 4).tolist(), np.round(w3[w3 < 1], 5).tolist(), np.round(w05[w05 < 1], 5).tolist()))
    assert half["edges"].tobytes() == pair["edges"].tobytes() and ((s > 0.5) & (s <= 3.0)).any()
    assert w3[K.ROBUST_BETWEEN] == 1.0 and 0.3 < w05[K.ROBUST_BETWEEN] < 0.4 and (w05[list(K.ROBUST_OUTLIERS)] < w3[list(K.ROBUST_OUTLIERS)] / 5.9).all()
    # the step the weights lead to differs by far more than the tolerance
    d3, d05 = (K.extra_first_steps()[n][0] for n in ("robust_chain_pair", "huber_half"))
    assert np.abs(d3 - d05).max() > 1e3 * _tolerance("huber_half", d05)
    # the counts: no s near its threshold
    seen = []
    for g in K.extra_step_shapes():
        lin = K.extra_first_steps()[g["name"]][1]
        _, res, (rho, w) = K.one_iteration(g["name"])
        assert res["n_robust_downweighted"] == int((w < 1.0).sum())
        seen += [(g["name"], g["huber_delta"], K.robust_s(g["edges"], lin["rho"], lin["w"], g["huber_delta"])),
                 (g["name"] + " after one iteration", g["huber_delta"], K.robust_s(g["edges"], rho, w, g["huber_delta"]))]
    for name, g in zip(("robust", "plain", "clean"), K.false_loop_cases()):
        _, res, (rho, w) = K.false_loop_runs()[name]
        seen.append(("false loop, " + name, 3.0, K.robust_s(g["edges"], rho, w, 3.0)))
        print("false loop, %s: %d down-weighted" % (name, res["n_robust_downweighted"]))
    for name, delta, s in seen:
        if len(s):
            near = float(np.abs(s / delta - 1.0).min())
            print("%-44s closest robust s to huber_delta: %.3e relative" % (name, near))
            assert near > 1e-9
    assert K.one_iteration("robust_chain_pair")[1]["n_robust_downweighted"] == 3 and K.one_iteration("huber_half")[1]["n_robust_downweighted"] == 4
    assert K.false_loop_runs()["robust"][1]["n_robust_downweighted"] >= 1


def test_the_dampings_move_the_dense_step():
    """The dense step of the damping graph at lambda = 1e-6 against the step at each damping of the device's cases: where the
    two differ by more than the tolerance, a device that ignored its config's damping would fail the case.  Measured:
    max |delta| 1.32334 at 0 and at 1e-6, 1.32327 at 1e-2, 1.26220 at 10; the steps differ from the one at 1e-6 by 1.4e-8
    (damping 0), 1.4e-4 (1e-2) and 1.1e-1 (10) against a tolerance of 2.1e-9.  damping_0 is 6.6 tolerances from 1e-6: too
    close to rest a mutation on, so it is kept as a case that runs and matches (lambda = 0: P is held by the edges alone)
    and only 1e-2 and 10, asserted to lie more than 1000 tolerances away, carry the mutation."""
    g = K.damping_graph()
    usual = R.dense_step(g["poses"], g["edges"], g["fixed"])[0]
    for name, damping in K.DAMPINGS:
        want = K.extra_first_steps()[name][0]
        apart, tol = float(np.abs(want - usual).max()), _tolerance(name, want)
        print("%-14s max |delta| %.5f; apart from the step at 1e-6 by %.3e; tolerance %.3e" % (name, np.abs(want).max(), apart, tol))
        if damping > 0.0:
            assert apart > 1e3 * tol


def test_the_growth_stages_on_the_restatement():
    """The growth test's stages run on the restatement (tests/test_pose_graph_gpu.py grows the device's graph the same way):
    the split of every stage is the one the header's rule gives, the robust second edge on (40, 41) IS the chain edge and
    is down-weighted, and every stage's first step lies below the whole-chain floor, which the device's is held to."""
    poses, _ = K.growth_graph()
    whole = K.floors()[0]
    cur, edges = np.zeros((0, 3, 4)), np.zeros(0, K.EDGE)
    for stage, (n, calls, fixed) in enumerate(K.growth_stages(), 1):
        cur = np.concatenate([cur, poses[len(cur):n]])
        edges = np.concatenate([edges] + calls)
        chain, loops = R.split_edges(edges, n)
        dense, lin = R.dense_step(cur, edges, fixed)
        diff = float(np.abs(R.woodbury_step(cur, edges, fixed, lin=lin) - dense).max())
        before = cur
        cur, res, (rho, w) = R.optimize(cur, edges, fixed)
        print("stage %d: %d nodes, %d chain and %d loop edges, fixed %s; woodbury - dense %.2e, max |delta| %.4f; code %d after %d iterations, %d down-weighted" % (
            stage, n, (chain >= 0).sum(), len(loops), fixed, diff, np.abs(dense).max(), res["code"], res["iterations"], res["n_robust_downweighted"]))
        assert diff <= whole and res["code"] == R.CONVERGED
        if stage == 3:
            assert chain[40] == 34 and int(edges[34]["flags"]) == R.ROBUST and chain[46] < 0 and lin["w"][34] < 0.1
            assert [int(edges[e]["i"]) for e in loops[-2:]] == [35, 40] and (chain >= 0).sum() == 46 and len(loops) == 5
            assert cur[20].tobytes() == before[20].tobytes() and cur[47].tobytes() == before[47].tobytes()
        if stage == 4:
            assert (chain >= 0).sum() == 47 and chain[46] == 51 and np.abs(cur[20] - before[20]).max() > 1e-6
        near = np.abs(K.robust_s(edges, rho, w, 3.0) / 3.0 - 1.0)
        assert not len(near) or near.min() > 1e-9


REFERENCE_UNITS = {"to 2.5 rad": 0.78, "beyond": 3.0}            # measured (below), in spacings of the largest term


def test_the_residual_against_the_50_digit_reference():
    """r = (Log(R_E), t_E) of the restatement (products rounded, as the device's) against tools/pose_graph_reference.py: mpmath at 50 digits,
    Log through the nearest rotation's quaternion, not the header's formula.  The error is counted in spacings of the
    largest term summed on the way to r (Arith.mark("r"): 2.6 .. 7.3 here, metres).  Measured, rotation / translation part:
      0 rad 0.06 / 0.56    1e-12 0.04 / 0.78    1e-7 0.03 / 0.38    9.9e-5 0.05 / 0.45    1.01e-4 0.07 / 0.25
      1e-2  0.04 / 0.12    1.0   0.25 / 0.50    2.5  0.50 / 0.31    2.9    3.00 / 0.25    2.99    1.75 / 0.62
    Up to 2.5 rad nothing exceeds 0.78; at 2.9 and 2.99 rad the rotation part is 3 to 6 times its error at 2.5 rad, which is
    the 1 / sin theta (4.2 and 6.6) by which v / |v| loses its direction near pi: in line with the formula's conditioning,
    no defect, and now said beside the header's "Valid for theta < 3 rad".  Asserted: 16 x the measured worst of each range."""
    cases = K.residual_reference()
    assert [c[0] for c in cases] == ["0", "1e-12", "1e-7", "9.9e-5", "1.01e-4", "1e-2", "1.0", "2.5", "2.9", "2.99"]
    try:
        import mpmath  # noqa: F401
    except ImportError:
        print("mpmath is not here: the file is taken as it is")
    else:
        import importlib.util
        spec = importlib.util.spec_from_file_location("pose_graph_reference", os.path.join(os.path.dirname(K.REFERENCE_PATH), "..", "..", "tools", "pose_graph_reference.py"))
        tool = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tool)
        with open(K.REFERENCE_PATH) as f:
            assert f.read() == tool.text(), "tests/golden/pose_graph_residual_reference.json is not what tools/pose_graph_reference.py writes"
    failed = []
    for angle, Ti, Tj, Z, want in cases:
        ar = R.Arith()
        got = np.array(R.edge_terms(Ti, Tj, Z, np.eye(6), 0, 3.0, ar)[0])
        unit = np.spacing(ar.seen["r"])
        rot, trans = np.abs(got - want)[:3].max() / unit, np.abs(got - want)[3:].max() / unit
        allowed = 16.0 * REFERENCE_UNITS["to 2.5 rad" if float(angle) <= 2.5 else "beyond"]
        print("residual angle %-8s (%.17g): rotation part %.2f, translation part %.2f spacings of the largest term %.3f; allowed %.1f" % (
            angle, np.linalg.norm(want[:3]), rot, trans, ar.seen["r"], allowed))
        assert abs(np.linalg.norm(want[:3]) - float(angle)) <= 1e-15 + 4e-16 * float(angle) and 0.1 < np.linalg.norm(want[3:]) < 3.0
        if not max(rot, trans) <= allowed:
            failed.append(angle)
    assert not failed, failed


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
