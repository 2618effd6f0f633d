"""lfx_pose_graph_* on the device against the restatement (tests/pose_graph_restatement.py; the graphs: tests/pose_graph_cases.py).

Linearisation: r, rho, w per edge, chi^2 and the nodes' gradient are held to the restatement within 16 x the difference
between the restatement evaluated with fused and with unfused products, with a floor of 4 ulp of the largest term that
went into the quantity (Arith.largest: r, rho and g each have their own).  The bracket is taken over the whole array: one
entry's own difference can be 0 by chance.
One step and convergence: 16 x and 64 x the measured floor of the shape's class (tests/test_pose_graph_expect.py).  The
extra shapes (down-weighted chain edges, huber_delta = 0.5, damping 0 .. 10, a node without an edge) and the stages of the
graph that grows run under their own config and are held to the same floor; a result's code and n_robust_downweighted are
the restatement's.  Growth, sub-range reads and the byte-for-byte rule: test_a_graph_that_grows.  Across streams and
objects: tests/test_pose_graph_streams_gpu.py.
Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest

from tests import deskew_cases as D
from tests import pose_graph_cases as K
from tests import pose_graph_restatement as R
from tests import segment_cases as S

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def fx():
    f = D.fx_for(16, 900, 1, test_hooks=True)       # (the test-hooks build: lfx_test_pose_graph_linearize)
    yield f
    f.close()


def build(fx, g, edge_calls=1, **config):
    """The graph g on the device: nodes, fixed flags, edges in `edge_calls` calls."""
    n, e = len(g["poses"]), g["edges"]
    pg = fx.pose_graph(n, max(len(e), 1), **config)
    assert pg.add_nodes(g["poses"], D.stream()) == 0
    for k in g["fixed"]:
        pg.set_fixed(k, True, D.stream())
    cuts = [len(e) * c // edge_calls for c in range(edge_calls + 1)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        pg.add_edges(e[a:b], D.stream())
    return pg


def linearize_on_device(fx, pg):
    info = pg.info()
    r, g, chi2 = np.zeros((info["n_edges"], 6)), np.zeros((info["n_nodes"], 6)), C.c_double(0.0)
    fn = fx._L.lfx_test_pose_graph_linearize
    fn.argtypes = [C.c_void_p] * 4 + [C.POINTER(C.c_double), C.c_void_p]
    rc = fn(fx._ctx, pg.handle, C.c_void_p(r.ctypes.data), C.c_void_p(g.ctypes.data), C.byref(chi2), C.c_void_p(D.stream()))
    assert rc == 0, fx._L.lfx_last_error(fx._ctx)
    rho, w = pg.edge_chi2(stream=D.stream())
    return dict(r=r, g=g, chi2=chi2.value, rho=rho, w=w)


def linearisation_graph():
    """8 nodes, 12 edges: residual rotations of 0 (an identity edge between two nodes at one pose), 1e-5, 1e-3, 1 and 2.5 rad,
    a backward edge, a duplicate pair, robust edges on both sides of the threshold, full information matrices."""
    rng = np.random.default_rng(77)
    poses = [K.pose(rng.standard_normal(3), 5 * rng.standard_normal(3)) for _ in range(8)]
    poses[5] = poses[4].copy()
    rows = []

    def edge(i, j, angle, shift, flags=0, sigma=(0.05, 0.1)):
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        Z = K.between(poses[i], poses[j])
        Z[:, :3] = Z[:, :3] @ R.exp_rotation(angle * axis).T
        Z[:, 3] += shift * rng.standard_normal(3)
        rows.append((i, j, Z, K.information(rng, *sigma), flags))

    edge(0, 1, 1e-5, 0.01)
    edge(1, 2, 1e-3, 0.01)
    edge(2, 3, 1.0, 0.5)
    edge(3, 4, 2.5, 1.0)
    rows.append((4, 5, K.pose([0, 0, 0], [0, 0, 0]), K.information(rng, 0.05, 0.1), 0))      # the identity edge: r = 0
    edge(5, 6, 0.0, 0.0)
    edge(6, 7, 0.2, 0.1)
    edge(7, 2, 0.3, 0.2)                                                                      # backward
    edge(1, 6, 0.02, 0.05, R.ROBUST, (0.05, 0.1))                                             # s below 3
    edge(0, 7, 1.5, 2.0, R.ROBUST)                                                            # s far above 3
    edge(2, 3, 1.0, 0.5)                                                                      # a second edge on (2, 3)
    edge(2, 3, 0.5, 0.2, R.ROBUST)                                                            # and a third
    return dict(poses=np.array(poses), edges=K.edges_of(rows), fixed=(), name="linearisation")


def _hold_linearisation(fx, g, plain, fused):
    """the device's r, rho, w, g and chi^2 of the graph g against the restatement's, under the bracket rule of the docstring"""
    pg = build(fx, g)
    got = linearize_on_device(fx, pg)
    largest = plain["largest"]
    failed = []
    for name, term in (("r", largest["r"]), ("rho", largest["rho"]), ("w", 1.0), ("g", largest["g"]), ("chi2", largest["rho"])):
        bracket = float(np.abs(np.asarray(plain[name]) - np.asarray(fused[name])).max())
        tol = max(16.0 * bracket, 4.0 * np.spacing(term))
        diff = float(np.abs(np.asarray(got[name]) - np.asarray(plain[name])).max())
        print("%-4s device - restatement %.3e; fused - unfused bracket %.3e; largest term %.3e; tolerance %.3e" % (name, diff, bracket, term, tol))
        if not diff <= tol:
            failed.append(name)
    assert not failed, failed
    pg.close()
    return got


@pytest.mark.gpu
def test_linearisation_against_the_restatement(fx):
    g = linearisation_graph()
    plain = R.linearize(g["poses"], g["edges"], fused=False)
    fused = R.linearize(g["poses"], g["edges"], fused=True)
    assert plain["w"][8] == 1.0 and plain["w"][9] < 0.1 and np.abs(plain["r"][4]).max() == 0.0
    _hold_linearisation(fx, g, plain, fused)


@pytest.mark.gpu
def test_linearisation_at_the_reference_residuals(fx):
    """The edges of tests/golden/pose_graph_residual_reference.json (residual rotations of 0, 1e-12, 1e-7, 9.9e-5, 1.01e-4,
    1e-2, 1, 2.5, 2.9 and 2.99 rad; the poses are the file's doubles), held to the restatement by the same bracket rule; the
    restatement is held to the file's 50-digit r in tests/test_pose_graph_expect.py.  The device's own distance from the
    reference is printed."""
    g = K.residual_reference_graph()
    plain = R.linearize(g["poses"], g["edges"], fused=False)
    fused = R.linearize(g["poses"], g["edges"], fused=True)
    got = _hold_linearisation(fx, g, plain, fused)
    for c, (angle, _Ti, _Tj, _Z, want) in enumerate(K.residual_reference()):
        print("residual angle %-8s device - reference %.2e (rotation) %.2e (translation); restatement - reference %.2e, %.2e" % (
            angle, np.abs(got["r"][c] - want)[:3].max(), np.abs(got["r"][c] - want)[3:].max(),
            np.abs(plain["r"][c] - want)[:3].max(), np.abs(plain["r"][c] - want)[3:].max()))
    assert (plain["w"][1::2] < 1.0).all() and (plain["w"][0::2] == 1.0).all()


def _one_step(fx, g, want):
    """One iteration of the graph g on the device, under g's own config, against the dense step `want`; the result's code
    and n_robust_downweighted are the restatement's after one iteration."""
    _, wres, _ = K.one_iteration(g["name"])
    pg = build(fx, g, max_iter=1, **K.config_of(g))
    res = pg.optimize(D.stream())
    after = pg.poses(stream=D.stream())
    got = R.step_between(g["poses"], after)
    tol = max(16.0 * K.floor_of(g["name"]), 1e-12 * np.abs(want).max())
    diff = float(np.abs(got - want).max())
    chain, loops = R.split_edges(g["edges"], len(g["poses"]))
    print("%s: device - dense %.3e, tolerance %.3e (floor %.2e, max |delta| %.2e); %d chain and %d loop edges; code %d (restatement %d), %d down-weighted (%d)" % (
        g["name"], diff, tol, K.floor_of(g["name"]), np.abs(want).max(), res["n_chain"], res["n_loop"], res["code"], wres["code"],
        res["n_robust_downweighted"], wres["n_robust_downweighted"]))
    assert (res["n_chain"], res["n_loop"]) == (int((chain >= 0).sum()), len(loops)) and res["iterations"] == 1
    assert wres["code"] in (R.CONVERGED, R.MAX_ITERATIONS) and res["code"] == wres["code"]
    assert res["n_robust_downweighted"] == wres["n_robust_downweighted"]
    assert abs(res["max_step"] - np.abs(want).max()) <= tol
    assert diff <= tol
    for k in set(g["fixed"]) | {0}:
        assert np.array_equal(pg.poses(k, 1, D.stream())[0], g["poses"][k])
    pg.close()
    return after


@pytest.mark.gpu
@pytest.mark.parametrize("g", K.step_shapes(), ids=lambda g: g["name"])
def test_one_step_against_the_dense_solve(fx, g):
    _one_step(fx, g, K.dense_first_steps()[g["name"]][0])


@pytest.mark.gpu
@pytest.mark.parametrize("g", K.extra_step_shapes(), ids=lambda g: g["name"])
def test_one_step_of_the_extra_shapes_against_the_dense_solve(fx, g):
    """Down-weighted chain edges (w in P's diagonal blocks twice and in the off-diagonal block, and beside a second fixed
    node), huber_delta = 0.5, damping 0, 1e-2 and 10, a last node without an edge: each under its own config, judged by
    R.dense_step with the same config, at the tolerance of the whole-chain class (tests/test_pose_graph_expect.py holds
    every one of these shapes below that floor)."""
    after = _one_step(fx, g, K.extra_first_steps()[g["name"]][0])
    if g["name"] == "dangling_last_node":                 # no edge, no loop: the step is 0 and the pose is not touched
        assert after[-1].tobytes() == g["poses"][-1].tobytes() and after[-2].tobytes() != g["poses"][-2].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1], ids=["circle_256_5", "circle_256_40"])
def test_convergence_on_the_circles(fx, which):
    g = K.circles()[which]
    want, wres, _ = K.circle_results()[which]
    pg = build(fx, g)
    res = pg.optimize(D.stream())
    got = pg.poses(stream=D.stream())
    f = K.floor_of(g["name"])
    dt = float(np.abs(got[:, :, 3] - want[:, :, 3]).max())
    dr = float(np.abs(got[:, :, :3] - want[:, :, :3]).max())
    ortho = float(np.abs(np.einsum("kij,kil->kjl", got[:, :, :3], got[:, :, :3]) - np.eye(3)).max())
    rel = abs(res["chi2_final"] - wres["chi2_final"]) / wres["chi2_final"]
    print("%s: %d iterations (restatement %d); translation %.2e, rotation %.2e (64 f = %.2e); chi2 %.9e vs %.9e (relative %.1e); "
          "|R^T R - I| %.1e; worst position error %.3f -> %.3f m" % (g["name"], res["iterations"], wres["iterations"], dt, dr, 64 * f,
                                                                      res["chi2_final"], wres["chi2_final"], rel, ortho,
                                                                      K.worst_error(g["poses"], g["truth"]), K.worst_error(got, g["truth"])))
    assert res["code"] == R.CONVERGED and abs(res["iterations"] - wres["iterations"]) <= 1
    assert dt <= 64 * f and dr <= 64 * f
    assert rel <= 1e-9 and abs(res["chi2_initial"] - wres["chi2_initial"]) <= 1e-9 * wres["chi2_initial"]
    assert ortho <= 1e-12
    # the view is where the poses live
    ptr, n = pg.view(D.stream())
    assert n == len(got) and ptr
    D.sync()
    probe = np.zeros((n, 3, 4))
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(probe.ctypes.data, ptr, probe.nbytes, 2) == 0
    assert probe.tobytes() == got.tobytes()
    pg.close()


@pytest.mark.gpu
def test_the_same_graph_gives_the_same_bytes(fx):
    g = K.circles()[0]
    runs = []
    for calls in (1, 1, 3):
        pg = build(fx, g, edge_calls=calls)
        res = pg.optimize(D.stream())
        runs.append((pg.poses(stream=D.stream()).tobytes(), res, pg.edge_chi2(stream=D.stream())[0].tobytes()))
        if calls == 3:                               # ... and once more in the same graph from the same start
            pg.set_poses(g["poses"], 0, D.stream())
            res = pg.optimize(D.stream())
            runs.append((pg.poses(stream=D.stream()).tobytes(), res, pg.edge_chi2(stream=D.stream())[0].tobytes()))
        pg.close()
    for r in runs[1:]:
        assert r[0] == runs[0][0] and r[1] == runs[0][1] and r[2] == runs[0][2]


@pytest.mark.gpu
def test_a_false_loop_is_singled_out(fx):
    errs, cpu, runs = {}, K.false_loop_results(), K.false_loop_runs()
    for name, g in zip(("robust", "plain", "clean"), K.false_loop_cases()):
        pg = build(fx, g, max_iter=20, huber_delta=3.0)
        res = pg.optimize(D.stream())
        rho, w = pg.edge_chi2(stream=D.stream())
        errs[name] = K.worst_error(pg.poses(stream=D.stream()), g["truth"])
        print("%s: code %d after %d iterations, worst position error %.4f m (restatement %.4f m); smallest w %.5f at edge %d; %d down-weighted" % (
            name, res["code"], res["iterations"], errs[name], cpu[name], w.min(), int(w.argmin()), res["n_robust_downweighted"]))
        if name == "robust":
            assert int(w.argmin()) == 255 + 2 and w.min() < 0.1 and res["n_robust_downweighted"] >= 1
            assert (w[:255] == 1.0).all()
        assert abs(errs[name] - cpu[name]) <= 1e-6
        assert res["n_robust_downweighted"] == runs[name][1]["n_robust_downweighted"] == int((w < 1.0).sum())
        pg.close()
    assert errs["robust"] <= 2.0 * errs["clean"] < errs["plain"]


def _fresh(fx, poses, edges, fixed, **config):
    """a new graph of the grown one's capacities: the nodes, the fixed flags, every edge in one call"""
    pg = fx.pose_graph(48, 52, **config)
    assert pg.add_nodes(poses, D.stream()) == 0
    for k in fixed:
        pg.set_fixed(k, True, D.stream())
    pg.add_edges(edges, D.stream())
    return pg


@pytest.mark.gpu
def test_a_graph_that_grows(fx):
    """A 48-node graph grown as a mapping run grows it (tests/pose_graph_cases.py growth_stages()): add nodes, add their
    edges, optimise, four times -- the incidence lists go up again, ldy changes with the number of loops, node 47 waits a
    stage for its edge, an edge on (40, 41) that arrives first is the chain edge and the later one a loop, node 20 is
    fixed for stage 3 and free again for stage 4.  After every stage the grown graph's poses, result and per-edge figures
    are, byte for byte, those of a fresh graph given the same nodes (at the poses the grown one held before the stage's
    optimise), edges and flags at once; the stage's first step is held to the dense step at the whole-chain tolerance
    (tests/test_pose_graph_expect.py holds the stages below that floor)."""
    from lidar_feature_extraction_amd import binding as B
    poses, _ = K.growth_graph()
    pg = fx.pose_graph(48, 52)
    edges, have = np.zeros(0, K.EDGE), 0
    tol_floor = 16.0 * K.floors()[0]
    for stage, (n, calls, fixed) in enumerate(K.growth_stages(), 1):
        if n > have:
            assert pg.add_nodes(poses[have:n], D.stream()) == have
            have = n
            with pytest.raises(B.LfxError) as err:                     # nodes were added: the last optimise's figures are gone
                pg.edge_chi2(0, 1, D.stream())
            assert err.value.code == -1
        for call in calls:
            pg.add_edges(call, D.stream())
            edges = np.concatenate([edges, call])
        if stage == 3:
            pg.set_fixed(20, True, D.stream())
        if stage == 4:
            pg.set_fixed(20, False, D.stream())
        chain, loops = R.split_edges(edges, n)
        info = pg.info()
        assert (info["n_nodes"], info["n_edges"], info["n_chain"], info["n_loop"]) == (n, len(edges), int((chain >= 0).sum()), len(loops))
        start = pg.poses(stream=D.stream())
        res = pg.optimize(D.stream())
        got, (rho, w) = pg.poses(stream=D.stream()), pg.edge_chi2(stream=D.stream())
        fresh = _fresh(fx, start, edges, fixed)
        fres = fresh.optimize(D.stream())
        fgot, (frho, fw) = fresh.poses(stream=D.stream()), fresh.edge_chi2(stream=D.stream())
        fresh.close()
        once = _fresh(fx, start, edges, fixed, max_iter=1)
        once.optimize(D.stream())
        step = R.step_between(start, once.poses(stream=D.stream()))
        once.close()
        want, _lin = R.dense_step(start, edges, fixed)
        tol = max(tol_floor, 1e-12 * np.abs(want).max())
        diff = float(np.abs(step - want).max())
        print("stage %d: %d nodes, %d chain and %d loop edges, fixed %s: code %d after %d iterations, %d down-weighted, chi2 %.6e -> %.6e; "
              "first step: device - dense %.3e, tolerance %.3e (max |delta| %.3e)" % (
                  stage, n, info["n_chain"], info["n_loop"], fixed, res["code"], res["iterations"], res["n_robust_downweighted"], res["chi2_initial"],
                  res["chi2_final"], diff, tol, np.abs(want).max()))
        assert res["code"] == R.CONVERGED and res == fres
        assert got.tobytes() == fgot.tobytes() and rho.tobytes() == frho.tobytes() and w.tobytes() == fw.tobytes()
        assert diff <= tol
        assert res["n_robust_downweighted"] == int((w < 1.0).sum())
        # a range in the middle and the last edge alone are the whole read's slices
        E = len(edges)
        for first, count in ((E // 3, E // 2), (E - 1, 1), (1, 1)):
            prho, pw = pg.edge_chi2(first, count, D.stream())
            assert prho.tobytes() == rho[first:first + count].tobytes() and pw.tobytes() == w[first:first + count].tobytes()
        assert len(set(rho.tolist())) == E                          # (no two edges alike: a slice from the wrong place shows)
        if stage == 3:
            assert got[20].tobytes() == start[20].tobytes() and got[47].tobytes() == poses[47].tobytes()
            assert w[34] < 0.1 and (np.delete(w, 34) == 1.0).all()
        if stage == 4:
            assert np.abs(got[20] - start[20]).max() > 1e-6 and np.abs(got[47] - start[47]).max() > 1e-6
    pg.close()


@pytest.mark.gpu
def test_an_information_matrix_that_overflows(fx):
    """One chain edge's information scaled by 1e300: finite and symmetric, so add_edges takes it, and Omega r is beyond the
    doubles.  The call returns LFX_OK with NOT_POSITIVE_DEFINITE or DIVERGED, the poses are the start's byte for byte and
    hold no NaN, and chi2_final is chi2_initial, as the header says for both codes."""
    g = K.graph(12, loops=[(0, 11), (2, 9)], seed=40)
    big = g["edges"].copy()
    big[4]["information"] = big[4]["information"] * 1e300
    assert np.isfinite(big[4]["information"]).all() and np.abs(big[4]["information"]).max() > 1e304
    pg = build(fx, dict(g, edges=big))
    res = pg.optimize(D.stream())
    after = pg.poses(stream=D.stream())
    print("information x 1e300 on chain edge 4: code %d after %d iterations, chi2 %r -> %r, max_step %r" % (
        res["code"], res["iterations"], res["chi2_initial"], res["chi2_final"], res["max_step"]))
    assert res["code"] in (R.NOT_POSITIVE_DEFINITE, R.DIVERGED)
    assert after.tobytes() == g["poses"].tobytes() and not np.isnan(after).any()
    assert res["chi2_final"] == res["chi2_initial"]
    pg.close()


def _kernel_launches(fx):
    return {k: v[1] for k, v in fx.kernel_times().items() if k.startswith("pose_graph_")}


@pytest.mark.gpu
def test_refusals(fx):
    g = K.graph(12, loops=[(0, 11), (2, 9)], seed=40)
    # an information matrix with a large negative eigenvalue on a chain edge breaks P; on a loop edge, its own factor
    for edge in (4, 11):
        bad = g["edges"].copy()
        om = bad[edge]["information"].reshape(6, 6).copy()
        om[4, 4] = -1e7
        bad[edge]["information"] = om.reshape(36)
        pg = build(fx, dict(g, edges=bad))
        before = pg.poses(stream=D.stream()).tobytes()
        res = pg.optimize(D.stream())
        print("edge %d not positive definite: code %d, iterations %d" % (edge, res["code"], res["iterations"]))
        assert res["code"] == R.NOT_POSITIVE_DEFINITE and pg.poses(stream=D.stream()).tobytes() == before == g["poses"].tobytes()
        assert res["chi2_final"] == res["chi2_initial"]
        pg.close()
    # the same refusal over more than one workgroup of the linearisation (64 edges each): the loop edge without a factor is
    # edge 0, in the first workgroup; every other edge's values must be written all the same, so chi^2 and the per-edge
    # figures of the refused call are those of the start whatever order the workgroups ran in
    wide = K.graph(100, loops=[(3, 70), (10, 95), (50, 20)], seed=41)
    order = np.concatenate([np.arange(99, 102), np.arange(99)])          # the loops first
    bad = wide["edges"][order].copy()
    om = bad[0]["information"].reshape(6, 6).copy()
    om[4, 4] = -1e7
    bad[0]["information"] = om.reshape(36)
    want = R.linearize(wide["poses"], bad)
    pg = build(fx, dict(wide, edges=bad))
    res = pg.optimize(D.stream())
    rho, w = pg.edge_chi2(stream=D.stream())
    print("102 edges, edge 0 not positive definite: code %d, chi2 %.9e (restatement %.9e), rho within %.2e" % (
        res["code"], res["chi2_initial"], want["chi2"], np.abs(rho - want["rho"]).max()))
    assert res["code"] == R.NOT_POSITIVE_DEFINITE and res["n_loop"] == 3 and pg.poses(stream=D.stream()).tobytes() == wide["poses"].tobytes()
    assert abs(res["chi2_initial"] - want["chi2"]) <= 1e-9 * abs(want["chi2"]) and res["chi2_final"] == res["chi2_initial"]
    assert np.abs(rho - want["rho"]).max() <= 1e-9 * np.abs(want["rho"]).max() and (w == 1.0).all()
    pg.close()
    # a start from which the first step makes chi^2 larger: the initial poses come back
    far = K.graph(12, loops=[(0, 11), (2, 9)], seed=40, start=(2.0, 3.0))
    _, wres, _ = R.optimize(far["poses"], far["edges"], max_iter=1)
    pg = build(fx, far, max_iter=1)
    res = pg.optimize(D.stream())
    print("diverging start: code %d (restatement %d), chi2 %.4e" % (res["code"], wres["code"], res["chi2_initial"]))
    assert wres["code"] == R.DIVERGED and res["code"] == R.DIVERGED and pg.poses(stream=D.stream()).tobytes() == far["poses"].tobytes()
    assert res["chi2_final"] == res["chi2_initial"] and abs(res["chi2_initial"] - wres["chi2_initial"]) <= 1e-9 * wres["chi2_initial"]
    rho, _w = pg.edge_chi2(stream=D.stream())
    assert abs(rho.sum() - res["chi2_initial"]) <= 1e-9 * res["chi2_initial"]
    pg.close()
    # capacities: nothing changes
    from lidar_feature_extraction_amd import binding as B
    pg = fx.pose_graph(12, 13, max_loop_edges=1)
    pg.add_nodes(g["poses"], D.stream())
    with pytest.raises(B.LfxError) as err:
        pg.add_nodes(g["poses"][:1], D.stream())
    assert err.value.code == -4 and len(pg) == 12
    pg.add_edges(g["edges"][:12], D.stream())
    with pytest.raises(B.LfxError) as err:
        pg.add_edges(g["edges"][:2], D.stream())                 # 14 edges
    assert err.value.code == -4
    with pytest.raises(B.LfxError) as err:
        pg.add_edges(g["edges"][11:12], D.stream())              # a second loop edge
    assert err.value.code == -4 and pg.info()["n_edges"] == 12 and pg.info()["n_loop"] == 1
    info = pg.info()
    assert info["device_bytes"] > 12 * 96 * 2 + 13 * 400
    # invalid arguments: refused with nothing launched
    fx._L.lfx_set_profiling(fx._ctx, 1)
    pg.optimize(D.stream())
    launched = _kernel_launches(fx)
    assert launched["pose_graph_linearize_kernel"] >= 2 and launched["pose_graph_chain_factor_kernel"] >= 1 and launched["pose_graph_s_diag_kernel"] >= 1
    start = pg.poses(stream=D.stream()).tobytes()
    nan_pose = g["poses"][:1].copy()
    nan_pose[0, 1, 3] = np.nan
    skew, same, outside, flags = (g["edges"][12:13].copy() for _ in range(4))
    om = skew[0]["information"].reshape(6, 6).copy()
    om[1, 2] += 1.0
    skew[0]["information"] = om.reshape(36)
    same[0]["j"] = same[0]["i"]
    outside[0]["j"] = 12
    flags[0]["flags"] = 2
    small = fx.pose_graph(13, 13, max_loop_edges=4)
    small.add_nodes(g["poses"], D.stream())
    for call in (lambda: small.add_nodes(nan_pose, D.stream()), lambda: small.set_poses(nan_pose, 3, D.stream()),
                 lambda: small.add_edges(skew, D.stream()), lambda: small.add_edges(same, D.stream()),
                 lambda: small.add_edges(outside, D.stream()), lambda: small.add_edges(flags, D.stream()),
                 lambda: small.optimize(D.stream()), lambda: small.set_fixed(12, True, D.stream()),
                 lambda: small.poses(5, 8, D.stream()), lambda: pg.edge_chi2(0, 13, D.stream())):
        with pytest.raises(B.LfxError) as err:
            call()
        assert err.value.code == -1, err.value
    assert _kernel_launches(fx) == launched
    assert small.info()["n_edges"] == 0 and len(small) == 12 and pg.poses(stream=D.stream()).tobytes() == start
    fx._L.lfx_set_profiling(fx._ctx, 0)
    small.close()
    pg.close()


@pytest.fixture(scope="module")
def hold():
    h = S.Hold()
    yield h
    for what, ms in h.issue_ms:
        print("held %.0f ms; issued %.3f ms after the hold was queued: %s" % (S.HOLD_MS, ms, what))


@pytest.mark.gpu
def test_optimize_waits_for_set_poses_on_another_stream(fx, hold):
    """The held-producer pattern of tests/test_newer_streams_gpu.py: the graph is warmed by one optimise; then other poses
    are written and, on held stream A, the start is written back; optimise is issued on B while A has not run.  Only the
    library's own wait (hipStreamWaitEvent on the graph's event) can put it behind: the result must be the first run's."""
    g = K.step_shapes()[2]
    pg = build(fx, g)
    first = pg.optimize(D.stream())
    want = pg.poses(stream=D.stream()).tobytes()
    a, b = S.two_streams()
    pg.set_poses(g["truth"], 0, D.stream())
    D.sync()
    hold(a)
    pg.set_poses(g["poses"], 0, a.cuda_stream)
    e = S.event_behind(a)
    hold.still_held(e, "pose graph: set_poses on A, optimize on B")
    res = pg.optimize(b.cuda_stream)
    assert res == first and pg.poses(stream=b.cuda_stream).tobytes() == want
    # ... and the poses read on A behind an optimise on B
    hold(b)
    pg.set_poses(g["truth"], 0, b.cuda_stream)
    e = S.event_behind(b)
    hold.still_held(e, "pose graph: set_poses on B, poses on A")
    assert pg.poses(stream=a.cuda_stream).tobytes() == g["truth"].tobytes()
    D.sync()
    pg.close()
