"""Priors on the device (lfx_pose_graph_reserve_priors, _add_priors, _release_first, _prior_chi2, _prior_info) against the
restatement with priors (tests/pose_graph_prior_restatement.py; the graphs: tests/pose_graph_prior_cases.py).

Linearisation: the bracket rule of tests/test_pose_graph_gpu.py (16 x fused - unfused, a floor of 4 ulp of the largest
term), through lfx_test_pose_graph_prior_linearize; a pose prior's r, rho and w are, value for value, the anchored edge's.
One step: every shape against the new dense step at max(16 K.floors()[0], 1e-12 max |delta|), the one-step tolerance of
the whole-chain class (tests/test_pose_graph_prior_expect.py holds every shape below that floor).  Convergence: the drift
case as tests/test_pose_graph_gpu.py holds its circles.  Then bytes, refusals and streams.
Every test prints its figures before it asserts."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import deskew_cases as D
from tests import pose_graph_cases as K
from tests import pose_graph_prior_cases as PK
from tests import pose_graph_prior_restatement as Q
from tests import pose_graph_restatement as R
from tests import segment_cases as S


@pytest.fixture(scope="module")
def fx():
    f = D.fx_for(16, 900, 1, test_hooks=True)       # (the test-hooks build: lfx_test_pose_graph_prior_linearize)
    yield f
    f.close()


def build(fx, g, calls=1, **config):
    """The graph g on the device: nodes, fixed flags, the release, the reserve, then edges and priors in `calls` calls each,
    taking turns."""
    n, e, p = len(g["poses"]), g["edges"], g["priors"]
    pg = fx.pose_graph(n, max(len(e), 1), **config)
    assert pg.add_nodes(g["poses"], D.stream()) == 0
    for k in g["fixed"]:
        pg.set_fixed(k, True, D.stream())
    if g["released"]:
        pg.release_first(True, D.stream())
    pg.reserve_priors(max(len(p), 1))
    ecuts = [len(e) * c // calls for c in range(calls + 1)]
    pcuts = [len(p) * c // calls for c in range(calls + 1)]
    for c in range(calls):
        pg.add_priors(p[pcuts[c]:pcuts[c + 1]], D.stream())
        pg.add_edges(e[ecuts[c]:ecuts[c + 1]], D.stream())
    return pg


def build_anchored(fx, g, **config):
    """The anchored form of g through the calls that existed before priors: (graph, its poses at the start)"""
    poses, edges, fixed = PK.anchored(g)
    pg = fx.pose_graph(len(poses), len(edges), **config)
    assert pg.add_nodes(poses, D.stream()) == 0
    for k in fixed:
        pg.set_fixed(k, True, D.stream())
    pg.add_edges(edges, D.stream())
    return pg, poses


def _hook(fx, pg, name, rows):
    info = pg.info()
    r, g, chi2 = np.zeros((rows, 6)), np.zeros((info["n_nodes"], 6)), C.c_double(0.0)
    fn = getattr(fx._L, name)
    fn.argtypes = [C.c_void_p] * 4 + [C.POINTER(C.c_double), C.c_void_p]
    rc = fn(fx._ctx, pg.handle, C.c_void_p(r.ctypes.data), C.c_void_p(g.ctypes.data), C.byref(chi2), C.c_void_p(D.stream()))
    assert rc == 0, fx._L.lfx_last_error(fx._ctx)
    return r, g, chi2.value


def linearize_on_device(fx, pg):
    r, g, chi2 = _hook(fx, pg, "lfx_test_pose_graph_prior_linearize", pg.prior_info()["n_priors"])
    rho, w = pg.prior_chi2(stream=D.stream())
    out = dict(p_r=r, g=g, chi2=chi2, p_rho=rho, p_w=w)
    if pg.info()["n_edges"]:
        out["rho"], out["w"] = pg.edge_chi2(stream=D.stream())
    return out


@pytest.mark.gpu
def test_linearisation_against_the_restatement(fx):
    g = PK.linearisation_case()
    args = (g["poses"], g["edges"], g["priors"], g["fixed"], g["released"])
    plain, fused = Q.linearize(*args, fused=False), Q.linearize(*args, fused=True)
    pg = build(fx, g)
    got = linearize_on_device(fx, pg)
    largest = plain["largest"]
    failed = []
    for name, term in (("p_r", largest["r"]), ("p_rho", largest["rho"]), ("p_w", 1.0), ("rho", largest["rho"]), ("w", 1.0), ("g", largest["g"]),
                       ("chi2", largest["rho"])):
        bracket = float(np.abs(np.asarray(plain[name]) - np.asarray(fused[name])).max())
        tol = max(16.0 * bracket, 4.0 * np.spacing(term))
        diff = float(np.abs(np.asarray(got[name]) - np.asarray(plain[name])).max())
        print("%-5s device - restatement %.3e; fused - unfused bracket %.3e; largest term %.3e; tolerance %.3e" % (name, diff, bracket, term, tol))
        if not diff <= tol:
            failed.append(name)
    assert not failed, failed
    info = pg.prior_info()
    assert info["n_priors"] == len(g["priors"]) and info["max_priors"] == len(g["priors"]) and info["reserved"] == 0
    pg.close()
    # the pose priors alone, against the anchored graph's edges on the device: the same routine, so the same values
    pose_kind = (g["priors"]["flags"] & Q.PRIOR_POSITION) == 0
    h = dict(g, priors=g["priors"][pose_kind])
    P = len(h["priors"])
    pg = build(fx, h)
    mine = linearize_on_device(fx, pg)
    pg.close()
    anchor, _ = build_anchored(fx, h)
    r, _g, chi2 = _hook(fx, anchor, "lfx_test_pose_graph_linearize", anchor.info()["n_edges"])
    rho, w = anchor.edge_chi2(stream=D.stream())
    anchor.close()
    print("%d pose priors against the anchored edges: r differs in %d values, rho in %d, w in %d; chi2 %.17g vs %.17g" % (
        P, int((mine["p_r"] != r[-P:]).sum()), int((mine["p_rho"] != rho[-P:]).sum()), int((mine["p_w"] != w[-P:]).sum()), mine["chi2"], chi2))
    assert np.array_equal(mine["p_r"], r[-P:]) and np.array_equal(mine["p_rho"], rho[-P:]) and np.array_equal(mine["p_w"], w[-P:])
    assert np.array_equal(mine["rho"], rho[:-P]) and np.array_equal(mine["w"], w[:-P])


@pytest.mark.gpu
@pytest.mark.parametrize("g", PK.step_shapes(), ids=lambda g: g["name"])
def test_one_step_against_the_dense_solve(fx, g):
    want, wlin = PK.dense_first_steps()[g["name"]]
    _, wres, _, _ = PK.one_iteration(g["name"])
    pg = build(fx, g, max_iter=1, **PK.config_of(g))
    res = pg.optimize(D.stream())
    after = pg.poses(stream=D.stream())
    info = pg.prior_info()
    got = R.step_between(g["poses"], after)
    tol = max(16.0 * K.floors()[0], 1e-12 * np.abs(want).max())
    diff = float(np.abs(got - want).max())
    print("%s: device - dense %.3e, tolerance %.3e (max |delta| %.2e); code %d (restatement %d); down-weighted: %d edges (%d), %d priors (%d); "
          "chi2 %.9e -> %.9e (restatement %.9e -> %.9e), the priors' share %.9e (%.9e)" % (
              g["name"], diff, tol, np.abs(want).max(), res["code"], wres["code"], res["n_robust_downweighted"], wres["n_robust_downweighted"],
              info["n_downweighted"], wres["n_prior_downweighted"], res["chi2_initial"], res["chi2_final"], wres["chi2_initial"], wres["chi2_final"],
              info["chi2"], wres["chi2_priors"]))
    assert res["iterations"] == 1 and res["code"] == wres["code"] and wres["code"] in (R.CONVERGED, R.MAX_ITERATIONS)
    assert res["n_robust_downweighted"] == wres["n_robust_downweighted"] and info["n_downweighted"] == wres["n_prior_downweighted"]
    assert abs(res["chi2_initial"] - wlin["chi2"]) <= 1e-9 * wlin["chi2"]
    assert abs(res["max_step"] - np.abs(want).max()) <= tol
    assert diff <= tol
    for k in set(g["fixed"]) | (set() if g["released"] else {0}):
        assert np.array_equal(pg.poses(k, 1, D.stream())[0], g["poses"][k]) and after[k].tobytes() == g["poses"][k].tobytes()
    if g["released"]:
        assert after[0].tobytes() != g["poses"][0].tobytes()
    if g["name"] == "prior_on_an_isolated_node":           # no edge touches node 10: it moves to its prior
        assert after[10].tobytes() != g["poses"][10].tobytes()
    pg.close()


@pytest.mark.gpu
def test_the_anchored_form_on_the_device(fx):
    """N64_L3 with 16 pose priors, optimised as priors and as the anchored graph (an extra fixed node at the identity, every
    prior an edge from it: 15 of them loop edges), both on the device."""
    rng = np.random.default_rng(700)
    base = [s for s in K.step_shapes() if s["name"] == "N64_L3"][0]
    g = PK.with_priors(base, "N64_L3_16_pose_priors", [PK.pose_row(base["truth"][k], k, rng) for k in range(0, 64, 4)])
    pg = build(fx, g)
    t0 = time.perf_counter()
    res = pg.optimize(D.stream())
    t1 = time.perf_counter()
    got = pg.poses(stream=D.stream())
    anchor, start = build_anchored(fx, g)
    t2 = time.perf_counter()
    ares = anchor.optimize(D.stream())
    t3 = time.perf_counter()
    want = anchor.poses(stream=D.stream())
    step = np.abs(R.step_between(start[1:], want[1:])).max()
    tol = max(16.0 * K.floors()[0], 1e-12 * step)
    diff = float(np.abs(got - want[1:]).max())
    print("prior form: code %d after %d iterations, chi2 %.9e, %.2f ms; anchored form: code %d after %d, chi2 %.9e, %d loop edges, %.2f ms; "
          "poses differ by %.3e (tolerance %.3e)" % (res["code"], res["iterations"], res["chi2_final"], 1e3 * (t1 - t0), ares["code"], ares["iterations"],
                                                     ares["chi2_final"], ares["n_loop"], 1e3 * (t3 - t2), diff, tol))
    assert res["code"] == ares["code"] == R.CONVERGED and res["n_loop"] == 3 and ares["n_loop"] == 3 + 15
    assert want[0].tobytes() == start[0].tobytes() and diff <= tol
    assert abs(res["chi2_final"] - ares["chi2_final"]) <= 1e-9 * ares["chi2_final"]
    pg.close()
    anchor.close()


@pytest.mark.gpu
def test_convergence_on_the_drifting_chain(fx):
    g = PK.drift_case()
    want, wres, _, (wrho, ww) = PK.drift_result()
    pg = build(fx, g, **PK.DRIFT_CONFIG)
    res = pg.optimize(D.stream())
    got = pg.poses(stream=D.stream())
    rho, w = pg.prior_chi2(stream=D.stream())
    info = pg.prior_info()
    f = K.floors()[0]
    dt = float(np.abs(got[:, :, 3] - want[:, :, 3]).max())
    dr = float(np.abs(got[:, :, :3] - want[:, :, :3]).max())
    ortho = float(np.abs(np.einsum("kij,kil->kjl", got[:, :, :3], got[:, :, :3]) - np.eye(3)).max())
    rel = abs(res["chi2_final"] - wres["chi2_final"]) / wres["chi2_final"]
    before, after, cpu = K.worst_error(g["poses"], g["truth"]), K.worst_error(got, g["truth"]), K.worst_error(want, g["truth"])
    print("%s: %d iterations (restatement %d); translation %.2e, rotation %.2e (64 f = %.2e); chi2 %.9e vs %.9e (relative %.1e), the priors' share "
          "%.9e vs %.9e; |R^T R - I| %.1e; smallest w %.5f at prior %d; worst position error %.3f -> %.3f m (restatement %.3f m)" % (
              g["name"], res["iterations"], wres["iterations"], dt, dr, 64 * f, res["chi2_final"], wres["chi2_final"], rel, info["chi2"],
              wres["chi2_priors"], ortho, w.min(), int(w.argmin()), before, after, cpu))
    assert res["code"] == R.CONVERGED and abs(res["iterations"] - wres["iterations"]) <= 1
    assert dt <= 64 * f and dr <= 64 * f
    assert rel <= 1e-9 and abs(res["chi2_initial"] - wres["chi2_initial"]) <= 1e-9 * wres["chi2_initial"]
    assert abs(info["chi2"] - wres["chi2_priors"]) <= 1e-9 * wres["chi2_priors"] and abs(rho.sum() - info["chi2"]) <= 1e-9 * info["chi2"]
    assert ortho <= 1e-12
    assert int(w.argmin()) == PK.DRIFT_OUTLIER and np.flatnonzero(w < 1.0).tolist() == [PK.DRIFT_OUTLIER] and info["n_downweighted"] == 1
    assert res["n_robust_downweighted"] == 0 and res["n_chain"] == 255 and res["n_loop"] == 0
    assert got[0].tobytes() != g["poses"][0].tobytes()
    assert after < before and abs(after - cpu) <= 1e-6
    pg.close()


@pytest.mark.gpu
def test_the_same_graph_gives_the_same_bytes(fx):
    g = PK.shape("65_priors")
    runs = []
    for calls in (1, 1, 3):
        pg = build(fx, g, calls=calls)
        res = pg.optimize(D.stream())
        runs.append((pg.poses(stream=D.stream()).tobytes(), res, pg.prior_chi2(stream=D.stream())[0].tobytes(), pg.prior_info()))
        if calls == 3:                               # ... and once more in the same graph from the same start
            pg.set_poses(g["poses"], 0, D.stream())
            res = pg.optimize(D.stream())
            runs.append((pg.poses(stream=D.stream()).tobytes(), res, pg.prior_chi2(stream=D.stream())[0].tobytes(), pg.prior_info()))
        pg.close()
    print("65 priors and 70 edges in 1, 1 and 3 + 3 interleaved calls, then again: code %d after %d iterations, chi2 %.17g" % (
        runs[0][1]["code"], runs[0][1]["iterations"], runs[0][1]["chi2_final"]))
    for r in runs[1:]:
        assert r[0] == runs[0][0] and r[1] == runs[0][1] and r[2] == runs[0][2] and r[3] == runs[0][3]


def _kernel_launches(fx):
    return {k: v[1] for k, v in fx.kernel_times().items() if k.startswith("pose_graph_")}


def _bad_priors(g):
    """name -> one prior record that lfx_pose_graph_add_priors must refuse as an invalid argument"""
    rng = np.random.default_rng(701)
    pose = PK.priors_of([PK.pose_row(g["truth"][3], 3, rng)])
    position = PK.priors_of([PK.position_row(g["truth"][3], 3, rng, PK.LEVER)])
    out = {}

    def variant(name, base, field, index, value):
        p = base.copy()
        v = p[0][field].copy() if index is not None else None
        if index is None:
            p[0][field] = value
        else:
            v[index] = value
            p[0][field] = v
        out[name] = p

    variant("a node that is not in the graph", pose, "node", None, len(g["poses"]))
    variant("unknown flags", pose, "flags", None, 4)
    variant("z not finite", pose, "z", 7, np.nan)
    variant("information not finite", pose, "information", 0, np.inf)
    variant("lever not finite", position, "lever", 1, np.nan)
    om = pose[0]["information"].reshape(6, 6).copy()
    om[1, 2] += 1.0
    variant("information not symmetric", pose, "information", slice(None), om.reshape(36))
    variant("a position prior with information outside its block", position, "information", 0, 1.0)
    variant("a pose prior with a lever", pose, "lever", 2, 0.5)
    return out, pose, position


REFUSAL_GRAPH = K.graph(12, loops=[(0, 11), (2, 9)], seed=40)
BAD_PRIORS = _bad_priors(REFUSAL_GRAPH)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BAD_PRIORS), ids=lambda n: n.replace(" ", "_"))
def test_add_priors_refuses_an_invalid_argument(fx, name):
    """One argument check each: LFX_ERR_INVALID_ARGUMENT, the graph as it was (its priors, their figures of the last optimise
    still readable, its poses), nothing launched -- also with a good prior in front of the bad one."""
    from lidar_feature_extraction_amd import binding as B
    g = REFUSAL_GRAPH
    _bad, pose, position = _bad_priors(g)
    pg = fx.pose_graph(12, 13)
    pg.add_nodes(g["poses"], D.stream())
    pg.add_edges(g["edges"], D.stream())
    pg.reserve_priors(4)
    pg.add_priors(np.concatenate([pose, position]), D.stream())
    fx._L.lfx_set_profiling(fx._ctx, 1)
    pg.optimize(D.stream())
    rho, w = pg.prior_chi2(stream=D.stream())
    launched, start = _kernel_launches(fx), pg.poses(stream=D.stream()).tobytes()
    for records in (BAD_PRIORS[name], np.concatenate([position, BAD_PRIORS[name]])):
        with pytest.raises(B.LfxError) as err:
            pg.add_priors(records, D.stream())
        print("%-52s code %d: %s" % (name, err.value.code, str(err.value)[:100]))
        assert err.value.code == -1
    after = pg.prior_chi2(stream=D.stream())
    assert pg.prior_info()["n_priors"] == 2 and after[0].tobytes() == rho.tobytes() and after[1].tobytes() == w.tobytes()
    assert _kernel_launches(fx) == launched and pg.poses(stream=D.stream()).tobytes() == start
    fx._L.lfx_set_profiling(fx._ctx, 0)
    pg.close()


@pytest.mark.gpu
def test_refusals(fx):
    from lidar_feature_extraction_amd import binding as B
    g = REFUSAL_GRAPH
    bad, pose, position = _bad_priors(g)
    pg = fx.pose_graph(12, 13)
    pg.add_nodes(g["poses"], D.stream())
    pg.add_edges(g["edges"], D.stream())
    # nothing reserved: a capacity of 0
    with pytest.raises(B.LfxError) as err:
        pg.add_priors(pose, D.stream())
    assert err.value.code == -4 and pg.prior_info() == dict(n_priors=0, max_priors=0, n_downweighted=0, reserved=0, chi2=0.0)
    with pytest.raises(B.LfxError) as err:
        pg.reserve_priors(0)
    assert err.value.code == -1
    before = pg.info()["device_bytes"]
    pg.reserve_priors(3)
    grown = pg.info()["device_bytes"] - before
    print("reserve_priors(3) on 12 nodes: device_bytes grows by %d" % grown)
    assert grown == 3 * 416 + 3 * 52 * 8 + (12 + 1 + 3) * 4
    with pytest.raises(B.LfxError) as err:
        pg.reserve_priors(3)
    assert err.value.code == -1 and pg.info()["device_bytes"] == before + grown
    pg.add_priors(np.concatenate([pose, position]), D.stream())
    with pytest.raises(B.LfxError) as err:
        pg.add_priors(np.concatenate([pose, position]), D.stream())          # 4 of 3
    assert err.value.code == -4 and pg.prior_info()["n_priors"] == 2
    with pytest.raises(B.LfxError) as err:
        pg.prior_chi2(stream=D.stream())                                     # before an optimise
    assert err.value.code == -1
    fx._L.lfx_set_profiling(fx._ctx, 1)
    first = pg.optimize(D.stream())
    rho, w = pg.prior_chi2(stream=D.stream())
    assert len(rho) == 2 and abs(rho.sum() - pg.prior_info()["chi2"]) <= 1e-9 * rho.sum()
    launched = _kernel_launches(fx)
    start = pg.poses(stream=D.stream()).tobytes()
    # (the argument checks of add_priors: test_add_priors_refuses_an_invalid_argument)  a range outside the priors; a graph
    # with neither edges nor priors: refused, nothing launched
    with pytest.raises(B.LfxError) as err:
        pg.prior_chi2(1, 2, D.stream())
    assert err.value.code == -1
    empty = fx.pose_graph(4, 4)
    empty.add_nodes(g["poses"][:4], D.stream())
    empty.reserve_priors(2)
    with pytest.raises(B.LfxError) as err:                                   # no edge and no prior
        empty.optimize(D.stream())
    assert err.value.code == -1
    empty.close()
    assert _kernel_launches(fx) == launched and pg.poses(stream=D.stream()).tobytes() == start
    fx._L.lfx_set_profiling(fx._ctx, 0)
    # a prior added: the per-prior figures are those of no optimise
    pg.add_priors(position, D.stream())
    for call in (lambda: pg.prior_chi2(stream=D.stream()), lambda: pg.edge_chi2(stream=D.stream())):
        with pytest.raises(B.LfxError) as err:
            call()
        assert err.value.code == -1
    again = pg.optimize(D.stream())
    assert again["code"] == first["code"] == R.CONVERGED and len(pg.prior_chi2(stream=D.stream())[0]) == 3
    pg.close()
    # an indefinite Omega shows as a chain pivot that is not positive: refused, the poses restored byte for byte
    neg = pose.copy()
    om = neg[0]["information"].reshape(6, 6).copy()
    om[4, 4] = -1e7
    neg[0]["information"] = om.reshape(36)
    pg = fx.pose_graph(12, 13)
    pg.add_nodes(g["poses"], D.stream())
    pg.add_edges(g["edges"], D.stream())
    pg.reserve_priors(1)
    pg.add_priors(neg, D.stream())
    res = pg.optimize(D.stream())
    print("a prior that is not positive definite: code %d, iterations %d, chi2 %.6e -> %.6e" % (res["code"], res["iterations"], res["chi2_initial"], res["chi2_final"]))
    assert res["code"] == R.NOT_POSITIVE_DEFINITE and pg.poses(stream=D.stream()).tobytes() == g["poses"].tobytes()
    assert res["chi2_final"] == res["chi2_initial"]
    pg.close()


@pytest.mark.gpu
def test_a_graph_without_priors_is_untouched_by_the_new_calls(fx):
    """release_first(0), a reserve that is never used and set_fixed(0, 0) leave a graph what it was: the same bytes as a graph
    that never heard of priors, node 0 where it stood."""
    g = K.step_shapes()[2]
    runs = []
    for touched in (False, True):
        pg = fx.pose_graph(len(g["poses"]), len(g["edges"]))
        pg.add_nodes(g["poses"], D.stream())
        if touched:
            pg.reserve_priors(8)
            pg.release_first(False, D.stream())
            pg.set_fixed(0, False, D.stream())
        pg.add_edges(g["edges"], D.stream())
        res = pg.optimize(D.stream())
        runs.append((pg.poses(stream=D.stream()).tobytes(), res, pg.edge_chi2(stream=D.stream())[0].tobytes()))
        assert pg.poses(0, 1, D.stream())[0].tobytes() == g["poses"][0].tobytes()
        pg.close()
    assert runs[0] == runs[1]
    # set_fixed(0, 1) holds a released first node; set_fixed(0, 0) lets it go again
    h = PK.shape("released_pose_prior_on_0")
    pg = build(fx, h, max_iter=1)
    pg.set_fixed(0, True, D.stream())
    pg.optimize(D.stream())
    assert pg.poses(0, 1, D.stream())[0].tobytes() == h["poses"][0].tobytes()
    pg.set_poses(h["poses"], 0, D.stream())
    pg.set_fixed(0, False, D.stream())
    pg.optimize(D.stream())
    want = PK.one_iteration(h["name"])[0]
    diff = float(np.abs(pg.poses(stream=D.stream()) - want).max())
    print("released, held by set_fixed(0, 1), let go again: device - restatement after one step %.3e" % diff)
    assert pg.poses(0, 1, D.stream())[0].tobytes() != h["poses"][0].tobytes() and diff <= 16.0 * K.floors()[0]
    pg.close()


@pytest.fixture(scope="module")
def hold():
    h = S.Hold()
    yield h
    for what, ms in h.issue_ms:
        print("held %.0f ms; issued %.3f ms after the hold was queued: %s" % (S.HOLD_MS, ms, what))


@pytest.mark.gpu
def test_optimize_waits_for_priors_and_the_release_on_another_stream(fx, hold):
    """The held-producer pattern of tests/test_pose_graph_streams_gpu.py, twice (a writing call waits on the host for the
    graph's last call, so one held call at a time): the priors are added on held stream A and optimise is issued on B while
    A has not run; then the start is written back, the first node is released on held A and optimise is issued on B again.
    Only the library's own wait can put either behind: the results must be those of the graphs built on one stream."""
    g = PK.shape("released_positions_only")
    wants = []
    for released in (False, True):
        pg = build(fx, dict(g, released=released))
        res = pg.optimize(D.stream())
        wants.append((res, pg.poses(stream=D.stream()).tobytes(), pg.prior_chi2(stream=D.stream())[0].tobytes()))
        pg.close()
    assert wants[0][1] != wants[1][1]
    pg = fx.pose_graph(len(g["poses"]), len(g["edges"]))
    pg.add_nodes(g["poses"], D.stream())
    pg.add_edges(g["edges"], D.stream())
    pg.reserve_priors(len(g["priors"]))
    a, b = S.two_streams()
    D.sync()
    hold(a)
    pg.add_priors(g["priors"], a.cuda_stream)
    e = S.event_behind(a)
    hold.still_held(e, "pose graph: add_priors on A, optimize on B")
    res = pg.optimize(b.cuda_stream)
    assert (res, pg.poses(stream=b.cuda_stream).tobytes(), pg.prior_chi2(stream=b.cuda_stream)[0].tobytes()) == wants[0]
    pg.set_poses(g["poses"], 0, D.stream())
    D.sync()
    hold(a)
    pg.release_first(True, a.cuda_stream)
    e = S.event_behind(a)
    hold.still_held(e, "pose graph: release_first on A, optimize on B")
    res = pg.optimize(b.cuda_stream)
    assert (res, pg.poses(stream=b.cuda_stream).tobytes(), pg.prior_chi2(stream=b.cuda_stream)[0].tobytes()) == wants[1]
    D.sync()
    pg.close()
