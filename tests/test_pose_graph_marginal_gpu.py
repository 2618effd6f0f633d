"""The covariances of optimised pose-graph nodes on the device (lfx_pose_graph_reserve_marginals, _marginals,
_joint_covariances, _relative_covariance) against the definition (tests/pose_graph_marginal_restatement.py; the graphs, the
pairs and the tolerance: tests/pose_graph_marginal_cases.py).

Against the definition: the device's final poses are read back and the 50-digit reference is built at those poses; every
diagonal block and every asked cross block within C * MARGIN * eps * kappa_2(H) * max |Sigma| of it, C and MARGIN from the
cases file (measured on the host alone), kappa_2 from the reference at those poses.  Then what must hold exactly: symmetry,
zeros, transposes, bytes; determinism over ranges, calls, splits and streams; that nothing the solver computes changes;
refusals; and what the numbers mean.  Every test prints its figures before it asserts."""
import numpy as np
import pytest

from lidar_feature_extraction_amd import binding as B
from lidar_feature_extraction_amd import relative_covariance
from tests import deskew_cases as D
from tests import pose_graph_cases as K
from tests import pose_graph_marginal_cases as MC
from tests import pose_graph_marginal_restatement as M
from tests import pose_graph_restatement as R

NAMES = [c["name"] for c in MC.cases()]


@pytest.fixture(scope="module")
def fx():
    f = D.fx_for(16, 900, 1)
    yield f
    f.close()


def build(fx, c, calls=1, reserve=True, extra_nodes=0, extra_edges=0, **config):
    """The case c on the device: nodes, fixed flags, the release, the reserves, priors, then the edges in `calls` calls"""
    n, e, p = len(c["poses"]), c["edges"], c["priors"]
    cfg = dict(damping=c["damping"], huber_delta=c["huber_delta"], max_iter=20)
    cfg.update(config)
    pg = fx.pose_graph(n + extra_nodes, max(len(e) + extra_edges, 1), **cfg)
    assert pg.add_nodes(c["poses"], D.stream()) == 0
    for k in c["fixed"]:
        pg.set_fixed(k, True, D.stream())
    if c["released"]:
        pg.release_first(True, D.stream())
    if len(p):
        pg.reserve_priors(len(p))
        pg.add_priors(p, D.stream())
    if reserve:
        pg.reserve_marginals()
    cuts = [len(e) * k // calls for k in range(calls + 1)]
    for k in range(calls):
        pg.add_edges(e[cuts[k]:cuts[k + 1]], D.stream())
    return pg


_runs = {}


def run(fx, name):
    """The case optimised on the device, once: its final poses, every marginal, the joint blocks of its pairs, and the
    50-digit reference at those poses"""
    if name not in _runs:
        c = MC.case(name)
        pg = build(fx, c)
        res = pg.optimize(D.stream())
        assert res["code"] in (R.CONVERGED, R.MAX_ITERATIONS), res
        poses = pg.poses(stream=D.stream())
        cov = pg.marginals(stream=D.stream())
        pairs = np.array(c["pairs"], np.uint32).reshape(-1, 2)
        joints = pg.joint_covariances(pairs, stream=D.stream())
        assert pg.poses(stream=D.stream()).tobytes() == poses.tobytes()      # the poses are never touched
        pg.close()
        _runs[name] = dict(case=c, poses=poses, cov=cov, pairs=pairs, joints=joints, ref=MC.reference_blocks(c, poses), result=res)
    return _runs[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_against_the_definition(fx, name):
    r = run(fx, name)
    diag, cross, kappa, top = r["ref"]
    tol = MC.bound(name, r["ref"])
    cross_got = {tuple(int(v) for v in p): r["joints"][k][:6, 6:] for k, p in enumerate(r["pairs"])}
    err_d = float(np.abs(r["cov"] - diag).max())
    err_x = max([0.0] + [float(np.abs(cross_got[p] - cross[p]).max()) for p in cross])
    print("%s: kappa_2 %.3e, max |Sigma| %.3e, tolerance %.3e (C %.3g x %g): marginals off by %.3e, cross blocks by %.3e = %.3g eps kappa max|Sigma|" % (
        name, kappa, top, tol, MC.c_of(name), MC.MARGIN, err_d, err_x, max(err_d, err_x) / (MC.EPS * kappa * top)))
    assert kappa <= MC.CAP
    assert err_d <= tol and err_x <= tol


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_exact_structure(fx, name):
    r = run(fx, name)
    c, cov, joints = r["case"], r["cov"], r["joints"]
    fixed = M.system(r["poses"], c["edges"], c["priors"], c["fixed"], c["released"])["fixed"]
    assert cov.tobytes() == np.ascontiguousarray(cov.transpose(0, 2, 1)).tobytes(), "a marginal that is not symmetric bit for bit"
    for k in range(len(cov)):
        assert (k in fixed) == (not cov[k].any())
        assert k in fixed or (np.diag(cov[k]) > 0.0).all()
    for k, (i, j) in enumerate(r["pairs"]):
        J = joints[k]
        assert J.tobytes() == np.ascontiguousarray(J.T).tobytes(), "Sigma_ji is not the transpose of Sigma_ij"
        assert J[:6, :6].tobytes() == cov[i].tobytes() and J[6:, 6:].tobytes() == cov[j].tobytes()
        if int(i) in fixed or int(j) in fixed:
            assert not J[:6, 6:].any()
    # the same pair in the other order is the same block transposed
    seen = {(int(i), int(j)): joints[k] for k, (i, j) in enumerate(r["pairs"])}
    swapped = [(i, j) for (i, j) in seen if (j, i) in seen]
    for (i, j) in swapped:
        assert seen[(i, j)][:6, 6:].tobytes() == np.ascontiguousarray(seen[(j, i)][6:, :6]).tobytes()
    print("%s: %d marginals, %d pairs (%d in both orders), fixed %s" % (name, len(cov), len(seen), len(swapped) // 2, sorted(fixed)))


@pytest.mark.gpu
def test_determinism_over_ranges_calls_splits_and_streams(fx):
    import torch
    name = "N65_L9"
    r = run(fx, name)
    c = r["case"]
    pg = build(fx, c, calls=3)                     # the edges split over three calls: the chain / loop split is the same
    pg.optimize(D.stream())
    assert pg.poses(stream=D.stream()).tobytes() == r["poses"].tobytes()
    other = torch.cuda.Stream()
    one_by_one = np.array([pg.marginals(k, 1, stream=other.cuda_stream)[0] for k in range(len(c["poses"]))])   # the work runs on another stream
    assert one_by_one.tobytes() == r["cov"].tobytes()
    assert pg.marginals(stream=D.stream()).tobytes() == r["cov"].tobytes()
    assert pg.marginals(7, 20, stream=D.stream()).tobytes() == r["cov"][7:27].tobytes()
    assert pg.joint_covariances(r["pairs"], stream=other.cuda_stream).tobytes() == r["joints"].tobytes()
    assert pg.joint_covariances(r["pairs"][2:3], stream=D.stream()).tobytes() == r["joints"][2:3].tobytes()
    # more pairs than one launch takes, the joint blocks asked before the marginals
    pg.set_poses(r["poses"][:1], 0, D.stream())
    with pytest.raises(B.LfxError):
        pg.marginals(stream=D.stream())
    pg.optimize(D.stream())
    many = np.array([(i, j) for i in range(1, 14) for j in range(20, 30)], np.uint32)
    got = pg.joint_covariances(many, stream=D.stream())
    again = pg.joint_covariances(many[::-1].copy(), stream=D.stream())[::-1]
    assert len(many) > 64 and got.tobytes() == np.ascontiguousarray(again).tobytes()
    cov = pg.marginals(stream=D.stream())
    assert got[:, :6, :6].tobytes() == np.ascontiguousarray(cov[many[:, 0]]).tobytes()
    pg.close()


@pytest.mark.gpu
def test_no_trespass_on_the_solver(fx):
    c = MC.case("N12_L9")
    last_pose, last_edge = K.compose(c["poses"][11], K.pose([0.0, 0.0, 0.1], [1.0, 0.0, 0.0])), c["edges"][10:11].copy()
    last_edge["i"], last_edge["j"] = 11, 12        # the chain edge 10 -> 11 once more, one node on
    out = []
    for with_marginals in (False, True):
        pg = build(fx, c, reserve=with_marginals, extra_nodes=1, extra_edges=1)
        pg.optimize(D.stream())
        if with_marginals:
            pg.marginals(stream=D.stream())
            pg.joint_covariances([(1, 9)], stream=D.stream())
        pg.add_nodes([last_pose], D.stream())
        pg.add_edges(last_edge, D.stream())
        res = pg.optimize(D.stream())
        out.append((pg.poses(stream=D.stream()), res, pg.edge_chi2(stream=D.stream())))
        pg.close()
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1] == out[1][1]
    assert out[0][2][0].tobytes() == out[1][2][0].tobytes()
    # a graph that never reserves holds what it always did; the reserve is what grows it, by what the header states
    plain, reserved = build(fx, c, reserve=False), build(fx, c, reserve=False)
    before = plain.info()["device_bytes"]
    assert reserved.info()["device_bytes"] == before
    reserved.reserve_marginals()
    grown = reserved.info()["device_bytes"] - before
    print("device_bytes %d without the reserve, %d more with it" % (before, grown))
    assert grown == 8 * (3 * 36 * len(c["poses"]) + 36 * 64) + 4 * (2 * 64 + 1) and plain.info()["device_bytes"] == before
    plain.close()
    reserved.close()


@pytest.mark.gpu
def test_refusals(fx):
    c = MC.case("N12_L1")
    pg = build(fx, c, reserve=False, extra_nodes=1, extra_edges=1)
    pg.reserve_priors(1)
    pg.optimize(D.stream())

    def refused(call):
        with pytest.raises(B.LfxError) as e:
            call()
        assert e.value.code == B.ERR_INVALID_ARGUMENT
    refused(lambda: pg.marginals(stream=D.stream()))                    # before the reserve
    refused(lambda: pg.joint_covariances([(1, 2)], stream=D.stream()))
    pg.reserve_marginals()
    refused(pg.reserve_marginals)                                       # a second reserve
    assert pg.marginals(stream=D.stream()).shape == (12, 6, 6)
    refused(lambda: pg.marginals(5, 8, stream=D.stream()))              # a range past the nodes
    refused(lambda: pg.marginals(13, 0, stream=D.stream()))
    sentinel = np.full((2, 12, 12), -7.0)
    refused(lambda: pg.joint_covariances([(1, 2), (3, 3)], stream=D.stream(), out=sentinel))     # i == j: nothing written
    refused(lambda: pg.joint_covariances([(1, 2), (3, 12)], stream=D.stream(), out=sentinel))    # not a node
    assert (sentinel == -7.0).all()
    z, om = np.reshape(c["edges"][0]["z"], (3, 4)), np.reshape(c["edges"][0]["information"], (6, 6))
    writes = [("set_poses", lambda: pg.set_poses(c["poses"][3:4], 3, D.stream())),
              ("set_fixed", lambda: pg.set_fixed(5, True, D.stream())),
              ("release_first", lambda: pg.release_first(False, D.stream())),
              ("add_priors", lambda: pg.add_prior(4, c["poses"][4], om, stream=D.stream())),
              ("add_edges", lambda: pg.add_edge(2, 7, K.between(c["poses"][2], c["poses"][7]), om, stream=D.stream())),
              ("add_nodes", lambda: pg.add_nodes([K.compose(c["poses"][11], z)], D.stream()))]
    for what, write in writes:                                          # after each kind of write, until the next optimise
        assert pg.optimize(D.stream())["code"] in (R.CONVERGED, R.MAX_ITERATIONS)
        pg.marginals(stream=D.stream())
        write()
        refused(lambda: pg.marginals(stream=D.stream()))
        refused(lambda: pg.joint_covariances([(1, 2)], stream=D.stream()))
        print("refused after", what)
    pg.close()
    fresh = build(fx, c)
    refused(lambda: fresh.marginals(stream=D.stream()))                 # before the first optimise
    fresh.close()
    # damping 0 and a node nothing holds: no covariance, and the caller's array as it was
    iso = MC.case("isolated_last_node")
    pg = build(fx, iso, damping=0.0)
    assert pg.optimize(D.stream())["code"] == R.NOT_POSITIVE_DEFINITE
    sentinel = np.full((20, 6, 6), -7.0)
    _, code = pg.marginals(stream=D.stream(), out=sentinel, return_code=True)
    assert code == B.POSE_GRAPH_NOT_POSITIVE_DEFINITE and (sentinel == -7.0).all()
    sentinel = np.full((1, 12, 12), -7.0)
    _, code = pg.joint_covariances([(1, 2)], stream=D.stream(), out=sentinel, return_code=True)
    assert code == B.POSE_GRAPH_NOT_POSITIVE_DEFINITE and (sentinel == -7.0).all()
    with pytest.raises(B.LfxError):
        pg.marginals(stream=D.stream())
    pg.close()


@pytest.mark.gpu
def test_what_the_numbers_mean(fx):
    # Two laps of a circle.  Along the open chain a node's covariance is the one before it carried over by a map of
    # determinant 1 plus the edge's own: det Sigma_kk grows at every node (Minkowski), the whole chain long.  The TRACE of the
    # position block grows along the first lap, and every node of the second lap has more than the node one lap before it --
    # but not at every step of the second lap: most of a position's variance here is an earlier heading error times the
    # distance from where it was made (0.002 rad x 40 m against 0.01 m), and on the way back to the start that distance
    # shrinks (the definition on the host shows the same: the trace falls at node 62 of 64).
    # The closures can only add information: with them the trace is smaller at every node.  To compare the two graphs at
    # ONE linearisation the closures here measure what the start poses say, so the start is the optimum of both; next to the
    # fixed node the gain is far below the rounding of either number, so "smaller" there is "not larger by more than the two
    # numbers' own bounds", and at the closed nodes of the second lap it is "less than half".
    n, half = 64, 32
    open_chain, closed = K.circle(n, 0, 11), K.circle(n, 4, 11)
    assert open_chain["poses"].tobytes() == closed["poses"].tobytes()
    for e in range(n - 1, n + 3):
        i, j = int(closed["edges"][e]["i"]), int(closed["edges"][e]["j"])
        closed["edges"][e]["z"] = K.between(closed["poses"][i], closed["poses"][j]).reshape(12)
    traces, logdets, tols = [], [], []
    for g in (open_chain, closed):
        c = MC.as_case(g["name"], g)
        pg = build(fx, c)
        assert pg.optimize(D.stream())["code"] == R.CONVERGED
        assert np.abs(pg.poses(stream=D.stream()) - g["poses"]).max() <= 1e-9
        cov = pg.marginals(stream=D.stream())
        traces.append(np.trace(cov[:, 3:, 3:], axis1=1, axis2=2))
        logdets.append(np.array([np.linalg.slogdet(b)[1] for b in cov[1:]]))
        tols.append(3.0 * MC.bound(g["name"], (None, None, M.condition(MC.system_of(c)), float(np.abs(cov).max()))))   # (a trace: three entries)
        pg.close()
    loop_ends = [int(closed["edges"][e]["j"]) for e in range(n - 1, n + 3)]
    print("trace of the position covariance, open chain: %s ...; with 4 closures: %s ...; bounds %.3e, %.3e" % (
        np.round(traces[0][:4], 6), np.round(traces[1][:4], 6), tols[0], tols[1]))
    print("open chain: the trace falls at nodes %s; at the closed nodes %s it is %s without and %s with the closures" % (
        np.where(np.diff(traces[0]) <= 0.0)[0] + 1, loop_ends, np.round(traces[0][loop_ends], 4), np.round(traces[1][loop_ends], 4)))
    assert traces[0][0] == 0.0 and (np.diff(logdets[0]) > 0.0).all()
    assert (np.diff(traces[0][:half + 1]) > 0.0).all() and (traces[0][half:] > traces[0][:half]).all()
    assert (traces[1] <= traces[0] + (tols[0] + tols[1])).all()
    assert (traces[1][loop_ends] < 0.5 * traces[0][loop_ends]).all()
    # two nodes, one edge, lambda = 0: the residual's covariance is the edge's Omega inverted (exact algebra: at the optimum
    # the residual is 0, where relative_covariance takes its Jacobians)
    c = MC.case("N2_L0")
    pg = build(fx, c, damping=0.0)
    assert pg.optimize(D.stream())["code"] == R.CONVERGED
    poses = pg.poses(stream=D.stream())
    joint = pg.joint_covariances([(0, 1)], stream=D.stream())[0]
    pg.close()
    rel = relative_covariance(poses[0], poses[1], joint)
    omega = np.reshape(c["edges"][0]["information"], (6, 6))
    want = np.linalg.inv(omega)
    ref = MC.reference_blocks(dict(c, damping=0.0, pairs=()), poses)
    # the marginal's own bound carried through A_j (rows of at most two entries of size <= 1: a factor 4), and the rounding of
    # the two products of twelve terms over entries of that size
    tol = 4.0 * MC.bound("N2_L0", ref) + 64.0 * np.spacing(ref[3]) + 16.0 * MC.EPS * np.linalg.cond(omega) * np.abs(want).max()
    print("relative covariance of the pair - Omega^-1: %.3e, tolerance %.3e" % (np.abs(rel - want).max(), tol))
    assert np.abs(rel - want).max() <= tol
    assert rel.tobytes() == np.ascontiguousarray(rel.T).tobytes()
