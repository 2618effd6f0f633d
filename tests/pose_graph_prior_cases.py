"""The graphs of the prior tests (tests/test_pose_graph_prior_expect.py on the host, tests/test_pose_graph_prior_gpu.py and
tests/test_pose_graph_prior_cpp_gpu.py on the device): graphs of tests/pose_graph_cases.py with priors on them, the anchored
form of each (the identity node first, the ids shifted by one, every prior an edge from the anchor), the linearisation case
and the drift case."""
import functools

import numpy as np

from tests import pose_graph_cases as K
from tests import pose_graph_prior_restatement as Q
from tests import pose_graph_restatement as R

PRIOR = np.dtype([("node", "<u4"), ("flags", "<u4"), ("z", "<f8", 12), ("information", "<f8", 36), ("lever", "<f8", 3)])
LEVER = (0.8, -0.2, 1.5)
IDENTITY = np.array(Q.IDENTITY)


def priors_of(rows):
    """rows: (node, flags, Z [3][4], Omega [6][6], lever [3])"""
    p = np.zeros(len(rows), PRIOR)
    for k, (node, flags, Z, om, lever) in enumerate(rows):
        p[k] = (node, flags, np.reshape(Z, 12), np.reshape(om, 36), np.asarray(lever, np.float64))
    return p


def information3(rng, sigma, full=True):
    """a symmetric positive definite 3 x 3 near I / sigma^2, every entry in use where `full`"""
    om = np.eye(3) / sigma ** 2
    if full:
        m = rng.standard_normal((3, 3))
        om = om + 0.2 * (m @ m.T) / sigma ** 2 / 3.0
    return 0.5 * (om + om.T)


def embed(om3):
    om = np.zeros((6, 6))
    om[3:, 3:] = om3
    return om


def pose_row(T, node, rng, noise=(0.002, 0.01), flags=0, angle=None, shift=(0.0, 0.0, 0.0), sigmas=None):
    """a pose prior on `node` whose pose is about T: Z = T with noise; angle: Z turned by that much about a random axis on
    top, so that the residual's rotation is that angle; shift: Z's translation moved (world frame)"""
    Z = K.perturb(T, rng, *noise)
    if angle is not None:
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        Z = T.copy()
        Z[:, :3] = T[:, :3] @ R.exp_rotation(angle * axis).T
    Z[:, 3] += np.asarray(shift, np.float64)
    return (node, flags, Z, K.information(rng, *(sigmas or noise)), (0.0, 0.0, 0.0))


def position_row(T, node, rng, lever=(0.0, 0.0, 0.0), sigma=0.05, flags=0, shift=(0.0, 0.0, 0.0), noise=None, full=True):
    """a position prior on `node` whose pose is about T: the antenna's place t + R l with noise (sigma unless given), moved by shift"""
    lever = np.asarray(lever, np.float64)
    Z = np.zeros((3, 4))
    Z[:, 3] = T[:, 3] + T[:, :3] @ lever + (sigma if noise is None else noise) * rng.standard_normal(3) + np.asarray(shift, np.float64)
    return (node, flags | Q.PRIOR_POSITION, Z, embed(information3(rng, sigma, full)), lever)


def with_priors(g, name, rows, released=False, **config):
    out = dict(g, name=name, priors=priors_of(rows), released=released)
    out.update(config)
    return out


def mixed_rows(g, nodes, rng):
    """a prior per node of `nodes`, the kinds in turn: pose, position with the lever, position without"""
    rows = []
    for n, k in enumerate(nodes):
        T = g["truth"][k]
        rows.append(pose_row(T, k, rng) if n % 3 == 0 else position_row(T, k, rng, LEVER if n % 3 == 1 else (0.0, 0.0, 0.0)))
    return rows


@functools.lru_cache(maxsize=None)
def step_shapes():
    """The shapes one Gauss-Newton step with priors is checked at (the issue's list), each a K.graph dict with priors,
    released and a name."""
    out = []
    rng = np.random.default_rng(600)
    g = K.graph(16, seed=60)
    out.append(with_priors(g, "one_prior", [pose_row(g["truth"][5], 5, rng)]))
    # 64 and 65 priors: the prior kernel's second workgroup of 64 holds none, then one
    g = K.graph(70, loops=[(3, 40)], seed=61)
    out.append(with_priors(g, "64_priors", mixed_rows(g, range(1, 65), rng)))
    out.append(with_priors(g, "65_priors", mixed_rows(g, range(1, 66), rng)))
    g = K.graph(12, loops=[(2, 9)], seed=62)
    T = g["truth"][4]
    out.append(with_priors(g, "three_mixed_on_one_node", [pose_row(T, 4, rng), position_row(T, 4, rng, LEVER),
                                                          position_row(T, 4, rng, flags=Q.PRIOR_ROBUST), pose_row(g["truth"][8], 8, rng)]))
    # a prior on a fixed node (7), on node 0 while it is fixed, on the last node
    g = K.graph(16, loops=[(1, 12)], fixed=(7,), seed=63)
    out.append(with_priors(g, "on_fixed_first_and_last", [pose_row(g["truth"][7], 7, rng, shift=(0.3, 0.0, 0.0)), position_row(g["truth"][0], 0, rng, LEVER, shift=(0.0, 0.2, 0.0)),
                                                          pose_row(g["truth"][15], 15, rng)]))
    # node 10 has no chain edge on either side and no loop: its prior alone holds it.  (The chain 11 .. 19 behind it hangs on
    # the loop (3, 14) alone, which is not in P: a pose prior on 17 holds P there.  With a position prior in its place P is
    # held by lambda along three directions of that chain, and woodbury - dense is 1.9e-7: the class of K.GAP_SHAPES.)
    g = K.graph(20, loops=[(3, 14)], missing=(9, 10), seed=64)
    out.append(with_priors(g, "prior_on_an_isolated_node", [pose_row(g["truth"][10], 10, rng), pose_row(g["truth"][17], 17, rng)]))
    g = K.graph(4, missing=(0, 1, 2), seed=65)
    out.append(with_priors(g, "four_nodes_no_edge", [pose_row(g["truth"][0], 0, rng), pose_row(g["truth"][1], 1, rng), pose_row(g["truth"][2], 2, rng),
                                                     position_row(g["truth"][2], 2, rng, LEVER), pose_row(g["truth"][3], 3, rng)]))
    # robust priors: s below huber_delta (w = 1), above it, and one 25 m off
    g = K.graph(24, loops=[(2, 15)], seed=66, start=(0.004, 0.01))
    S = g["poses"]
    out.append(with_priors(g, "robust_priors", [position_row(S[3], 3, rng, LEVER, flags=Q.PRIOR_ROBUST, noise=0.0, shift=(0.02, 0.0, 0.0), full=False),
                                                position_row(S[9], 9, rng, LEVER, flags=Q.PRIOR_ROBUST, noise=0.0, shift=(0.0, 0.4, 0.0), full=False),
                                                position_row(S[14], 14, rng, flags=Q.PRIOR_ROBUST, noise=0.0, shift=(25.0, 0.0, 0.0)),
                                                pose_row(S[20], 20, rng, noise=(0.0, 0.0), flags=Q.PRIOR_ROBUST, shift=(0.0, 0.0, 0.5), sigmas=(0.002, 0.01)),
                                                pose_row(g["truth"][22], 22, rng, flags=Q.PRIOR_ROBUST)]))
    g = K.graph(24, loops=[(20, 6)], seed=67)
    out.append(with_priors(g, "position_levers", [position_row(g["truth"][k], k, rng, LEVER if k % 2 else (0.0, 0.0, 0.0)) for k in range(2, 24, 3)]))
    g = [s for s in K.step_shapes() if s["name"] == "N65_chain_31_32_missing_bridged"][0]
    out.append(with_priors(g, "N65_gap_prior_every_8th", mixed_rows(g, range(0, 65, 8), rng)))
    # the first node released
    g = K.graph(16, loops=[(2, 12)], seed=68)
    out.append(with_priors(g, "released_pose_prior_on_0", [pose_row(g["truth"][0], 0, rng), position_row(g["truth"][11], 11, rng, LEVER)], released=True))
    g = K.graph(24, seed=69)                                   # (K.trajectory turns about every axis: not a line)
    out.append(with_priors(g, "released_positions_only", [position_row(g["truth"][k], k, rng, LEVER) for k in range(0, 24, 4)], released=True))
    g = [s for s in K.step_shapes() if s["name"] == "257_nodes_257_edges"][0]
    out.append(with_priors(g, "released_257_a_fix_per_node", [position_row(g["truth"][k], k, rng, LEVER) for k in range(257)], released=True))
    for s in out:
        s.setdefault("huber_delta", 3.0)
        s.setdefault("damping", 1e-6)
    return out


ROBUST_INSIDE, ROBUST_BEYOND, ROBUST_FAR = 0, 1, 2          # priors of the shape robust_priors


def shape(name):
    return [g for g in step_shapes() if g["name"] == name][0]


def config_of(g):
    return dict(damping=g.get("damping", 1e-6), huber_delta=g.get("huber_delta", 3.0))


def linearisation_case():
    """8 nodes, the chain's edges, 14 priors: pose priors with residual rotations of 0 (Z is the pose itself), 1e-5, 1e-3, 1
    and 2.5 rad, robust ones on both sides of huber_delta and one 25 m off, position priors without and with the lever and
    with a full Omega_t, three priors on node 6, one on the fixed node 0."""
    rng = np.random.default_rng(177)
    poses = np.array([K.pose(rng.standard_normal(3), 5 * rng.standard_normal(3)) for _ in range(8)])
    erows = [(i, i + 1, K.perturb(K.between(poses[i], poses[i + 1]), rng, 0.01, 0.05), K.information(rng, 0.05, 0.1), 0) for i in range(7)]
    rows = [(1, 0, poses[1].copy(), K.information(rng, 0.05, 0.1), (0.0, 0.0, 0.0))]
    for node, angle in ((2, 1e-5), (3, 1e-3), (4, 1.0), (5, 2.5)):
        rows.append(pose_row(poses[node], node, rng, noise=(0.05, 0.1), angle=angle, shift=0.1 * rng.standard_normal(3)))
    rows += [pose_row(poses[6], 6, rng, noise=(0.05, 0.1), flags=Q.PRIOR_ROBUST, angle=0.02, shift=(0.05, 0.0, 0.0)),      # s below 3
             pose_row(poses[6], 6, rng, noise=(0.05, 0.1), flags=Q.PRIOR_ROBUST, angle=1.5, shift=(2.0, 0.0, 0.0)),       # far above
             position_row(poses[6], 6, rng, LEVER, flags=Q.PRIOR_ROBUST, shift=(25.0, 0.0, 0.0)),
             position_row(poses[7], 7, rng, noise=0.04, flags=Q.PRIOR_ROBUST),
             position_row(poses[7], 7, rng), position_row(poses[2], 2, rng, LEVER), position_row(poses[3], 3, rng, LEVER, full=False),
             position_row(poses[0], 0, rng, LEVER), pose_row(poses[0], 0, rng)]
    return dict(poses=poses, edges=K.edges_of(erows), priors=priors_of(rows), fixed=(), released=False, name="prior_linearisation")


def anchored(g):
    """The graph g with its priors as edges: the identity node first (node 0: the old functions fix it), every id shifted by
    one, prior p the edge (0, node + 1, Z, Omega).  Only for pose priors and position priors with a zero lever: such a
    position prior is the edge with R_Z = I and Omega = blkdiag(0, Omega_t).  The old first node (now 1) is fixed unless g
    released it.  (poses, edges, fixed)"""
    rows = [(int(e["i"]) + 1, int(e["j"]) + 1, np.reshape(e["z"], (3, 4)), np.reshape(e["information"], (6, 6)), int(e["flags"])) for e in g["edges"]]
    for p in g["priors"]:
        flags = int(p["flags"])
        Z = np.reshape(p["z"], (3, 4)).copy()
        if flags & Q.PRIOR_POSITION:
            assert not np.any(p["lever"])
            Z[:, :3] = np.eye(3)
        rows.append((0, int(p["node"]) + 1, Z, np.reshape(p["information"], (6, 6)), R.ROBUST if flags & Q.PRIOR_ROBUST else 0))
    poses = np.concatenate([IDENTITY[None], np.asarray(g["poses"]).reshape(-1, 3, 4)])
    fixed = tuple(int(k) + 1 for k in g["fixed"]) + (() if g["released"] else (1,))
    return poses, K.edges_of(rows), fixed


def without_levers(g):
    """g with every position prior's lever removed and its fix moved to the node's own origin (by the lever at the true
    pose): what has an anchored form"""
    p = g["priors"].copy()
    for k in range(len(p)):
        if np.any(p[k]["lever"]):
            z = p[k]["z"].copy()
            z[[3, 7, 11]] -= g["truth"][int(p[k]["node"])][:, :3] @ p[k]["lever"]
            p[k]["z"] = z
    p["lever"] = 0.0
    return dict(g, priors=p)


@functools.lru_cache(maxsize=None)
def dense_first_steps():
    """name -> (delta of the first dense step with priors, its linearisation), each shape under its own config"""
    return {g["name"]: Q.dense_step(g["poses"], g["edges"], g["priors"], g["fixed"], g["released"], **config_of(g)) for g in step_shapes()}


@functools.lru_cache(maxsize=None)
def differences():
    """name -> the shape's own woodbury_step - dense_step with priors"""
    seen = {}
    for g in step_shapes():
        dense, lin = dense_first_steps()[g["name"]]
        seen[g["name"]] = float(np.abs(Q.woodbury_step(g["poses"], g["edges"], g["priors"], g["fixed"], g["released"], lin=lin, **config_of(g)) - dense).max())
    return seen


@functools.lru_cache(maxsize=None)
def one_iteration(name):
    g = shape(name)
    return Q.optimize(g["poses"], g["edges"], g["priors"], g["fixed"], g["released"], max_iter=1, **config_of(g))


# --- the drift case ----------------------------------------------------------------------------------------------------------------
DRIFT_SEED = 11
DRIFT_OUTLIER = 9            # the prior (of 16) that is 25 m off
DRIFT_CONFIG = dict(max_iter=20)


@functools.lru_cache(maxsize=None)
def drift_case(seed=DRIFT_SEED):
    """An open chain of 256 nodes that drifts (K.circle without its loops: two laps, the start chained from the noisy
    odometry), a robust position fix with the lever arm on every 16th node, the one on node 144 25 m off; the first node
    released."""
    g = K.circle(256, 0, seed)
    rng = np.random.default_rng(1000 + seed)
    rows = []
    for n, k in enumerate(range(0, 256, 16)):
        rows.append(position_row(g["truth"][k], k, rng, LEVER, sigma=0.05, noise=0.03, flags=Q.PRIOR_ROBUST,
                                 shift=(25.0, 0.0, 0.0) if n == DRIFT_OUTLIER else (0.0, 0.0, 0.0), full=False))
    return with_priors(g, "drift_256", rows, released=True)


@functools.lru_cache(maxsize=None)
def drift_result():
    g = drift_case()
    return Q.optimize(g["poses"], g["edges"], g["priors"], g["fixed"], True, **DRIFT_CONFIG)
