"""The graphs of the pose-graph tests (tests/test_pose_graph_expect.py on the host, tests/test_pose_graph_gpu.py,
tests/test_pose_graph_streams_gpu.py and tests/test_pose_graph_cpp_gpu.py on the device): generators, the list of one-step
shapes and the measured floor between the two ways to one step, the extra shapes with a config of their own, the stages of
the graph that grows, and the 50-digit reference of the residual (tests/golden/pose_graph_residual_reference.json)."""
import functools
import json
import os

import numpy as np

from tests import pose_graph_restatement as R

EDGE = np.dtype([("i", "<u4"), ("j", "<u4"), ("flags", "<u4"), ("reserved", "<u4"), ("z", "<f8", 12), ("information", "<f8", 36)])
PANEL = 48            # lfx::kPgPanel: the S factor's panel width


def pose(rotvec, t):
    T = np.zeros((3, 4))
    T[:, :3] = R.exp_rotation(rotvec)
    T[:, 3] = t
    return T


def between(Ta, Tb):
    """Ta^-1 Tb"""
    Z = np.zeros((3, 4))
    Z[:, :3] = Ta[:, :3].T @ Tb[:, :3]
    Z[:, 3] = Ta[:, :3].T @ (Tb[:, 3] - Ta[:, 3])
    return Z


def compose(Ta, Z):
    T = np.zeros((3, 4))
    T[:, :3] = Ta[:, :3] @ Z[:, :3]
    T[:, 3] = Ta[:, :3] @ Z[:, 3] + Ta[:, 3]
    return T


def perturb(T, rng, rot, trans):
    return compose(T, pose(rot * rng.standard_normal(3), trans * rng.standard_normal(3)))


def edges_of(rows):
    """rows: (i, j, Z [3][4], Omega [6][6], flags)"""
    e = np.zeros(len(rows), EDGE)
    for k, (i, j, Z, om, flags) in enumerate(rows):
        e[k] = (i, j, flags, 0, np.reshape(Z, 12), np.reshape(om, 36))
    return e


def information(rng, sigma_rot, sigma_t, full=True):
    """a symmetric positive definite matrix near diag(1 / sigma^2), with every entry in use where `full`"""
    om = np.diag([1.0 / sigma_rot ** 2] * 3 + [1.0 / sigma_t ** 2] * 3)
    if full:
        m = rng.standard_normal((6, 6))
        s = np.sqrt(np.diag(om))
        om = om + 0.05 * (m @ m.T) * np.outer(s, s) / 6.0
    return 0.5 * (om + om.T)


def trajectory(N, rng):
    """N poses along a rising curve, turning about every axis"""
    out = [pose(0.3 * rng.standard_normal(3), rng.standard_normal(3))]
    for _ in range(N - 1):
        out.append(compose(out[-1], pose(np.array([0.02, -0.03, 0.12]) + 0.02 * rng.standard_normal(3), np.array([1.0, 0.05, 0.02]))))
    return np.array(out)


def graph(N, loops=(), seed=0, missing=(), fixed=(), duplicate=(), start=(0.02, 0.05), noise=(0.002, 0.01)):
    """A chain of N nodes with its edges i -> i + 1 (those starting at `missing` left out), then the `loops` (i, j), then a
    second edge for every pair of `duplicate`; measurements with noise; the start is the truth perturbed per node."""
    rng = np.random.default_rng(seed)
    truth = trajectory(N, rng)
    rows = []
    for i, j in [(i, i + 1) for i in range(N - 1) if i not in missing] + list(loops) + list(duplicate):
        rows.append((i, j, perturb(between(truth[i], truth[j]), rng, *noise), information(rng, *noise), 0))
    first = np.array([truth[0]] + [perturb(truth[k], rng, *start) for k in range(1, N)])
    return dict(poses=first, truth=truth, edges=edges_of(rows), fixed=tuple(fixed), name="")


def step_shapes():
    """The shapes one Gauss-Newton step is checked at (every path of the solver), each a graph() dict with a name."""
    out = []

    def add(name, **kw):
        g = graph(**kw)
        g["name"] = name
        out.append(g)

    add("N2_L0", N=2, seed=1)
    add("N3_L1", N=3, loops=[(0, 2)], seed=2)
    add("N64_L3", N=64, loops=[(3, 40), (10, 63), (50, 20)], seed=3)
    add("N65_chain_31_32_missing_bridged", N=65, loops=[(30, 33), (5, 60)], missing=(31,), seed=4)
    add("N16_L0_perturbed", N=16, seed=5, start=(0.1, 0.5))
    add("loop_at_node_0", N=32, loops=[(0, 20), (31, 0)], seed=6)
    add("second_fixed_node_32", N=64, loops=[(3, 40), (10, 63), (31, 33), (32, 50)], fixed=(32,), seed=7)
    add("two_edges_on_one_pair", N=16, loops=[(2, 12)], duplicate=[(3, 4), (2, 12), (12, 2)], seed=8)
    for L in (PANEL // 6 - 1, PANEL // 6, PANEL // 6 + 1, 2 * PANEL // 6):     # 6 L = 42, 48, 54, 96
        rng = np.random.default_rng(100 + L)
        add("S_of_%d_rows" % (6 * L), N=40, loops=[tuple(int(v) for v in rng.choice(40, 2, replace=False)) for _ in range(L)], seed=9 + L)
    # 6 L + 1 = 193 columns: the chain solve's fourth workgroup of 64 holds one; 257 nodes and 257 edges: the reductions'
    # second pass of 256 and the linearisation's fifth workgroup of 64 hold one
    rng = np.random.default_rng(300)
    add("193_columns", N=80, loops=[tuple(int(v) for v in rng.choice(80, 2, replace=False)) for _ in range(32)], seed=30)
    add("257_nodes_257_edges", N=257, loops=[(5, 250)], seed=31)
    # 6 L = 336: S's assembly has a second workgroup of 256 columns, the first panel 288 rows below it (a second workgroup
    # of rows), the update 18 x 18 tiles, the solve six blocks of 64 with a partial last one
    rng = np.random.default_rng(301)
    add("S_of_336_rows", N=120, loops=[tuple(int(v) for v in rng.choice(120, 2, replace=False)) for _ in range(56)], seed=32)
    return out


def remeasure(g, e, flags=0, shift=(0.0, 0.0, 0.0), from_start=False):
    """Edge e of the graph g given `flags` and its measured translation moved by `shift` (metres, in the frame of node i).
    from_start: the measurement is first replaced by the one the START poses agree with, so that the edge's residual at the
    start is the shift alone: s = sqrt(r^T Omega r) is then chosen, not met."""
    ed = g["edges"][e]
    Z = between(g["poses"][int(ed["i"])], g["poses"][int(ed["j"])]) if from_start else np.reshape(ed["z"], (3, 4)).copy()
    Z[:, 3] += np.asarray(shift, np.float64)
    g["edges"][e]["z"] = Z.reshape(12)
    g["edges"][e]["flags"] = flags


def robust_chain_graph(name, fixed=(), huber_delta=3.0):
    """24 nodes, a whole chain (edge k is k -> k + 1), loops (2, 15) = edge 23 and (20, 6) = edge 24.  Robust and 1 m, 0.7 m
    and 1 m off: the adjacent chain edges 7 and 8 and loop edge 23 (sigma_t = 0.01 m: s of 70 .. 100).  Robust and measured
    from the start: chain edge 12, 1 mm off (s about 0.1: w = 1 under every huber_delta used), and chain edge 16, 15 mm off
    (s about 1.5: w = 1 under huber_delta = 3, below 1 under 0.5)."""
    g = graph(24, loops=[(2, 15), (20, 6)], seed=50, fixed=fixed, start=(0.004, 0.01))
    remeasure(g, 7, R.ROBUST, (1.0, 0.0, 0.0))
    remeasure(g, 8, R.ROBUST, (0.0, 0.7, 0.0))
    remeasure(g, 23, R.ROBUST, (0.0, 0.0, 1.0))
    remeasure(g, 12, R.ROBUST, (0.001, 0.0, 0.0), from_start=True)
    remeasure(g, 16, R.ROBUST, (0.015, 0.0, 0.0), from_start=True)
    g.update(name=name, huber_delta=huber_delta)
    return g


ROBUST_OUTLIERS, ROBUST_INLIER, ROBUST_BETWEEN = (7, 8, 23), 12, 16       # edges of robust_chain_graph()
DAMPINGS = (("damping_0", 0.0), ("damping_1e-2", 1e-2), ("damping_10", 10.0))


def damping_graph():
    """24 nodes, a whole chain, two loops, a start half a metre off: the one graph the dampings are run at"""
    return graph(24, loops=[(2, 15), (20, 6)], seed=51, start=(0.1, 0.5))


@functools.lru_cache(maxsize=None)
def extra_step_shapes():
    """More one-step shapes, each with its own config (huber_delta, damping) and fixed nodes: down-weighted CHAIN edges, a
    second huber_delta, three dampings, a last node without an edge.  A list of its own: floor() takes its maximum over
    step_shapes() and the circles, and these are held to that floor, which they must not move
    (tests/test_pose_graph_expect.py asserts that each shape's own difference lies below it)."""
    out = [robust_chain_graph("robust_chain_pair"), robust_chain_graph("robust_chain_beside_fixed", fixed=(9,)),
           robust_chain_graph("huber_half", huber_delta=0.5)]
    for name, damping in DAMPINGS:
        out.append(dict(damping_graph(), name=name, damping=damping))
    # the chain edge 18 -> 19 is missing and no loop touches node 19: P's last block is lambda I, the gradient there is 0
    out.append(dict(graph(20, loops=[(3, 14), (16, 5)], missing=(18,), seed=52), name="dangling_last_node"))
    for g in out:
        g.setdefault("huber_delta", 3.0)
        g.setdefault("damping", 1e-6)
    return out


def config_of(g):
    """the solver's config of a shape (the defaults where it has none of its own)"""
    return dict(damping=g.get("damping", 1e-6), huber_delta=g.get("huber_delta", 3.0))


@functools.lru_cache(maxsize=None)
def extra_first_steps():
    """name -> (delta of the first dense step, its linearisation), each extra shape under its own config"""
    return {g["name"]: R.dense_step(g["poses"], g["edges"], g["fixed"], **config_of(g)) for g in extra_step_shapes()}


@functools.lru_cache(maxsize=None)
def extra_differences():
    """name -> the shape's own woodbury_step - dense_step, under its own config"""
    seen = {}
    for g in extra_step_shapes():
        dense, lin = extra_first_steps()[g["name"]]
        seen[g["name"]] = float(np.abs(R.woodbury_step(g["poses"], g["edges"], g["fixed"], lin=lin, **config_of(g)) - dense).max())
    return seen


def all_step_shapes():
    return {g["name"]: g for g in step_shapes() + list(extra_step_shapes())}


@functools.lru_cache(maxsize=None)
def one_iteration(name):
    """The restatement's (poses, result, (rho, w)) after ONE iteration of the shape `name` (old or extra) under its config:
    what the device's code and n_robust_downweighted of a max_iter = 1 run are held to."""
    g = all_step_shapes()[name]
    return R.optimize(g["poses"], g["edges"], g["fixed"], max_iter=1, **config_of(g))


def robust_s(edges, rho, w, huber_delta):
    """s = sqrt(r^T Omega r) of the robust edges, from what lfx_pose_graph_edge_chi2 reports: sqrt(rho) where w = 1,
    huber_delta / w beyond"""
    rho, w = np.asarray(rho), np.asarray(w)
    s = np.where(w < 1.0, huber_delta / np.where(w < 1.0, w, 1.0), np.sqrt(np.maximum(rho, 0.0)))
    return s[(edges["flags"] & R.ROBUST) != 0]


def growth_graph():
    """The 48-node graph of the growth test (tests/test_pose_graph_gpu.py grows it in four stages): every chain edge, three
    loops of which (25, 4) runs backward into the first part, and a second edge on (40, 41), robust and 0.5 m off.
    (poses, {name: edge records})"""
    g = graph(48, loops=[(2, 13), (18, 30), (25, 4), (35, 10)], duplicate=[(40, 41)], seed=53)
    e = g["edges"]
    remeasure(g, 51, R.ROBUST, (0.5, 0.0, 0.0))
    return g["poses"], dict(chain=e[:47], loop_a=e[47:48], loop_b=e[48:50], loop_c=e[50:51], second_40_41=e[51:52])


def growth_stages():
    """The growth test's four stages as (nodes in the graph, the add_edges calls of the stage, fixed nodes at its optimise).
    Stage 3: the robust second edge on (40, 41) and the loop (35, 10) arrive in a call of their own BEFORE the chain edges,
    so by the header's rule that edge on (40, 41) is the chain edge and the plain one, later, a loop edge; 35 -> 36 arrives
    behind a loop edge on node 35; the edge into node 47 is left out until stage 4."""
    _, e = growth_graph()
    chain = e["chain"]
    return [(16, [np.concatenate([chain[:15], e["loop_a"]])], ()),
            (32, [np.concatenate([chain[15:31], e["loop_b"]])], ()),
            (48, [np.concatenate([e["second_40_41"], e["loop_c"]]), chain[31:46]], (20,)),
            (48, [chain[46:47]], ())]


REFERENCE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_graph_residual_reference.json")


@functools.lru_cache(maxsize=None)
def residual_reference():
    """tests/golden/pose_graph_residual_reference.json (tools/pose_graph_reference.py wrote it, 50 digits, rounded once):
    a list of (angle as text, Ti, Tj, Z [3][4], r [6])"""
    with open(REFERENCE_PATH) as f:
        doc = json.load(f)

    def arr(c, k, shape):
        return np.array([float.fromhex(v) for v in c[k]]).reshape(shape)

    return [(c["angle"], arr(c, "Ti", (3, 4)), arr(c, "Tj", (3, 4)), arr(c, "Z", (3, 4)), arr(c, "r", 6)) for c in doc["cases"]]


def residual_reference_graph():
    """The reference's cases as one graph: case c is the edge 2 c -> 2 c + 1 between its own two poses, the doubles of the
    file, with a full information matrix; every second edge robust."""
    rng = np.random.default_rng(78)
    poses, rows = [], []
    for c, (_angle, Ti, Tj, Z, _r) in enumerate(residual_reference()):
        poses += [Ti, Tj]
        rows.append((2 * c, 2 * c + 1, Z, information(rng, 0.05, 0.1), R.ROBUST if c % 2 else 0))
    return dict(poses=np.array(poses), edges=edges_of(rows), fixed=(), name="residual_reference")


def circle(N, L, seed, radius=20.0, noise=(0.002, 0.01), laps=2, false_loop=None, robust=False):
    """Two laps of a circle: chained noisy odometry edges, the start their composition from the true first pose, and L loop
    edges from a node of the first lap to the node at the same place in the second.  false_loop: that loop edge measures a
    translation 5 m off; robust: loop edges carry LFX_EDGE_ROBUST."""
    rng = np.random.default_rng(seed)
    ang = 2.0 * np.pi * laps * np.arange(N) / N
    truth = np.array([pose([0.0, 0.0, a + np.pi / 2.0], [radius * np.cos(a), radius * np.sin(a), 0.0]) for a in ang])
    om = information(rng, *noise, full=False)
    rows, first = [], [truth[0]]
    for i in range(N - 1):
        Z = perturb(between(truth[i], truth[i + 1]), rng, *noise)
        rows.append((i, i + 1, Z, om, 0))
        first.append(compose(first[-1], Z))
    half = N // laps
    for l in range(L):
        i = int(round((l + 0.5) * half / L)) % half
        Z = perturb(between(truth[i], truth[i + half]), rng, *noise)
        if false_loop == l:
            Z[:, 3] += np.array([5.0, 0.0, 0.0])
        rows.append((i, i + half, Z, om, R.ROBUST if robust else 0))
    return dict(poses=np.array(first), truth=truth, edges=edges_of(rows), fixed=(), name="circle_%d_%d" % (N, L))


def worst_error(poses, truth):
    return float(np.linalg.norm(np.asarray(poses)[:, :, 3] - truth[:, :, 3], axis=1).max())


# the seeds of the convergence and the robust cases, chosen on the restatement alone (test_pose_graph_expect.py holds the
# conditions they were chosen by)
CIRCLE_SEED = {5: 11, 40: 11}
FALSE_LOOP_SEED = 21


def circles():
    return [circle(256, L, CIRCLE_SEED[L]) for L in (5, 40)]


def false_loop_cases():
    """(with the false loop and robust edges, the same without the flag, the same graph without the outlier)"""
    return (circle(256, 5, FALSE_LOOP_SEED, false_loop=2, robust=True), circle(256, 5, FALSE_LOOP_SEED, false_loop=2, robust=False),
            circle(256, 5, FALSE_LOOP_SEED, robust=True))


@functools.lru_cache(maxsize=None)
def circle_results():
    """the restatement's (poses, result, (rho, w)) for circles(), computed once"""
    return [R.optimize(g["poses"], g["edges"]) for g in circles()]


@functools.lru_cache(maxsize=None)
def false_loop_runs():
    """the restatement's (poses, result, (rho, w)) for false_loop_cases(), by name"""
    return {name: R.optimize(g["poses"], g["edges"], max_iter=20, huber_delta=3.0)
            for name, g in zip(("robust", "plain", "clean"), false_loop_cases())}


@functools.lru_cache(maxsize=None)
def false_loop_results():
    """the restatement's worst position error for false_loop_cases(), by name"""
    return {name: worst_error(false_loop_runs()[name][0], g["truth"]) for name, g in zip(("robust", "plain", "clean"), false_loop_cases())}


@functools.lru_cache(maxsize=None)
def dense_first_steps():
    """name -> (delta of the first dense step, its linearisation) for every one-step shape and both circles"""
    return {g["name"]: R.dense_step(g["poses"], g["edges"], g["fixed"]) for g in step_shapes() + circles()}


@functools.lru_cache(maxsize=None)
def floor():
    """The measured floor f: the largest difference between the step through the solver's statement and the dense step,
    over every shape the device is checked at.  (f, {name: difference})"""
    seen = {}
    for g in step_shapes() + circles():
        dense, lin = dense_first_steps()[g["name"]]
        seen[g["name"]] = float(np.abs(R.woodbury_step(g["poses"], g["edges"], g["fixed"], lin=lin) - dense).max())
    return max(seen.values()), seen


GAP_SHAPES = ("N65_chain_31_32_missing_bridged",)


def floors():
    """(the floor over the shapes with a whole chain, the floor of the shape with a missing chain edge): the second is five
    orders above the first (P is held by lambda alone along six directions there), so each class is held to its own."""
    seen = floor()[1]
    return max(v for k, v in seen.items() if k not in GAP_SHAPES), max(seen[k] for k in GAP_SHAPES)


def floor_of(name):
    whole, gap = floors()
    return gap if name in GAP_SHAPES else whole
