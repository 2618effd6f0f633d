"""The graphs the covariances are checked at (tests/test_pose_graph_marginal_expect.py on the host,
tests/test_pose_graph_marginal_gpu.py on the device): the smallest shapes at which each kernel can go wrong, with the pairs
whose joint blocks are asked for, and the tolerance's constants beside them.

THE TOLERANCE of a case: |Sigma_device - Sigma_reference| <= C * MARGIN * eps * kappa_2(H) * max |Sigma|, every block.
C is the worst ratio, over the cases of its class (C_WHOLE, C_GAP: below), of the float64 restatement of the device's algorithm (pose_graph_marginal_restatement
.algorithm) against the 50-digit reference, in units of eps * kappa_2 * max |Sigma|, measured on the host alone (measure()
below prints it; the expect test holds the restatement to it).  MARGIN = 4 is for the device's other order of summation
(strided and tree dot products, the panel-blocked substitution): both are backward-stable float64 eliminations of one matrix.
KAPPA records kappa_2(H + lambda I) over the free nodes of each case at its start poses (the expect test holds the record to
what it computes, and every value below CAP = 1e10, so that the bound stays below 1e-5 relative and cannot hide a wrong
block); the device's bound uses kappa_2 at the device's own final poses."""
import functools

import numpy as np

from tests import pose_graph_cases as K
from tests import pose_graph_marginal_restatement as M
from tests import pose_graph_prior_cases as PK

EPS = 2.0 ** -52
MARGIN = 4.0
CAP = 1e10
DENSE_REFERENCE_NODES = 12       # up to here the 50-digit reference is mpmath's dense inverse; beyond, the algorithm at 50 digits
PANEL = K.PANEL


def _loops(N, L, seed):
    rng = np.random.default_rng(seed)
    return [tuple(int(v) for v in rng.choice(N, 2, replace=False)) for _ in range(L)]


def as_case(name, g, pairs=(), priors=None, released=False, **config):
    out = dict(g, name=name, pairs=tuple(pairs), priors=M.NO_PRIORS if priors is None else priors, released=released)
    out.setdefault("damping", 1e-6)
    out.setdefault("huber_delta", 3.0)
    out.update(config)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    rng = np.random.default_rng(900)
    # one node: free, held by a pose prior alone
    g = K.graph(1, seed=61)
    out.append(as_case("N1_prior", g, priors=PK.priors_of([PK.pose_row(g["truth"][0], 0, rng)]), released=True))
    out.append(as_case("N2_L0", K.graph(2, seed=62)))
    out.append(as_case("N3_L1", K.graph(3, loops=[(0, 2)], seed=63), pairs=[(1, 2), (2, 1)]))
    # 6 L = 0, 6, 48 (one panel exactly full), 54 (one over), 102 (two panels and a bit)
    for L in (0, 1, PANEL // 6, PANEL // 6 + 1, 2 * PANEL // 6 + 1):
        out.append(as_case("N12_L%d" % L, K.graph(12, loops=_loops(12, L, 200 + L), seed=64 + L), pairs=[(1, 2), (3, 9), (9, 3), (3, 11)]))
    # wave and workgroup boundaries of the per-node kernels and of the row tiles (6 N = 384, 390, 1542 rows in tiles of 64)
    out.append(as_case("N64_L9", K.graph(64, loops=_loops(64, 9, 264), seed=70), pairs=[(1, 2), (1, 3), (1, 63), (63, 1), (0, 5)]))
    out.append(as_case("N65_L9", K.graph(65, loops=_loops(65, 9, 265), seed=71), pairs=[(1, 64), (64, 1), (1, 65 - 1), (2, 64), (10, 11)]))
    g = K.graph(257, loops=_loops(257, 9, 457), seed=72)
    out.append(as_case("N257_L9_released", g, priors=PK.priors_of([PK.pose_row(g["truth"][0], 0, rng)]), released=True,
                     pairs=[(0, 1), (1, 0), (0, 2), (0, 63), (0, 64), (64, 0), (0, 256), (256, 0), (5, 6), (6, 7), (100, 228)]))
    out.append(as_case("N65_chain_31_32_missing_bridged", K.graph(65, loops=[(30, 33), (5, 60)], missing=(31,), seed=4),
                     pairs=[(31, 32), (32, 31), (30, 33), (1, 64)]))
    out.append(as_case("fixed_middle_and_end", K.graph(24, loops=[(2, 15), (20, 6), (11, 13)], fixed=(12, 23), seed=73),
                     pairs=[(11, 13), (13, 11), (12, 13), (5, 12), (22, 23), (3, 20)]))
    g = K.graph(16, loops=[(2, 12)], seed=74)
    out.append(as_case("released_pose_prior", g, priors=PK.priors_of([PK.pose_row(g["truth"][5], 5, rng)]), released=True,
                     pairs=[(0, 15), (15, 0), (5, 6)]))
    g = K.graph(16, loops=[(3, 13)], seed=75)
    rows = [PK.position_row(g["truth"][k], k, rng, lever=PK.LEVER) for k in (0, 4, 8, 12, 15)]
    out.append(as_case("released_position_priors_lever", g, priors=PK.priors_of(rows), released=True, pairs=[(0, 15), (4, 8)]))
    # a false loop, robust.  The start is the truth: there, as at the optimum, the false loop alone is down-weighted (at the
    # circle's own start, the chained odometry, the drift would put every loop beyond huber_delta)
    g = K.circle(64, 5, K.FALSE_LOOP_SEED, false_loop=2, robust=True)
    g["poses"] = g["truth"].copy()
    out.append(as_case("robust_false_loop", g, pairs=[(10, 42), (42, 10), (1, 2)]))
    # node 19 has no edge: Sigma = I / lambda there.  lambda = 1e-3: with 1e-6, 1 / lambda alone would carry kappa past the cap
    out.append(as_case("isolated_last_node", K.graph(20, loops=[(3, 14), (16, 5)], missing=(18,), seed=52), pairs=[(18, 19), (19, 3)],
                     damping=1e-3))
    return out


def case(name):
    return [c for c in cases() if c["name"] == name][0]


def system_of(c, poses=None):
    return M.system(c["poses"] if poses is None else poses, c["edges"], c["priors"], c["fixed"], c["released"], c["damping"], c["huber_delta"])


def reference_blocks(c, poses=None):
    """(Sigma_kk, {pair: Sigma_ij}, kappa_2, max |Sigma|) of the case at `poses` (its start poses where None), 50 digits"""
    s = system_of(c, poses)
    if s["N"] <= DENSE_REFERENCE_NODES:
        diag, cross = M.blocks(M.reference(s), s["N"], c["pairs"])
    else:
        diag, cross = M.algorithm(s, c["pairs"], digits=M.DIGITS)
    top = max([float(np.abs(diag).max())] + [float(np.abs(v).max()) for v in cross.values()])
    return diag, cross, M.condition(s), top


@functools.lru_cache(maxsize=None)
def start_reference(name):
    return reference_blocks(case(name))


def worst(got_diag, got_cross, ref):
    """the largest difference over every block, in units of eps * kappa_2 * max |Sigma|"""
    diag, cross, kappa, top = ref
    err = max([float(np.abs(got_diag - diag).max())] + [float(np.abs(got_cross[p] - cross[p]).max()) for p in cross])
    return err / (EPS * kappa * top)


def bound(name, ref):
    """the device's tolerance for the case `name`, from a reference at the device's own poses"""
    _, _, kappa, top = ref
    return c_of(name) * MARGIN * EPS * kappa * top


@functools.lru_cache(maxsize=None)
def measure():
    """{name: (the float64 restatement's error in units of eps * kappa_2 * max |Sigma|, kappa_2)} at the start poses"""
    out = {}
    for c in cases():
        ref = start_reference(c["name"])
        d, x = M.algorithm(system_of(c), c["pairs"])
        out[c["name"]] = (worst(d, x, ref), ref[2])
    return out


# Measured by measure() on the host (python -m tests.pose_graph_marginal_cases prints them), rounded up to two digits.  Two
# classes, as pose_graph_cases.floors(): where a chain edge is missing and only a loop bridges the gap, P is held by lambda
# alone along six directions, P^-1 and V V^T are both near 1 / lambda there and cancel, and the algorithm -- on the host as
# on the device -- loses kappa_2(P) / kappa_2(H) digits.  One C over all cases would be that shape's 162 and would let the
# others' bounds grow 2 000-fold, past the 1e-5 the cap is there for; so every other case is held to its own class's worst.
C_WHOLE, C_GAP = 0.069, 162.0
GAP_CASES = ("N65_chain_31_32_missing_bridged",)
KAPPA = {
    "N1_prior": 2.634e+01,   # ratio 0.0474
    "N2_L0": 2.725e+01,   # ratio 0.0681
    "N3_L1": 8.023e+01,   # ratio 0.0235
    "N12_L0": 9.626e+03,   # ratio 0.00735
    "N12_L1": 9.468e+03,   # ratio 0.00222
    "N12_L8": 2.025e+03,   # ratio 0.0106
    "N12_L9": 2.503e+03,   # ratio 0.00808
    "N12_L17": 1.097e+03,   # ratio 0.0646
    "N64_L9": 4.868e+05,   # ratio 0.000206
    "N65_L9": 7.005e+05,   # ratio 0.000212
    "N257_L9_released": 7.365e+07,   # ratio 0.000225
    "N65_chain_31_32_missing_bridged": 5.636e+05,   # ratio 161
    "fixed_middle_and_end": 3.539e+03,   # ratio 0.00162
    "released_pose_prior": 1.194e+04,   # ratio 0.00227
    "released_position_priors_lever": 5.645e+04,   # ratio 0.00294
    "robust_false_loop": 1.195e+06,   # ratio 0.00122
    "isolated_last_node": 2.191e+09,   # ratio 4.67e-10
}


def c_of(name):
    return C_GAP if name in GAP_CASES else C_WHOLE


if __name__ == "__main__":
    seen = measure()
    print("C_WHOLE = %.3g, C_GAP = %.3g" % (max(v[0] for k, v in seen.items() if k not in GAP_CASES), max(seen[k][0] for k in GAP_CASES)))
    for name, (ratio, kappa) in seen.items():
        print('    "%s": %.3e,   # ratio %.3g' % (name, kappa, ratio))
