"""The pose-graph problem of include/lfx.h (the pose graph section) restated on the host, literally.

Two layers.  The LINEARISATION of an edge -- r, w, rho, A_i, A_j, q = w Omega r -- and the nodes' gradient are written with
scalars, every sum of products through Arith.dot, left to right, so that one text gives two evaluations: every product
rounded before it is added (what the library's kernels do: they are built with contraction off) and every product fused
into the addition (one rounding; exact through fractions).  The difference between the two is the bracket the device's
linearisation is held to.  Arith also remembers the largest term it added: the floor of that comparison is in its units.

The STEP is dense numpy: H assembled over all nodes (a fixed node has the identity and no coupling), numpy.linalg.solve.
That is what the device is judged by.  woodbury_step follows the solver's statement -- chain / loop split, block-tridiagonal
P factored block by block, y0 = P^-1 (-g), Y = P^-1 J^T, S = W^-1 + J Y, delta = y0 - Y S^-1 (J y0) -- in numpy and exists
only to measure how far the two ways to the same step lie apart in double precision (tests/pose_graph_cases.py floor())."""
import math
from fractions import Fraction

import numpy as np

ROBUST = 1
CONVERGED, MAX_ITERATIONS, DIVERGED, NOT_POSITIVE_DEFINITE = 0, 1, 2, 3
DEFAULTS = dict(max_iter=10, damping=1e-6, tolerance=1e-9, huber_delta=3.0)


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


class Arith:
    def __init__(self, fused=False):
        self.fused = fused
        self.largest = 0.0
        self.seen = {}

    def mark(self, name):
        """The largest term since the last mark goes under `name` (the largest of all that went there)."""
        self.seen[name] = max(self.seen.get(name, 0.0), self.largest)
        self.largest = 0.0

    def dot(self, a, b):
        """sum of a[k] * b[k], left to right"""
        s = 0.0
        for k, (x, y) in enumerate(zip(a, b)):
            x, y = float(x), float(y)
            self.largest = max(self.largest, abs(x * y))
            if k == 0:
                s = x * y
            elif self.fused:
                s = _fma(x, y, s)
            else:
                s = s + x * y
        return s


def _cols(m, c):
    return [m[0][c], m[1][c], m[2][c]]


def _tmul(ar, a, b):
    """a^T b, 3 x 3"""
    return [[ar.dot(_cols(a, r), _cols(b, c)) for c in range(3)] for r in range(3)]


def _hat(v):
    return [[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]]


def log_rotation(RE):
    v = [0.5 * (RE[2][1] - RE[1][2]), 0.5 * (RE[0][2] - RE[2][0]), 0.5 * (RE[1][0] - RE[0][1])]
    nv = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    theta = math.atan2(nv, 0.5 * (((RE[0][0] + RE[1][1]) + RE[2][2]) - 1.0))
    if nv < 1e-10:
        return list(v), theta
    return [x * (theta / nv) for x in v], theta


def jr_inverse(ar, phi, theta):
    if theta < 1e-4:
        c = 1.0 / 12.0 + theta * theta / 720.0
    else:
        c = 1.0 / (theta * theta) - (1.0 + math.cos(theta)) / (2.0 * theta * math.sin(theta))
    px = _hat(phi)
    out = [[0.0] * 3 for _ in range(3)]
    for r in range(3):
        for k in range(3):
            p2 = ar.dot(px[r], _cols(px, k))
            out[r][k] = ((1.0 if r == k else 0.0) + 0.5 * px[r][k]) + c * p2
    return out


def edge_terms(Ti, Tj, Z, omega, flags, huber_delta, ar=None):
    """One edge at the poses Ti, Tj ([3][4]): (r [6], w, rho, A_i [6][6], A_j [6][6], q = w Omega r [6])."""
    ar = ar or Arith()
    Ti, Tj, Z, omega = (np.asarray(x, np.float64).tolist() for x in (Ti, Tj, Z, omega))
    Ri, Rj, Rz = ([row[:3] for row in T] for T in (Ti, Tj, Z))
    ti, tj, tz = ([row[3] for row in T] for T in (Ti, Tj, Z))
    M = _tmul(ar, Ri, Rj)
    RE = _tmul(ar, Rz, M)
    dt = [tj[k] - ti[k] for k in range(3)]
    d = [ar.dot(_cols(Ri, r), dt) for r in range(3)]
    dz = [d[k] - tz[k] for k in range(3)]
    tE = [ar.dot(_cols(Rz, r), dz) for r in range(3)]
    RzRi = [[ar.dot(_cols(Rz, r), Ri[c]) for c in range(3)] for r in range(3)]
    phi, theta = log_rotation(RE)
    Jri = jr_inverse(ar, phi, theta)
    dx = _hat(d)
    Ai = [[0.0] * 6 for _ in range(6)]
    Aj = [[0.0] * 6 for _ in range(6)]
    for r in range(3):
        for c in range(3):
            Aj[r][c] = Jri[r][c]
            Aj[3 + r][3 + c] = RzRi[r][c]
            Ai[r][c] = -ar.dot(Jri[r], M[c])
            Ai[3 + r][c] = ar.dot(_cols(Rz, r), _cols(dx, c))
            Ai[3 + r][3 + c] = -RzRi[r][c]
    res = phi + tE
    ar.mark("r")
    q = [ar.dot(omega[r], res) for r in range(6)]
    s2 = ar.dot(res, q)
    ar.mark("rho")
    w, rho = 1.0, s2
    if flags & ROBUST:
        s = math.sqrt(s2 if s2 > 0.0 else 0.0)
        if s > huber_delta:
            w = huber_delta / s
            rho = 2.0 * huber_delta * s - huber_delta * huber_delta
    return res, w, rho, Ai, Aj, [w * x for x in q]


def linearize(poses, edges, fixed=(), huber_delta=3.0, fused=False):
    """Every edge's terms and every node's gradient (a node's sum runs over its edges in edge order, as the library's
    incidence lists do).  edges: records with i, j, flags, z, information.  A dict of arrays, `largest` = the largest term
    added on the way to r (and the Jacobians), to rho and to g."""
    poses = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    N, E = len(poses), len(edges)
    fixed = set(int(k) for k in fixed) | {0}
    ar = Arith(fused)
    out = dict(r=np.zeros((E, 6)), w=np.zeros(E), rho=np.zeros(E), A_i=np.zeros((E, 6, 6)), A_j=np.zeros((E, 6, 6)), q=np.zeros((E, 6)),
               g=np.zeros((N, 6)))
    g = [[0.0] * 6 for _ in range(N)]
    for e in range(E):
        ed = edges[e]
        i, j = int(ed["i"]), int(ed["j"])
        r, w, rho, Ai, Aj, q = edge_terms(poses[i], poses[j], np.reshape(ed["z"], (3, 4)), np.reshape(ed["information"], (6, 6)),
                                          int(ed["flags"]), huber_delta, ar)
        out["r"][e], out["w"][e], out["rho"][e], out["A_i"][e], out["A_j"][e], out["q"][e] = r, w, rho, Ai, Aj, q
        for node, A in ((i, Ai), (j, Aj)):
            if node in fixed:
                continue
            for c in range(6):
                g[node][c] = g[node][c] + ar.dot([A[m][c] for m in range(6)], q)
        ar.mark("g")
    out["g"][:] = g
    out["chi2"] = float(np.sum(out["rho"]))
    out["largest"] = dict(ar.seen)
    return out


# --- the step, dense -----------------------------------------------------------------------------------------------------------
def exp_rotation(a):
    a = np.asarray(a, np.float64)
    th2 = float((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    th = math.sqrt(th2)
    A = 1.0 - th2 / 6.0 if th < 1e-4 else math.sin(th) / th
    B = 0.5 - th2 / 24.0 if th < 1e-4 else (1.0 - math.cos(th)) / th2
    ax = np.array(_hat(a))
    return np.eye(3) + A * ax + B * (ax @ ax)


def retract(poses, delta, fixed=()):
    """R <- R Exp(a), t <- t + b, then R <- R (3 I - R^T R) / 2; fixed nodes stay, and so does a node whose step is 0."""
    poses = np.array(poses, np.float64).reshape(-1, 3, 4)
    fixed = set(int(k) for k in fixed) | {0}
    for k in range(len(poses)):
        if k in fixed or not np.any(delta[k]):
            continue
        R = poses[k, :, :3] @ exp_rotation(delta[k, :3])
        poses[k, :, :3] = R @ (1.5 * np.eye(3) - 0.5 * (R.T @ R))
        poses[k, :, 3] += delta[k, 3:]
    return poses


def normal_equations(lin, edges, N, fixed=(), damping=1e-6):
    """(H + lambda I, g) over all nodes, dense; a fixed node has the identity, no coupling and no gradient."""
    fixed = set(int(k) for k in fixed) | {0}
    H = np.zeros((6 * N, 6 * N))
    for e in range(len(edges)):
        i, j = int(edges[e]["i"]), int(edges[e]["j"])
        W = lin["w"][e] * np.reshape(edges[e]["information"], (6, 6))
        Ai, Aj = lin["A_i"][e], lin["A_j"][e]
        si, sj = slice(6 * i, 6 * i + 6), slice(6 * j, 6 * j + 6)
        H[si, si] += Ai.T @ W @ Ai
        H[sj, sj] += Aj.T @ W @ Aj
        H[sj, si] += Aj.T @ W @ Ai
        H[si, sj] += Ai.T @ W @ Aj
    H += damping * np.eye(6 * N)
    g = lin["g"].reshape(-1).copy()
    for k in fixed:
        s = slice(6 * k, 6 * k + 6)
        H[s, :] = 0.0
        H[:, s] = 0.0
        H[s, s] = np.eye(6)
        g[s] = 0.0
    return H, g


def dense_step(poses, edges, fixed=(), damping=1e-6, huber_delta=3.0):
    lin = linearize(poses, edges, fixed, huber_delta)
    N = len(np.asarray(poses).reshape(-1, 12))
    H, g = normal_equations(lin, edges, N, fixed, damping)
    return np.linalg.solve(H, -g).reshape(N, 6), lin


def split_edges(edges, N):
    """(chain_edge [N] with -1 for none, loop edges in edge order): the chain is the first edge with j == i + 1 for each i."""
    chain = -np.ones(N, np.int64)
    loops = []
    for e in range(len(edges)):
        i, j = int(edges[e]["i"]), int(edges[e]["j"])
        if j == i + 1 and chain[i] < 0:
            chain[i] = e
        else:
            loops.append(e)
    return chain, loops


def woodbury_step(poses, edges, fixed=(), damping=1e-6, huber_delta=3.0, lin=None):
    """The same step through the solver's statement (module docstring); only tests/pose_graph_cases.py floor() uses it."""
    poses = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    N = len(poses)
    fixed = set(int(k) for k in fixed) | {0}
    lin = lin or linearize(poses, edges, fixed, huber_delta)
    chain, loops = split_edges(edges, N)
    D = np.array([np.eye(6) if k in fixed else damping * np.eye(6) for k in range(N)])
    O = np.zeros((N, 6, 6))
    for i in range(N):
        e = chain[i]
        if e < 0:
            continue
        W = lin["w"][e] * np.reshape(edges[e]["information"], (6, 6))
        Ai, Aj = lin["A_i"][e], lin["A_j"][e]
        if i not in fixed:
            D[i] += Ai.T @ W @ Ai
        if i + 1 not in fixed:
            D[i + 1] += Aj.T @ W @ Aj
        if i not in fixed and i + 1 not in fixed:
            O[i] = Aj.T @ W @ Ai
    L6 = len(loops)
    J = np.zeros((6 * L6, 6 * N))
    Winv = np.zeros((6 * L6, 6 * L6))
    for l, e in enumerate(loops):
        i, j = int(edges[e]["i"]), int(edges[e]["j"])
        if i not in fixed:
            J[6 * l:6 * l + 6, 6 * i:6 * i + 6] = lin["A_i"][e]
        if j not in fixed:
            J[6 * l:6 * l + 6, 6 * j:6 * j + 6] = lin["A_j"][e]
        Winv[6 * l:6 * l + 6, 6 * l:6 * l + 6] = np.linalg.inv(lin["w"][e] * np.reshape(edges[e]["information"], (6, 6)))
    g = lin["g"].reshape(-1).copy()
    for k in fixed:
        g[6 * k:6 * k + 6] = 0.0
    rhs = np.concatenate([-g[:, None], J.T], axis=1).reshape(N, 6, -1)
    # block Cholesky of the tridiagonal P, then forward and backward over the nodes for every column at once
    Lk, Mk = np.zeros((N, 6, 6)), np.zeros((N, 6, 6))
    S = D[0]
    for k in range(N):
        Lk[k] = np.linalg.cholesky(S)
        if k + 1 < N:
            Mk[k] = np.linalg.solve(Lk[k], O[k].T).T
            S = D[k + 1] - Mk[k] @ Mk[k].T
    y = np.zeros_like(rhs)
    for k in range(N):
        b = rhs[k] - (Mk[k - 1] @ y[k - 1] if k else 0.0)
        y[k] = np.linalg.solve(Lk[k], b)
    x = np.zeros_like(rhs)
    for k in range(N - 1, -1, -1):
        b = y[k] - (Mk[k].T @ x[k + 1] if k + 1 < N else 0.0)
        x[k] = np.linalg.solve(Lk[k].T, b)
    x = x.reshape(6 * N, -1)
    y0, Y = x[:, 0], x[:, 1:]
    if L6 == 0:
        return y0.reshape(N, 6)
    Sm = Winv + J @ Y
    return (y0 - Y @ np.linalg.solve(Sm, J @ y0)).reshape(N, 6)


def optimize(poses, edges, fixed=(), max_iter=10, damping=1e-6, tolerance=1e-9, huber_delta=3.0):
    """Gauss-Newton as lfx_pose_graph_optimize runs it, with the dense step: (poses, result dict, per-edge (rho, w) at the
    poses returned).  The result's steps: max |delta| of every iteration."""
    start = np.array(poses, np.float64).reshape(-1, 3, 4)
    cur = start.copy()
    lin = linearize(cur, edges, fixed, huber_delta)
    first = lin["chi2"]
    N = len(cur)
    it, steps, converged = 0, [], False
    while it < max_iter:
        it += 1
        H, g = normal_equations(lin, edges, N, fixed, damping)
        delta = np.linalg.solve(H, -g).reshape(N, 6)
        cur = retract(cur, delta, fixed)
        lin = linearize(cur, edges, fixed, huber_delta)
        steps.append(float(np.abs(delta).max()))
        if steps[-1] < tolerance:
            converged = True
            break
    last = lin["chi2"]
    chain, loops = split_edges(edges, N)
    res = dict(iterations=it, chi2_initial=first, chi2_final=last, max_step=steps[-1], steps=steps, n_chain=int((chain >= 0).sum()), n_loop=len(loops))
    if not (last == last) or last > first + 1e-12 * max(1.0, first):
        lin = linearize(start, edges, fixed, huber_delta)
        res.update(code=DIVERGED, chi2_final=first)
        cur = start
    else:
        res.update(code=CONVERGED if converged else MAX_ITERATIONS)
    res["n_robust_downweighted"] = int((lin["w"] < 1.0).sum())
    return cur, res, (lin["rho"].copy(), lin["w"].copy())


def edge_information(pose_j, H):
    """B H B^T, B = blkdiag(I, R_j^T)"""
    B = np.eye(6)
    B[3:, 3:] = np.asarray(pose_j, np.float64).reshape(3, 4)[:, :3].T
    return B @ np.asarray(H, np.float64).reshape(6, 6) @ B.T


def step_between(before, after):
    """The increments that lead from `before` to `after` ([N][3][4] each): a = Log(R^T R'), b = t' - t, [N][6]."""
    before, after = (np.asarray(x, np.float64).reshape(-1, 3, 4) for x in (before, after))
    out = np.zeros((len(before), 6))
    for k in range(len(before)):
        out[k, :3] = log_rotation((before[k, :, :3].T @ after[k, :, :3]).tolist())[0]
        out[k, 3:] = after[k, :, 3] - before[k, :, 3]
    return out
