"""The pose graph with priors (include/lfx.h, PRIORS) restated on the host, on top of tests/pose_graph_restatement.py.

A prior is a unary term on one node.  A POSE prior is, by definition, the edge from the identity to its node: prior_terms
calls R.edge_terms with the identity and keeps A_j.  A POSITION prior is written out with scalars through the same Arith, so
that it too has a fused and an unfused evaluation.  linearize, normal_equations, dense_step, woodbury_step and optimize are
those of the old restatement with the priors' terms added -- to the node's diagonal block and its gradient, nothing else --
and with `released_first`: node 0 is fixed unless it is released (the old functions always fix it, which is why they are
restated here instead of called).  tests/test_pose_graph_prior_expect.py holds this file to the old one: its dense step
against R.dense_step on the anchored graph (tests/pose_graph_prior_cases.py anchored())."""
import math

import numpy as np

from tests import pose_graph_restatement as R

PRIOR_ROBUST, PRIOR_POSITION = 1, 2
IDENTITY = [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]


def fixed_set(fixed, released_first):
    return set(int(k) for k in fixed) | (set() if released_first else {0})


def position_terms(Tk, tz, lever, ar):
    """r [6] and A [6][6] of a position prior at the pose Tk: r = (0, t_k + R_k l - t_Z), A = [[0, 0], [-R_k [l]x, I]]"""
    Tk = np.asarray(Tk, np.float64).tolist()
    Rk, tk = [row[:3] for row in Tk], [row[3] for row in Tk]
    l = [float(x) for x in lever]
    lx = R._hat(l)
    res = [0.0, 0.0, 0.0] + [(tk[r] + ar.dot(Rk[r], l)) - float(tz[r]) for r in range(3)]
    A = [[0.0] * 6 for _ in range(6)]
    for r in range(3):
        for c in range(3):
            A[3 + r][c] = -ar.dot(Rk[r], R._cols(lx, c))
            A[3 + r][3 + c] = 1.0 if r == c else 0.0
    return res, A


def prior_terms(Tk, prior, huber_delta, ar=None):
    """One prior at the pose Tk ([3][4]): (r [6], w, rho, A [6][6], q = w Omega r [6])."""
    ar = ar or R.Arith()
    flags = int(prior["flags"])
    Z = np.reshape(prior["z"], (3, 4))
    omega = np.reshape(prior["information"], (6, 6))
    robust = R.ROBUST if flags & PRIOR_ROBUST else 0
    if not flags & PRIOR_POSITION:
        res, w, rho, _Ai, Aj, q = R.edge_terms(IDENTITY, Tk, Z, omega, robust, huber_delta, ar)
        return res, w, rho, Aj, q
    res, A = position_terms(Tk, Z[:, 3], prior["lever"], ar)
    ar.mark("r")
    om = np.asarray(omega, np.float64).tolist()
    q = [ar.dot(om[r], res) for r in range(6)]
    s2 = ar.dot(res, q)
    ar.mark("rho")
    w, rho = 1.0, s2
    if robust:
        s = math.sqrt(s2 if s2 > 0.0 else 0.0)
        if s > huber_delta:
            w = huber_delta / s
            rho = 2.0 * huber_delta * s - huber_delta * huber_delta
    return res, w, rho, A, [w * x for x in q]


def linearize(poses, edges, priors, fixed=(), released_first=False, huber_delta=3.0, fused=False):
    """R.linearize with priors: every edge's and every prior's terms; a node's gradient sums its edges in edge order, then
    its priors in prior order (the library's two lists).  The priors' arrays carry the prefix p_."""
    poses = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    N, E, P = len(poses), len(edges), len(priors)
    fixed = fixed_set(fixed, released_first)
    ar = R.Arith(fused)
    out = dict(r=np.zeros((E, 6)), w=np.zeros(E), rho=np.zeros(E), A_i=np.zeros((E, 6, 6)), A_j=np.zeros((E, 6, 6)), q=np.zeros((E, 6)),
               p_r=np.zeros((P, 6)), p_w=np.zeros(P), p_rho=np.zeros(P), p_A=np.zeros((P, 6, 6)), p_q=np.zeros((P, 6)), g=np.zeros((N, 6)))
    g = [[0.0] * 6 for _ in range(N)]
    for e in range(E):
        ed = edges[e]
        i, j = int(ed["i"]), int(ed["j"])
        r, w, rho, Ai, Aj, q = R.edge_terms(poses[i], poses[j], np.reshape(ed["z"], (3, 4)), np.reshape(ed["information"], (6, 6)),
                                            int(ed["flags"]), huber_delta, ar)
        out["r"][e], out["w"][e], out["rho"][e], out["A_i"][e], out["A_j"][e], out["q"][e] = r, w, rho, Ai, Aj, q
        for node, A in ((i, Ai), (j, Aj)):
            if node in fixed:
                continue
            for c in range(6):
                g[node][c] = g[node][c] + ar.dot([A[m][c] for m in range(6)], q)
        ar.mark("g")
    for p in range(P):
        k = int(priors[p]["node"])
        r, w, rho, A, q = prior_terms(poses[k], priors[p], huber_delta, ar)
        out["p_r"][p], out["p_w"][p], out["p_rho"][p], out["p_A"][p], out["p_q"][p] = r, w, rho, A, q
        if k not in fixed:
            for c in range(6):
                g[k][c] = g[k][c] + ar.dot([A[m][c] for m in range(6)], q)
        ar.mark("g")
    out["g"][:] = g
    out["chi2_priors"] = float(np.sum(out["p_rho"]))
    out["chi2"] = float(np.sum(out["rho"])) + out["chi2_priors"]
    out["largest"] = dict(ar.seen)
    return out


def retract(poses, delta, fixed):
    """R.retract over the given fixed set alone"""
    poses = np.array(poses, np.float64).reshape(-1, 3, 4)
    for k in range(len(poses)):
        if k in fixed or not np.any(delta[k]):
            continue
        Rk = poses[k, :, :3] @ R.exp_rotation(delta[k, :3])
        poses[k, :, :3] = Rk @ (1.5 * np.eye(3) - 0.5 * (Rk.T @ Rk))
        poses[k, :, 3] += delta[k, 3:]
    return poses


def prior_block(lin, priors, p):
    """A^T w Omega A of prior p: what it adds to its node's diagonal block"""
    A = lin["p_A"][p]
    return A.T @ (lin["p_w"][p] * np.reshape(priors[p]["information"], (6, 6))) @ A


def normal_equations(lin, edges, priors, N, fixed=(), released_first=False, damping=1e-6):
    """(H + lambda I, g) over all nodes, dense; a fixed node has the identity, no coupling and no gradient."""
    fixed = fixed_set(fixed, released_first)
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
    for p in range(len(priors)):
        k = int(priors[p]["node"])
        H[6 * k:6 * k + 6, 6 * k:6 * k + 6] += prior_block(lin, priors, p)
    H += damping * np.eye(6 * N)
    g = lin["g"].reshape(-1).copy()
    for k in fixed:
        s = slice(6 * k, 6 * k + 6)
        H[s, :] = 0.0
        H[:, s] = 0.0
        H[s, s] = np.eye(6)
        g[s] = 0.0
    return H, g


def dense_step(poses, edges, priors, fixed=(), released_first=False, damping=1e-6, huber_delta=3.0):
    lin = linearize(poses, edges, priors, fixed, released_first, huber_delta)
    N = len(np.asarray(poses).reshape(-1, 12))
    H, g = normal_equations(lin, edges, priors, N, fixed, released_first, damping)
    return np.linalg.solve(H, -g).reshape(N, 6), lin


def woodbury_step(poses, edges, priors, fixed=(), released_first=False, damping=1e-6, huber_delta=3.0, lin=None):
    """R.woodbury_step with the priors' blocks added to D (their gradient is in lin["g"] already); S, J and the chain solve
    are untouched by them."""
    poses = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    N = len(poses)
    fixed = fixed_set(fixed, released_first)
    lin = lin or linearize(poses, edges, priors, fixed, released_first, huber_delta)
    chain, loops = R.split_edges(edges, N)
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
    for p in range(len(priors)):
        k = int(priors[p]["node"])
        if k not in fixed:
            D[k] += prior_block(lin, priors, p)
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


def optimize(poses, edges, priors, fixed=(), released_first=False, max_iter=10, damping=1e-6, tolerance=1e-9, huber_delta=3.0):
    """R.optimize with priors: (poses, result dict, per-edge (rho, w), per-prior (rho, w)).  n_robust_downweighted counts
    edges only, n_prior_downweighted the priors; chi2_priors is the priors' share of chi2_final."""
    start = np.array(poses, np.float64).reshape(-1, 3, 4)
    cur = start.copy()
    fs = fixed_set(fixed, released_first)
    lin = linearize(cur, edges, priors, fixed, released_first, huber_delta)
    first = lin["chi2"]
    N = len(cur)
    it, steps, converged = 0, [], False
    while it < max_iter:
        it += 1
        H, g = normal_equations(lin, edges, priors, N, fixed, released_first, damping)
        delta = np.linalg.solve(H, -g).reshape(N, 6)
        cur = retract(cur, delta, fs)
        lin = linearize(cur, edges, priors, fixed, released_first, huber_delta)
        steps.append(float(np.abs(delta).max()))
        if steps[-1] < tolerance:
            converged = True
            break
    last = lin["chi2"]
    chain, loops = R.split_edges(edges, N)
    res = dict(iterations=it, chi2_initial=first, chi2_final=last, max_step=steps[-1], steps=steps, n_chain=int((chain >= 0).sum()), n_loop=len(loops))
    if not (last == last) or last > first + 1e-12 * max(1.0, first):
        lin = linearize(start, edges, priors, fixed, released_first, huber_delta)
        res.update(code=R.DIVERGED, chi2_final=first)
        cur = start
    else:
        res.update(code=R.CONVERGED if converged else R.MAX_ITERATIONS)
    res["n_robust_downweighted"] = int((lin["w"] < 1.0).sum())
    res["n_prior_downweighted"] = int((lin["p_w"] < 1.0).sum())
    res["chi2_priors"] = lin["chi2_priors"]
    return cur, res, (lin["rho"].copy(), lin["w"].copy()), (lin["p_rho"].copy(), lin["p_w"].copy())
