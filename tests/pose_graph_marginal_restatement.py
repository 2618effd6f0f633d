"""The covariances of a pose graph's nodes (include/lfx.h, COVARIANCES) restated on the host.

THE DEFINITION: H + lambda I of the solver's linearisation at given poses, dense (tests/pose_graph_restatement.py and
tests/pose_graph_prior_restatement.py assemble it), the rows and columns of fixed nodes removed, inverted, zeros put back.
definition() does that with numpy, reference() with mpmath at 50 digits.

THE DEVICE'S ALGORITHM (lfx_kernels_posegraph.hpp, 6): H + lambda I = P + Jt^T Jt, P block-tridiagonal, Jt the loop edges'
whitened rows; the selected inverse of P's block Cholesky factor, G_k = L_k^-T L_k^-1 + T_k G_{k+1} T_k^T with
T_k = -L_k^-T M_k^T; V = Y L_S^-T by forward substitution, Y = P^-1 Jt^T, S = I + Jt Y = L_S L_S^T; Sigma_kk = G_k - V_k V_k^T,
Sigma_ij = T_i ... T_{j-1} G_j - V_i V_j^T.  algorithm() is that text over arrays of any number type: float64 arrays make it
the float64 restatement whose error measures the tolerance's constant; arrays of mpmath numbers make it a 50-digit evaluation
of the same algebra, which is the reference where the dense 50-digit inverse is out of reach (6 N beyond a few hundred) and
which tests/test_pose_graph_marginal_expect.py holds against the dense one wherever both exist."""
import numpy as np

from tests import pose_graph_prior_restatement as Q
from tests import pose_graph_restatement as R

NO_PRIORS = np.zeros(0, np.dtype([("node", "<u4"), ("flags", "<u4"), ("z", "<f8", 12), ("information", "<f8", 36), ("lever", "<f8", 3)]))
DIGITS = 50


def system(poses, edges, priors=None, fixed=(), released=False, damping=1e-6, huber_delta=3.0):
    """The solver's linearisation at `poses`: a dict with H (H + lambda I over all nodes, a fixed node the identity), the
    fixed set, the linearisation and N."""
    priors = NO_PRIORS if priors is None else priors
    poses = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    N = len(poses)
    lin = Q.linearize(poses, edges, priors, fixed, released, huber_delta)
    H, _ = Q.normal_equations(lin, edges, priors, N, fixed, released, damping)
    return dict(H=H, fixed=Q.fixed_set(fixed, released), lin=lin, N=N, edges=edges, priors=priors, damping=damping)


def free_index(N, fixed):
    return np.array([6 * k + c for k in range(N) if k not in fixed for c in range(6)], np.int64)


def definition(sys):
    """Sigma [6 N][6 N] by the definition, float64"""
    N, idx = sys["N"], free_index(sys["N"], sys["fixed"])
    out = np.zeros((6 * N, 6 * N))
    if len(idx):
        out[np.ix_(idx, idx)] = np.linalg.inv(sys["H"][np.ix_(idx, idx)])
    return out


def condition(sys):
    """kappa_2 of H + lambda I over the free nodes, from its eigenvalues"""
    idx = free_index(sys["N"], sys["fixed"])
    ev = np.linalg.eigvalsh(sys["H"][np.ix_(idx, idx)])
    return float(ev[-1] / ev[0])


def reference(sys):
    """Sigma [6 N][6 N] by the definition at 50 digits (mpmath's inverse of the free part), rounded once to float64.  For
    graphs of a few dozen nodes: the cost grows as (6 N)^3 operations of Python numbers."""
    import mpmath
    N, idx = sys["N"], free_index(sys["N"], sys["fixed"])
    out = np.zeros((6 * N, 6 * N))
    with mpmath.workdps(DIGITS):
        inv = mpmath.matrix(sys["H"][np.ix_(idx, idx)].tolist()) ** -1
        out[np.ix_(idx, idx)] = np.array([[float(inv[r, c]) for c in range(len(idx))] for r in range(len(idx))])
    return out


# --- the device's algorithm, over any number type -------------------------------------------------------------------------
def _chol(a, sqrt):
    """the lower Cholesky factor of a (its lower triangle is read)"""
    n = len(a)
    L = np.zeros_like(a)
    for j in range(n):
        p = a[j, j] - (L[j, :j] * L[j, :j]).sum() if j else a[j, j]
        if not p > 0:
            raise ArithmeticError("a pivot that is not positive")
        L[j, j] = sqrt(p)
        for r in range(j + 1, n):
            L[r, j] = (a[r, j] - ((L[r, :j] * L[j, :j]).sum() if j else 0)) / L[j, j]
    return L


def _forward(L, b):
    """L x = b, b a matrix of right-hand sides"""
    x = np.zeros_like(b)
    for r in range(len(L)):
        x[r] = (b[r] - (L[r, :r] @ x[:r] if r else 0)) / L[r, r]
    return x


def _backward(L, b):
    """L^T x = b"""
    x = np.zeros_like(b)
    n = len(L)
    for r in range(n - 1, -1, -1):
        x[r] = (b[r] - (L[r + 1:, r] @ x[r + 1:] if r + 1 < n else 0)) / L[r, r]
    return x


def split(sys):
    """(D [N][6][6], O [N][6][6], Jt [6 L][6 N]) of H + lambda I = P + Jt^T Jt, float64: P's blocks (k, k) and (k + 1, k),
    and the loop edges' rows whitened, sqrt(w) C^T A with Omega = C C^T, zero for a fixed node"""
    N, fixed, lin, edges, priors = sys["N"], sys["fixed"], sys["lin"], sys["edges"], sys["priors"]
    chain, loops = R.split_edges(edges, N)
    D = np.array([np.eye(6) if k in fixed else sys["damping"] * np.eye(6) for k in range(N)])
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
            D[k] += Q.prior_block(lin, priors, p)
    Jt = np.zeros((6 * len(loops), 6 * N))
    for l, e in enumerate(loops):
        i, j = int(edges[e]["i"]), int(edges[e]["j"])
        C = np.linalg.cholesky(np.reshape(edges[e]["information"], (6, 6)))
        sw = np.sqrt(lin["w"][e])
        if i not in fixed:
            Jt[6 * l:6 * l + 6, 6 * i:6 * i + 6] = sw * (C.T @ lin["A_i"][e])
        if j not in fixed:
            Jt[6 * l:6 * l + 6, 6 * j:6 * j + 6] = sw * (C.T @ lin["A_j"][e])
    return D, O, Jt


def algorithm(sys, pairs=(), digits=None, chain_solve=False):
    """The device's algorithm: (Sigma_kk [N][6][6], {(i, j): Sigma_ij [6][6]}), float64 -- computed in float64, or where
    `digits` is given with that many digits and rounded once.  pairs: (i, j) in either order.  chain_solve: the chain part
    of Sigma_ij from six columns of a solve with P (P^-1 E_j) and not from the product of the T_k."""
    N, fixed = sys["N"], sys["fixed"]
    D, O, Jt = split(sys)
    sqrt, conv = np.sqrt, (lambda x: x)
    if digits:
        import mpmath
        ctx = mpmath.mp.clone()
        ctx.dps = digits
        sqrt = ctx.sqrt
        conv = np.vectorize(ctx.mpf, otypes=[object])
        D, O, Jt = conv(D), conv(O), (conv(Jt) if Jt.size else Jt.astype(object))
    n = len(Jt)
    eye = conv(np.eye(6))
    Lk, Mk = [None] * N, [None] * N
    S = D[0]
    for k in range(N):
        Lk[k] = _chol(S, sqrt)
        Mk[k] = _forward(Lk[k], O[k].T).T                      # M_k = O_k L_k^-T
        if k + 1 < N:
            S = D[k + 1] - Mk[k] @ Mk[k].T
    # the selected inverse, backward
    G, T = [None] * N, [None] * N
    for k in range(N - 1, -1, -1):
        Li = _forward(Lk[k], eye)
        W = Li.T @ Li
        if k + 1 < N:
            T[k] = -(Li.T @ Mk[k].T)
            G[k] = W + T[k] @ G[k + 1] @ T[k].T
        else:
            T[k] = 0 * eye
            G[k] = W
        G[k] = (G[k] + G[k].T) / 2

    def chain(rhs):
        """P^-1 rhs, rhs [N][6][m]"""
        y = [None] * N
        for k in range(N):
            y[k] = _forward(Lk[k], rhs[k] - (Mk[k - 1] @ y[k - 1] if k else 0))
        x = [None] * N
        for k in range(N - 1, -1, -1):
            x[k] = _backward(Lk[k], y[k] - (Mk[k].T @ x[k + 1] if k + 1 < N else 0))
        return x

    V = None
    if n:
        Y = np.concatenate(chain(list(Jt.T.reshape(N, 6, n))), axis=0)      # [6 N][n]
        Ls = _chol(conv(np.eye(n)) + Jt @ Y, sqrt)
        V = _forward(Ls, Y.T).T                                  # every row v solves v L_S^T = y
    diag = np.zeros((N, 6, 6))
    for k in range(N):
        if k in fixed:
            continue
        s = G[k] - (V[6 * k:6 * k + 6] @ V[6 * k:6 * k + 6].T if n else 0)
        diag[k] = np.array(s, dtype=np.float64)
    cross = {}
    for (a, b) in pairs:
        i, j = min(a, b), max(a, b)
        if i in fixed or j in fixed:
            cross[(a, b)] = np.zeros((6, 6))
            continue
        if chain_solve:
            X = chain([eye if k == j else 0 * eye for k in range(N)])[i]
        else:
            X = G[j]
            for k in range(j - 1, i - 1, -1):
                X = T[k] @ X
        s = np.array(X - (V[6 * i:6 * i + 6] @ V[6 * j:6 * j + 6].T if n else 0), dtype=np.float64)
        cross[(a, b)] = s if a < b else s.T
    return diag, cross


def blocks(sigma, N, pairs=()):
    """(Sigma_kk [N][6][6], {(i, j): Sigma_ij}) cut from a dense Sigma"""
    diag = np.array([sigma[6 * k:6 * k + 6, 6 * k:6 * k + 6] for k in range(N)])
    return diag, {(i, j): sigma[6 * i:6 * i + 6, 6 * j:6 * j + 6] for (i, j) in pairs}


def joint(diag, cross, i, j):
    """[[Sigma_ii, Sigma_ij], [Sigma_ji, Sigma_jj]], 12 x 12"""
    return np.block([[diag[i], cross[(i, j)]], [cross[(i, j)].T, diag[j]]])


# --- the covariance of an edge's residual -----------------------------------------------------------------------------------
def relative_covariance(pose_i, pose_j, joint12):
    """[A_i A_j] joint [A_i A_j]^T with the Jacobians of the edge (i, j, Z = T_i^-1 T_j) at the poses themselves"""
    Ti, Tj = (np.asarray(x, np.float64).reshape(3, 4) for x in (pose_i, pose_j))
    Ri, Rj = Ti[:, :3], Tj[:, :3]
    d = Ri.T @ (Tj[:, 3] - Ti[:, 3])
    Ai, Aj = np.zeros((6, 6)), np.zeros((6, 6))
    Ai[:3, :3] = -Rj.T @ Ri
    Ai[3:, :3] = Rj.T @ Ri @ np.array(R._hat(d))
    Ai[3:, 3:] = -Rj.T
    Aj[:3, :3] = np.eye(3)
    Aj[3:, 3:] = Rj.T
    A = np.concatenate([Ai, Aj], axis=1)
    return A @ np.asarray(joint12, np.float64).reshape(12, 12) @ A.T


def edge_residual(Ti, Tj, Z):
    """r [6] of an edge at the poses Ti, Tj"""
    return np.array(R.edge_terms(Ti, Tj, Z, np.eye(6), 0, 3.0)[0])
