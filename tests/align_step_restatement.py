"""Test-side restatement of ONE iteration of Optimizer::Run (optimizer.hpp:79-123) from the rows of a scan at a pose, in plain
Python and numpy (no GPU, nothing of the library, nothing of the oracle): ComputeErrors, Median and Scale by sorted(), the
Huber weights, IsDegenerate(D, 0.1) by eigvalsh, D, A and b summed EXACTLY (math.fsum per entry over the rounded products),
H = M^T A M, g = M^T b, dx = -H^-1 g, AngleAxisToQuaternion with its 1e-8 branch, q * dq, t + dt, the pose matrix as the
library's refresh_pose writes it, and the stopping tests.  tests/test_align_step_expect.py holds it to the oracle,
tests/test_align_step_gpu.py holds the device to it.

The tolerance that goes with it is derived, not tuned.  The sums have `rows` = 3 n3 + n1 terms, the 7 x 6 products and the
6 x 6 Cholesky solve stand for 64 more, every one rounds to 2^-53, and the solve carries a relative perturbation of H and g
to dx with cond2(H):

    B = (rows + 64) * 2^-53 * cond2(H) * |dx|                       (on the increment dq, dt)
    |dP| <= B * (1 + |t|_inf) + 16 * 2^-53 * (1 + max |P|)          (on the 3 x 4 pose)"""
import math

import numpy as np

from tests.report_restatement import HUBER_K, MAD_TO_SIGMA, make_m, quaternion_of

U = 2.0 ** -53
CONVERGED, LARGER_ERROR, LARGER_SCALE, MAX_ITERATION, EMPTY, NO_PLANE = 0, 1, 2, 3, 4, 5
DBL_MAX = 1.7976931348623157e308


def median_sorted(values):
    """Median (lib/src/stats.cpp:34-55) by sorted(): the middle value, or the mean of the lower and the upper middle one."""
    v = sorted(float(x) for x in values)
    n = len(v)
    if n & 1:
        return v[(n - 1) // 2]
    return (v[n // 2 - 1] + v[n // 2]) / 2.0


def scale_sorted(errors):
    """Scale (robust.cpp:36-50): 1.4826 * median(|e - median(e)|)."""
    m = median_sorted(errors)
    return MAD_TO_SIGMA * median_sorted(abs(float(e) - m) for e in errors)


def errors_of(r3, r1):
    """ComputeErrors (optimizer.cpp:99-107): (r0 r0 + r1 r1) + r2 r2 per residual of dimension 3, r r per one of dimension 1."""
    r3 = np.asarray(r3, np.float64).reshape(-1, 3)
    r1 = np.asarray(r1, np.float64).reshape(-1)
    with np.errstate(over="ignore", under="ignore"):
        return np.concatenate([(r3[:, 0] * r3[:, 0] + r3[:, 1] * r3[:, 1]) + r3[:, 2] * r3[:, 2], r1 * r1])


def drp_dq(q, p):
    """rotationlib DRpDq (jacobian/quaternion.cpp:35-52) for points p [n][3]: [n][3][4]."""
    w, v = q[0], np.asarray(q[1:], np.float64)
    p = np.asarray(p, np.float64).reshape(-1, 3)
    out = np.zeros((len(p), 3, 4))
    out[:, :, 0] = 2.0 * (w * p + np.cross(v[None, :], p))
    vp = p @ v
    for r in range(3):
        for c in range(3):
            hat = 0.0 if r == c else (1.0 if (c - r) % 3 == 2 else -1.0) * p[:, 3 - r - c]      # Hat(p)[r][c]
            out[:, r, 1 + c] = 2.0 * ((vp if r == c else 0.0) + v[r] * p[:, c] - p[:, r] * v[c] - w * hat)
    return out


def pair_rows(X, Y, pose):
    """AlignmentProblem::Make (alignment.cpp:33-78): residual pose * x - y, Jacobian [DRpDq(q, x), I]; r3 [n][3], J3 [n][21]."""
    X, Y = np.asarray(X, np.float64).reshape(-1, 3), np.asarray(Y, np.float64).reshape(-1, 3)
    P = np.asarray(pose, np.float64).reshape(3, 4)
    J = np.zeros((len(X), 3, 7))
    J[:, :, :4] = drp_dq(quaternion_of(P[:, :3]), X)
    J[:, :, 4:] = np.eye(3)[None]
    r = np.stack([P[i, 0] * X[:, 0] + P[i, 1] * X[:, 1] + P[i, 2] * X[:, 2] + P[i, 3] - Y[:, i] for i in range(3)], 1)
    return r, J.reshape(len(X), 21)


def pose_of(q, t):
    """The 3 x 4 pose of (q, t) in the order of operations of the library's refresh_pose (Eigen's toRotationMatrix)."""
    w, x, y, z = (float(a) for a in q)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy, t[0]], [txy + twz, 1.0 - (txx + tzz), tyz - twx, t[1]],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy), t[2]]], np.float64)


def exact_sums(J, r, w_rows):
    """D = sum J^T J, A = sum w J^T J, b = sum w J^T r over the 1 x 7 rows: every entry the exactly rounded sum (math.fsum) of
    its products."""
    D, A, b = np.zeros((7, 7)), np.zeros((7, 7)), np.zeros(7)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        wJ = J * w_rows[:, None]
        for a in range(7):
            for c in range(a, 7):
                D[a, c] = D[c, a] = math.fsum((J[:, a] * J[:, c]).tolist())
                A[a, c] = A[c, a] = math.fsum((wJ[:, a] * J[:, c]).tolist())
            b[a] = math.fsum((wJ[:, a] * r).tolist())
    return D, A, b


def restate_step(pose, r3, J3, r1=(), J1=(), max_iter=1):
    """One call of the optimizer with `max_iter` = 1 on the rows (r3 [n3][3], J3 [n3][21], r1 [n1], J1 [n1][7]) of a scan at
    `pose` (3 x 4).  Returns a dict: pose, error, error_scale, code, iteration (what the entry points return), and beside
    them dq, dt, dx_norm, cond (cond2 of H), rows, bound (B), pose_bound, degenerate, weights, errors, near_threshold,
    min_eigenvalue_d, near_degenerate, near_convergence, excluded (any of the three)."""
    assert max_iter == 1
    P = np.asarray(pose, np.float64).reshape(3, 4)
    r3 = np.asarray(r3, np.float64).reshape(-1, 3)
    J3 = np.asarray(J3, np.float64).reshape(-1, 7)
    r1 = np.asarray(r1, np.float64).reshape(-1)
    J1 = np.asarray(J1, np.float64).reshape(-1, 7)
    n3, n1 = len(r3), len(r1)
    q = quaternion_of(P[:, :3])
    t = P[:, 3].copy()
    out = dict(pose=pose_of(q, t), error=0.0, error_scale=0.0, iteration=0, rows=3 * n3 + n1, dq=np.array([1.0, 0, 0, 0]),
               dt=np.zeros(3), dx_norm=0.0, cond=1.0, bound=0.0, degenerate=False, near_threshold=False, near_degenerate=False,
               near_convergence=False, excluded=False, min_eigenvalue_d=float("nan"), weights=np.zeros(0), errors=np.zeros(0))
    out["pose_bound"] = 16 * U * (1.0 + np.abs(out["pose"]).max())
    if n3 + n1 == 0:
        out["code"] = EMPTY
        return out
    if n1 and not J1[:, 4:7].any():
        out["code"] = NO_PLANE
        return out
    e = errors_of(r3, r1)
    error, scale = math.fsum(e.tolist()), scale_sorted(e)
    out.update(error=error, error_scale=scale, errors=e)
    if error > DBL_MAX:                                        # LargerErrorThanPrevious against numeric_limits::max()
        out["code"] = LARGER_ERROR
        return out
    if scale > DBL_MAX:
        out["code"] = LARGER_SCALE
        return out
    k2 = HUBER_K * HUBER_K
    with np.errstate(over="ignore", divide="ignore"):
        en = e / (scale + 1e-16)
        inlier = en < k2
        w = np.where(inlier, 1.0, HUBER_K / np.sqrt(np.where(inlier, 1.0, en)))
    out["weights"] = w
    out["near_threshold"] = bool((np.abs(en - k2) <= 1e-6 * k2).any())
    J = np.vstack([J3, J1])
    r = np.concatenate([r3.reshape(-1), r1])
    w_rows = np.concatenate([np.repeat(w[:n3], 3), w[n3:]])
    D, A, b = exact_sums(J, r, w_rows)
    lam = np.linalg.eigvalsh(D)
    out["D"] = D
    out["min_eigenvalue_d"] = float(lam[0])
    out["near_degenerate"] = bool(abs(lam[0] - 0.1) <= 1e-6 * lam[-1])
    out["degenerate"] = bool(np.abs(lam).min() < 0.1)           # IsDegenerate (degenerate.cpp:32-37)
    dx = np.zeros(6)
    if not out["degenerate"]:
        M = make_m(q)
        H, g = M.T @ A @ M, M.T @ b
        H = 0.5 * (H + H.T)
        dx = -np.linalg.solve(H, g)
        out["cond"] = float(np.linalg.cond(H))
    k = math.sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2])  # AngleAxisToQuaternion, posevec.cpp:32-45
    if k < 1e-8:
        dq = np.array([1.0, 0.0, 0.0, 0.0])
    else:
        dq = np.array([math.cos(k / 2.0)] + [(dx[a] / k) * math.sin(k / 2.0) for a in range(3)])
    dt = dx[3:].copy()
    qn = np.array([q[0] * dq[0] - q[1] * dq[1] - q[2] * dq[2] - q[3] * dq[3],
                   q[0] * dq[1] + q[1] * dq[0] + q[2] * dq[3] - q[3] * dq[2],
                   q[0] * dq[2] + q[2] * dq[0] + q[3] * dq[1] - q[1] * dq[3],
                   q[0] * dq[3] + q[3] * dq[0] + q[1] * dq[2] - q[2] * dq[1]])
    new = pose_of(qn, t + dt)
    nq, nt = float(np.linalg.norm(dq[1:])), float(np.linalg.norm(dt))
    converged = nq < 1e-3 and nt < 1e-3                         # CheckConvergence (optimizer.cpp:35-38)
    dx_norm = float(np.linalg.norm(dx))
    bound = (out["rows"] + 64) * U * out["cond"] * dx_norm
    out.update(pose=new, dq=dq, dt=dt, dx_norm=dx_norm, bound=bound, code=CONVERGED if converged else MAX_ITERATION,
               iteration=0 if converged else max_iter, near_convergence=bool(abs(nq - 1e-3) <= 1e-9 or abs(nt - 1e-3) <= 1e-9),
               pose_bound=bound * (1.0 + np.abs(new[:, 3]).max()) + 16 * U * (1.0 + np.abs(new).max()))
    out["excluded"] = out["near_threshold"] or out["near_degenerate"] or out["near_convergence"]
    return out
