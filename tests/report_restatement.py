"""Test-side restatement of lfx_align_report in numpy (no GPU, nothing of the library): from the residual rows of a scan at
a pose -- as lfx_scan_to_map_residuals hands them out -- the weights of optimizer.cpp:100-128 (ComputeErrors,
NormalizeErrorScale with Scale = 1.4826 * MAD, HuberDerivative with k = 1.345), D = sum J^T J, A = sum w J^T J, the projection
H = M^T A M with M = MakeM(q) (optimizer.cpp:74-85), the eigen-decomposition, the floored covariance and the counts.
tests/test_align_report_gpu.py holds the device to it; tests/test_align_report.py pins covariance_ros_np's bits."""
import numpy as np

HUBER_K = 1.345
MAD_TO_SIGMA = 1.482602218505602
FLOOR = 1e-9


def quaternion_of(R):
    """Eigen::Quaterniond(Matrix3d) as (w, x, y, z): the branch on the trace, then on the largest diagonal entry."""
    R = np.asarray(R, np.float64)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1:] = [(R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t]
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[1 + i] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[k, j] - R[j, k]) * t
        q[1 + j] = (R[j, i] + R[i, j]) * t
        q[1 + k] = (R[k, i] + R[i, k]) * t
    return q


def make_m(q):
    """MakeM: [[0.5 * LeftMultiplicationMatrix(q)[:, 1:4], 0], [0, I]], 7 x 6."""
    w, x, y, z = q
    L = np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]])
    M = np.zeros((7, 6))
    M[:4, :3] = 0.5 * L[:, 1:4]
    M[4:, 3:] = np.eye(3)
    return M


def covariance_from(H, sigma2):
    """(eigenvalues ascending, eigenvectors as rows, floored covariance, rank) of a symmetric H."""
    lam, V = np.linalg.eigh(np.asarray(H, np.float64))
    floor = FLOOR * lam[5]
    cov = np.zeros((6, 6))
    for k in range(6):
        cov += np.outer(V[:, k], V[:, k]) * (sigma2 / max(lam[k], floor))
    return lam, V.T.copy(), cov, int((lam > floor).sum())


def restate(pose, edge_residual, edge_jacobian, surface_residual, surface_jacobian):
    """The report of one scan from its rows at `pose` (3 x 4): edge_residual [n3][3], edge_jacobian [n3][21],
    surface_residual [n1], surface_jacobian [n1][7].  Returns a dict with the record's fields plus D, near_threshold (a
    residual whose normalised error lies within 1e-6 k^2 of the Huber threshold: the inlier counts are then a matter of
    rounding) and the weights."""
    re = np.asarray(edge_residual, np.float64).reshape(-1, 3)
    Je = np.asarray(edge_jacobian, np.float64).reshape(-1, 7)
    rs = np.asarray(surface_residual, np.float64).reshape(-1)
    Js = np.asarray(surface_jacobian, np.float64).reshape(-1, 7)
    n3, n1 = len(re), len(rs)
    e = np.concatenate([(re * re).sum(1), rs * rs])
    median = np.median(e)
    scale = MAD_TO_SIGMA * np.median(np.abs(e - median))
    en = e / (scale + 1e-16)
    k2 = HUBER_K * HUBER_K
    inlier = en < k2
    w = np.where(inlier, 1.0, HUBER_K / np.sqrt(np.where(inlier, 1.0, en)))
    J = np.vstack([Je, Js])
    w_rows = np.concatenate([np.repeat(w[:n3], 3), w[n3:]])
    D = J.T @ J
    A = J.T @ (J * w_rows[:, None])
    M = make_m(quaternion_of(np.asarray(pose, np.float64).reshape(3, 4)[:, :3]))
    H = M.T @ A @ M
    H = 0.5 * (H + H.T)
    dim = 3.0 * w[:n3].sum() + w[n3:].sum() - 6.0
    sigma2 = (w * e).sum() / dim if dim > 0 else float("nan")
    lam, vec, cov, rank = covariance_from(H, sigma2)
    return dict(
        information=H, eigenvalues=lam, eigenvectors=vec, covariance=cov, rank=rank, sigma2=sigma2, D=D,
        min_eigenvalue_d=float(np.linalg.eigvalsh(0.5 * (D + D.T))[0]), error=float(e.sum()), error_scale=float(scale),
        rms_edge=float(np.sqrt(e[:n3].mean())) if n3 else 0.0, rms_surface=float(np.sqrt(e[n3:].mean())) if n1 else 0.0,
        n_edge=n3, n_surface=n1, n_edge_inliers=int(inlier[:n3].sum()), n_surface_inliers=int(inlier[n3:].sum()),
        n_surface_no_plane=int((~Js[:, 4:7].any(axis=1)).sum()) if n1 else 0,
        near_threshold=bool((np.abs(en - k2) <= 1e-6 * k2).any()), weights=w)


def covariance_ros_np(pose, covariance):
    """lfx_align_covariance_ros in numpy, in its order of operations: out = T C T^T, T = [[0, I], [R, 0]], every sum of three
    terms (a0 b0 + a1 b1) + a2 b2 in double, nothing fused."""
    P = np.asarray(pose, np.float64).reshape(3, 4)
    Cm = np.asarray(covariance, np.float64).reshape(6, 6)
    tc = np.zeros((6, 6))
    for i in range(3):
        tc[i] = Cm[3 + i]
        tc[3 + i] = (P[i, 0] * Cm[0] + P[i, 1] * Cm[1]) + P[i, 2] * Cm[2]
    out = np.zeros((6, 6))
    for j in range(3):
        out[:, j] = tc[:, 3 + j]
        out[:, 3 + j] = (tc[:, 0] * P[j, 0] + tc[:, 1] * P[j, 1]) + tc[:, 2] * P[j, 2]
    return out
