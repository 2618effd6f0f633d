"""The de-skew section of include/lfx.h restated in numpy float64, in the header's order of operations (no reference
counterpart: the project defines the operation, this pins it).  Nothing here calls the library."""
import numpy as np

IDENTITY = np.eye(4)[:3].copy()


def exp_so3(w):
    """Rodrigues: the rotation of an angle-axis vector."""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / (th * th) * (K @ K)


def pose(w, t):
    return np.ascontiguousarray(np.hstack([exp_so3(w), np.asarray(t, np.float64).reshape(3, 1)]))


def compose(a, b):
    """a b for 3 x 4 poses."""
    a, b = np.asarray(a, np.float64).reshape(3, 4), np.asarray(b, np.float64).reshape(3, 4)
    return np.hstack([a[:, :3] @ b[:, :3], (a[:, :3] @ b[:, 3] + a[:, 3]).reshape(3, 1)])


def apply(p, x):
    """pose p applied to points x [n, 3] (float64)."""
    p = np.asarray(p, np.float64).reshape(3, 4)
    return np.asarray(x, np.float64) @ p[:, :3].T + p[:, 3]


def between(pose0, pose1):
    """lfx_motion_between: pose0^-1 pose1, every 3-term sum (a0 b0 + a1 b1) + a2 b2."""
    a, b = np.asarray(pose0, np.float64).reshape(3, 4), np.asarray(pose1, np.float64).reshape(3, 4)
    if np.array_equal(a, b):
        return IDENTITY.copy()
    out = np.zeros((3, 4))
    for r in range(3):
        inv_t = -((a[0, r] * a[0, 3] + a[1, r] * a[1, 3]) + a[2, r] * a[2, 3])
        out[r, 3] = ((a[0, r] * b[0, 3] + a[1, r] * b[1, 3]) + a[2, r] * b[2, 3]) + inv_t
        for c in range(3):
            out[r, c] = (a[0, r] * b[0, c] + a[1, r] * b[1, c]) + a[2, r] * b[2, c]
    return out


def twist(motion):
    """lfx_motion_twist: (w, theta) -- the quaternion of the matrix as lfx_pose_diff states it, theta = 2 atan2(|vec|, q_w)."""
    m = np.asarray(motion, np.float64).reshape(3, 4)
    q = np.zeros(3)
    tr = (m[0, 0] + m[1, 1]) + m[2, 2]
    if tr > 0.0:
        t = np.sqrt(tr + 1.0)
        qw = 0.5 * t
        s = 0.5 / t
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * s, (m[0, 2] - m[2, 0]) * s, (m[1, 0] - m[0, 1]) * s
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(((m[i, i] - m[j, j]) - m[k, k]) + 1.0)
        q[i] = 0.5 * t
        s = 0.5 / t
        qw = (m[k, j] - m[j, k]) * s
        q[j], q[k] = (m[j, i] + m[i, j]) * s, (m[k, i] + m[i, k]) * s
    n = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
    if n == 0.0:
        return np.zeros(3), 0.0
    th = 2.0 * np.arctan2(n, qw)
    return q * (th / n), float(th)


def scale(motion, ratio):
    """lfx_motion_scale: [Exp(ratio w) | ratio t]."""
    m = np.asarray(motion, np.float64).reshape(3, 4)
    w, th = twist(m)
    out = np.zeros((3, 4))
    if th < 1e-8:
        x, y, z = ratio * w
        out[:, :3] = [[1.0, 0.0 - z, y], [z, 1.0, 0.0 - x], [0.0 - y, x, 1.0]]
    else:
        k = w / th
        a = ratio * th
        c, s = np.cos(a), np.sin(a)
        hat = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
        for i in range(3):
            for j in range(3):
                out[i, j] = ((c if i == j else 0.0) + hat[i, j] * s) + k[i] * (k[j] * (1.0 - c))
    out[:, 3] = ratio * m[:, 3]
    return out


def alpha_from_index(index, n_points):
    return np.asarray(index, np.float64) / np.float64(n_points)


def alpha_from_time(value, scale_, t0, t1):
    """value: the field as stored (any dtype); t = (double)value * scale; alpha = (t - t0) * (1 / (t1 - t0))."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(value).astype(np.float64) * np.float64(scale_) - np.float64(t0)) * (np.float64(1.0) / (np.float64(t1) - np.float64(t0)))


def deskew(records, alpha, motion, to_end):
    """records [n, 4] float32, alpha [n] float64 -> [n, 4] float32, the header's arithmetic step by step."""
    rec = np.asarray(records, np.float32).reshape(-1, 4)
    alpha = np.asarray(alpha, np.float64)
    m = np.asarray(motion, np.float64).reshape(3, 4)
    w, theta = twist(m)
    v, R = m[:, 3], m[:, :3]
    px, py, pz = (rec[:, i].astype(np.float64) for i in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        if theta < 1e-8:
            rx = px + alpha * (w[1] * pz - w[2] * py)
            ry = py + alpha * (w[2] * px - w[0] * pz)
            rz = pz + alpha * (w[0] * py - w[1] * px)
        else:
            k = w / theta
            a = alpha * theta
            c, s = np.cos(a), np.sin(a)
            cx, cy, cz = k[1] * pz - k[2] * py, k[2] * px - k[0] * pz, k[0] * py - k[1] * px
            g = ((k[0] * px + k[1] * py) + k[2] * pz) * (1.0 - c)
            rx = (px * c + cx * s) + k[0] * g
            ry = (py * c + cy * s) + k[1] * g
            rz = (pz * c + cz * s) + k[2] * g
        mx, my, mz = rx + alpha * v[0], ry + alpha * v[1], rz + alpha * v[2]
        if to_end:
            u0, u1, u2 = mx - v[0], my - v[1], mz - v[2]
            res = [(R[0, i] * u0 + R[1, i] * u1) + R[2, i] * u2 for i in range(3)]
        else:
            res = [mx, my, mz]
        out = rec.copy()
        ok = np.isfinite(alpha)
        for i in range(3):
            out[ok, i] = res[i][ok].astype(np.float32)
    return out
