"""The trajectory part of include/lfx.h's de-skew section restated in numpy float64, in the header's order of operations, on
top of tests/deskew_restatement.py (no reference counterpart: the project defines the operation, this pins it).  Nothing here
calls the library."""
import numpy as np

from tests import deskew_restatement as R

K, THETA, W, A, Q, DQ, TIME, INV_DT, STRIDE = 0, 3, 4, 7, 16, 19, 22, 23, 24


def segment_of(times, t):
    """j = clamp(#{knots with times[k] <= t} - 1, 0, n_knots - 2); t may be an array (a NaN counts no knot)."""
    times = np.asarray(times, np.float64)
    with np.errstate(invalid="ignore"):
        count = (times[None, :] <= np.asarray(t, np.float64).reshape(-1, 1)).sum(axis=1)
    j = np.clip(count - 1, 0, len(times) - 2)
    return j if np.ndim(t) else int(j[0])


def rotate(a, b):
    """The rotation of pose a times that of b, every sum (a0 b0 + a1 b1) + a2 b2."""
    out = np.zeros((3, 3))
    for r in range(3):
        for c in range(3):
            out[r, c] = (a[r, 0] * b[0, c] + a[r, 1] * b[1, c]) + a[r, 2] * b[2, c]
    return out


def reference_pose(times, poses, t_ref):
    """P_ref: the knot's pose itself where t_ref is a knot time, else the model's pose at t_ref in the helpers' arithmetic."""
    times = np.asarray(times, np.float64)
    P = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    hit = np.nonzero(times == t_ref)[0]
    if len(hit):
        return P[hit[0]].copy()
    j = segment_of(times, t_ref)
    beta = (np.float64(t_ref) - times[j]) * (np.float64(1.0) / (times[j + 1] - times[j]))
    S = R.scale(R.between(P[j], P[j + 1]), beta)
    out = np.zeros((3, 4))
    out[:, :3] = rotate(P[j], S)
    out[:, 3] = P[j, :, 3] + beta * (P[j + 1, :, 3] - P[j, :, 3])
    return out


def segments(times, poses, t_ref):
    """lfx_trajectory_segments: [n_knots - 1][24], the header's columns."""
    times = np.asarray(times, np.float64)
    P = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    ref = reference_pose(times, P, t_ref)
    Qs = [R.between(ref, p) for p in P]
    out = np.zeros((len(times) - 1, STRIDE))
    for j in range(len(times) - 1):
        w, theta = R.twist(R.between(Qs[j], Qs[j + 1]))
        out[j, K:K + 3] = 0.0 if theta < 1e-8 else w / theta
        out[j, THETA] = theta
        out[j, W:W + 3] = w
        out[j, A:A + 9] = Qs[j][:, :3].reshape(9)
        out[j, Q:Q + 3] = Qs[j][:, 3]
        out[j, DQ:DQ + 3] = Qs[j + 1][:, 3] - Qs[j][:, 3]
        out[j, TIME] = times[j]
        out[j, INV_DT] = np.float64(1.0) / (times[j + 1] - times[j])
    return out


def time_from_index(index, n_points):
    return np.asarray(index, np.float64) / np.float64(n_points)


def time_from_field(value, scale_):
    """value: the field as stored (any dtype); t = (double)value * scale."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(value).astype(np.float64) * np.float64(scale_)


def deskew(records, t, times, poses, t_ref):
    """records [n, 4] float32, their times t [n] float64 -> [n, 4] float32: the device arithmetic step by step."""
    rec = np.asarray(records, np.float32).reshape(-1, 4)
    t = np.asarray(t, np.float64).reshape(-1)
    T = segments(times, poses, t_ref)
    j = segment_of(times, t)
    S = T[j]
    px, py, pz = (rec[:, i].astype(np.float64) for i in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        beta = (t - S[:, TIME]) * S[:, INV_DT]
        theta = S[:, THETA]
        w, k = S[:, W:W + 3], S[:, K:K + 3]
        # the small-angle form
        sx = px + beta * (w[:, 1] * pz - w[:, 2] * py)
        sy = py + beta * (w[:, 2] * px - w[:, 0] * pz)
        sz = pz + beta * (w[:, 0] * py - w[:, 1] * px)
        # the general one
        a = beta * theta
        c, s = np.cos(a), np.sin(a)
        cx, cy, cz = k[:, 1] * pz - k[:, 2] * py, k[:, 2] * px - k[:, 0] * pz, k[:, 0] * py - k[:, 1] * px
        g = ((k[:, 0] * px + k[:, 1] * py) + k[:, 2] * pz) * (1.0 - c)
        small = theta < 1e-8
        r = [np.where(small, sx, (px * c + cx * s) + k[:, 0] * g), np.where(small, sy, (py * c + cy * s) + k[:, 1] * g),
             np.where(small, sz, (pz * c + cz * s) + k[:, 2] * g)]
        out = rec.copy()
        ok = np.isfinite(beta)
        for i in range(3):
            v = ((S[:, A + 3 * i] * r[0] + S[:, A + 3 * i + 1] * r[1]) + S[:, A + 3 * i + 2] * r[2]) + (S[:, Q + i] + beta * S[:, DQ + i])
            out[ok, i] = v[ok].astype(np.float32)
    return out


def from_gyro(times, rates, bias=None, velocity=None):
    """lfx_trajectory_from_gyro: [n][3][4]."""
    times = np.asarray(times, np.float64)
    rates = np.asarray(rates, np.float64).reshape(-1, 3)
    b = np.zeros(3) if bias is None else np.asarray(bias, np.float64)
    out = np.zeros((len(times), 3, 4))
    out[0] = R.IDENTITY
    for j in range(len(times) - 1):
        phi = (0.5 * ((rates[j] - b) + (rates[j + 1] - b))) * (times[j + 1] - times[j])
        theta = np.sqrt((phi[0] * phi[0] + phi[1] * phi[1]) + phi[2] * phi[2])
        E = np.zeros((3, 3))
        if theta < 1e-8:
            x, y, z = phi
            E[:] = [[1.0, 0.0 - z, y], [z, 1.0, 0.0 - x], [0.0 - y, x, 1.0]]
        else:
            k = phi / theta
            c, s = np.cos(theta), np.sin(theta)
            hat = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
            for r in range(3):
                for q in range(3):
                    E[r, q] = ((c if r == q else 0.0) + hat[r, q] * s) + k[r] * (k[q] * (1.0 - c))
        out[j + 1, :, :3] = rotate(out[j], E)
        if velocity is not None:
            out[j + 1, :, 3] = np.asarray(velocity, np.float64) * (times[j + 1] - times[0])
    return out
