#!/usr/bin/env python3
"""An independent reference for the scan-to-map rows (include/lfx.h, lfx_scan_to_map_residuals), computed with mpmath at
50 digits and written to tests/golden/row_reference.json.

The row is restated literally: q = R p + t; the quaternion of R by the branch rule of Eigen::Quaterniond(Matrix3d) (trace
> 0, else the largest diagonal entry, the first one on a tie), which fixes its sign; DRpDq; for an EDGE row the mean and
covariance of the k neighbours, the eigenvalues l1 >= l2 >= l3 and the top eigenvector u (mpmath.eigsy), kappa = l1 /
(l1 - l2), p1 / p2 = mean -/+ u, the Jacobian [Hat(p2 - p1) DRpDq | Hat(p2 - p1)] and the residual (q - p1) x (q - p2);
for a SURFACE row the least-squares solution w of X w = -1 (the normal equations, at 50 digits), the singular values of X
(mpmath.svd_r), u = w / |w|, the Jacobian [u^T DRpDq | u^T] and the residual (w . q + 1) / |w|; the zero row where the
diagonal of X's triangular factor has a ratio of 1e-9 or less (the no-plane rule).  For every entry the sum of the absolute
values of its terms is computed alongside.  edge_row(..., u=...) evaluates an edge row with a given u in the eigenvector's
place.

The inputs are float32 map points, the neighbours' indices in order of distance, the float32 scan point and the pose as 12
doubles; the cases are those of tests/row_cases.py, whose clusters are made from integers; the poses are made here
(Rodrigues' formula at 50 digits, rounded once).  The file holds numbers only: the inputs (float32 as the 8 hex digits of
their bits, doubles as hex floats) and what takes a root to compute (tests/row_cases.py evaluates the rest exactly, in
rational arithmetic; tests/test_row_reference_expect.py checks that evaluation against this one).

    python tools/row_reference.py            writes the file
    python tools/row_reference.py --check    compares the file with what would be written"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import row_cases as K  # noqa: E402

import numpy as np  # noqa: E402

DIGITS = 50


def _mp():
    import mpmath
    mpmath.mp.dps = DIGITS
    return mpmath


# ------------------------------------------------------------------------------------------------ the row, restated
def make_pose(mp, name):
    """[R | t] as 12 doubles: Rodrigues' formula at 50 digits, every entry rounded once"""
    axis, angle, t = K.POSES[name]
    if name == "turn_111":
        R = [[0., 0., 1.], [1., 0., 0.], [0., 1., 0.]]                       # 120 degrees about (1, 1, 1), exactly
    elif name == "turn_1m10":
        R = [[0., -1., 0.], [-1., 0., 0.], [0., 0., -1.]]                     # 180 degrees about (1, -1, 0), exactly
    elif axis is None:
        R = [[1., 0., 0.], [0., 1., 0.], [0., 0., 1.]]
    else:
        th = mp.mpf(angle[:-3]) * mp.pi / 180 if angle.endswith("deg") else mp.mpf(angle)
        n = mp.sqrt(sum(mp.mpf(a) ** 2 for a in axis))
        a = [mp.mpf(v) / n for v in axis]
        ax = mp.matrix([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        M = mp.eye(3) + mp.sin(th) * ax + (1 - mp.cos(th)) * (ax * ax)
        R = [[float(M[r, c]) for c in range(3)] for r in range(3)]
    return [v for r in range(3) for v in R[r] + [float(t[r])]]


def quaternion(mp, pose):
    """(w, x, y, z) of the pose's rotation by the branches of Eigen::Quaterniond(Matrix3d)"""
    M = lambda r, c: mp.mpf(pose[4 * r + c])  # noqa: E731
    t = M(0, 0) + M(1, 1) + M(2, 2)
    q = [None] * 3
    if t > 0:
        t = mp.sqrt(t + 1)
        w = t / 2
        t = 1 / (2 * t)
        q = [(M(2, 1) - M(1, 2)) * t, (M(0, 2) - M(2, 0)) * t, (M(1, 0) - M(0, 1)) * t]
    else:
        i = 0
        if M(1, 1) > M(0, 0):
            i = 1
        if M(2, 2) > M(i, i):
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = mp.sqrt(M(i, i) - M(j, j) - M(k, k) + 1)
        q[i] = t / 2
        t = 1 / (2 * t)
        w = (M(k, j) - M(j, k)) * t
        q[j] = (M(j, i) + M(i, j)) * t
        q[k] = (M(k, i) + M(i, k)) * t
    return [w] + q


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def hat(e):
    return [[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]]


def transform(mp, pose, p):
    """q = R p + t and the sums of the absolute values of its terms"""
    P, p = [mp.mpf(v) for v in pose], [mp.mpf(float(v)) for v in p]
    q = [P[4 * r] * p[0] + P[4 * r + 1] * p[1] + P[4 * r + 2] * p[2] + P[4 * r + 3] for r in range(3)]
    a = [abs(P[4 * r] * p[0]) + abs(P[4 * r + 1] * p[1]) + abs(P[4 * r + 2] * p[2]) + abs(P[4 * r + 3]) for r in range(3)]
    return q, a


def drp_dq(mp, quat, p):
    """rotationlib::DRpDq (3 x 4): [2 (w p + v x p) | 2 (v.p I + v p^T - p v^T - w Hat(p))], and each entry's term sum"""
    w, v, p = quat[0], quat[1:], [mp.mpf(float(x)) for x in p]
    vxp, vp, Kp = cross(v, p), sum(v[i] * p[i] for i in range(3)), hat(p)
    vxpa = [abs(v[1] * p[2]) + abs(v[2] * p[1]), abs(v[2] * p[0]) + abs(v[0] * p[2]), abs(v[0] * p[1]) + abs(v[1] * p[0])]
    vpa = sum(abs(v[i] * p[i]) for i in range(3))
    d, a = [[0] * 4 for _ in range(3)], [[0] * 4 for _ in range(3)]
    for r in range(3):
        d[r][0], a[r][0] = 2 * (w * p[r] + vxp[r]), 2 * (abs(w * p[r]) + vxpa[r])
        for c in range(3):
            d[r][1 + c] = 2 * ((vp if r == c else 0) + v[r] * p[c] - p[r] * v[c] - w * Kp[r][c])
            a[r][1 + c] = 2 * ((vpa if r == c else 0) + abs(v[r] * p[c]) + abs(p[r] * v[c]) + abs(w * Kp[r][c]))
    return d, a


def edge_row(mp, nb, p0, pose, u=None):
    """nb: the neighbours [k][3] in order.  u given: it stands in for the eigenvector (and kappa is not computed)."""
    k = len(nb)
    X = [[mp.mpf(float(v)) for v in p] for p in nb]
    mean = [sum(x[i] for x in X) / k for i in range(3)]
    mean_abs = [sum(abs(x[i]) for x in X) / k for i in range(3)]
    out = dict(mean=mean)
    if u is None:
        cov = mp.matrix(3, 3)
        for a in range(3):
            for b in range(3):
                cov[a, b] = sum((x[a] - mean[a]) * (x[b] - mean[b]) for x in X) / k
        E, Q = mp.eigsy(cov)
        lam = sorted(((E[i], i) for i in range(3)), key=lambda t: t[0])
        l1, l2, l3 = lam[2][0], lam[1][0], lam[0][0]
        top = [Q[r, lam[2][1]] for r in range(3)]
        n = mp.sqrt(sum(v * v for v in top))
        top = [v / n for v in top]
        tiny = mp.mpf(10) ** (-(DIGITS - 10)) * (abs(l1) + 1)
        out.update(cov=cov, eigenvalues=(l1, l2, l3), fallback=bool(l1 - l3 <= tiny))
        if out["fallback"]:
            top = [mp.mpf(0), mp.mpf(0), mp.mpf(1)]                         # the isotropic neighbourhood's row
            out["kappa"] = mp.mpf(0)
        else:
            assert l1 - l2 > tiny, "l1 = l2 > l3: the direction is not defined"
            out["kappa"] = l1 / (l1 - l2)
        u = top
    else:
        u = [mp.mpf(float(v)) for v in u]
    q, qa = transform(mp, pose, p0)
    p1, p2 = [mean[i] - u[i] for i in range(3)], [mean[i] + u[i] for i in range(3)]
    a, b = [q[i] - p1[i] for i in range(3)], [q[i] - p2[i] for i in range(3)]
    s = [qa[i] + mean_abs[i] + abs(u[i]) for i in range(3)]
    res = cross(a, b)
    rs = []
    for i in range(3):
        j, l = (i + 1) % 3, (i + 2) % 3
        rs.append(s[j] * abs(b[l]) + abs(a[j]) * s[l] + s[l] * abs(b[j]) + abs(a[l]) * s[j] + abs(a[j] * b[l]) + abs(a[l] * b[j]))
    d, da = drp_dq(mp, quaternion(mp, pose), p0)
    Kh = hat([p2[i] - p1[i] for i in range(3)])
    J, Js = [], []
    for r in range(3):
        J += [sum(Kh[r][t] * d[t][c] for t in range(3)) for c in range(4)] + [Kh[r][c] for c in range(3)]
        Js += [sum(abs(Kh[r][t]) * da[t][c] for t in range(3)) for c in range(4)] + [mp.mpf(0)] * 3
    out.update(u=u, q=q, residual=res, residual_scale=rs, jacobian=J, jacobian_scale=Js)
    return out


def triangular_diagonal(mp, X):
    """|R_cc| of X = Q R (unpivoted; Gram-Schmidt at 50 digits: the magnitudes are those of the Householder factor)"""
    cols = [[X[r][c] for r in range(len(X))] for c in range(3)]
    basis, diag = [], []
    for c in range(3):
        v = list(cols[c])
        for b in basis:
            s = sum(x * y for x, y in zip(b, v))
            v = [x - s * y for x, y in zip(v, b)]
        n = mp.sqrt(sum(x * x for x in v))
        diag.append(n)
        basis.append([x / n for x in v] if n > 0 else [mp.mpf(0)] * len(v))
    return diag


def surface_row(mp, nb, p0, pose):
    k = len(nb)
    X = [[mp.mpf(float(v)) for v in p] for p in nb]
    diag = triangular_diagonal(mp, X)
    ratio = min(diag) / max(diag) if max(diag) > 0 else mp.mpf(0)
    out = dict(pivot_ratio=ratio, zero=not ratio > mp.mpf("1e-9"))
    if out["zero"]:
        return out
    A = mp.matrix(X)
    w = mp.lu_solve(A.T * A, A.T * mp.matrix([-1] * k))
    w = [w[i] for i in range(3)]
    sv = sorted(mp.svd_r(A, compute_uv=False))
    norm_w = mp.sqrt(sum(v * v for v in w))
    fit = mp.sqrt(sum((sum(X[r][c] * w[c] for c in range(3)) + 1) ** 2 for r in range(k)))
    kx = sv[2] / sv[0]
    u = [v / norm_w for v in w]
    q, qa = transform(mp, pose, p0)
    d, da = drp_dq(mp, quaternion(mp, pose), p0)
    J = [sum(u[t] * d[t][c] for t in range(3)) for c in range(4)] + u
    Js = [sum(da[t][c] for t in range(3)) for c in range(4)] + [mp.mpf(1)] * 3
    out.update(w=w, singular_values=sv, u=u, q=q, condition=kx + kx * kx * fit / (sv[2] * norm_w), inv_norm_w=1 / norm_w,
               residual=(sum(w[i] * q[i] for i in range(3)) + 1) / norm_w, residual_scale=sum(qa) + 1 / norm_w, jacobian=J, jacobian_scale=Js)
    return out


# ------------------------------------------------------------------------------------------------ the cases
def scan_point(pose, target):
    """the float32 scan point whose image under the pose lies at (about) `target`: R^T (target - t), plain double sums"""
    d = [target[r] - pose[4 * r + 3] for r in range(3)]
    return [float(np.float32(pose[c] * d[0] + pose[4 + c] * d[1] + pose[8 + c] * d[2])) for c in range(3)]


def hexes(values):
    return [float.hex(float(v)) for v in values]


def short(v):
    return "%.6e" % float(v)


def build(mp):
    poses = {n: make_pose(mp, n) for n in K.POSES}
    doc = dict(about="tools/row_reference.py: the scan-to-map rows at %d digits, rounded once; float32 as hex bits, doubles as hex floats; "
                     "rows: name, family, map, pose, k, first point, scan point, expected (edge: u, kappa, fallback; surface: zero, u, "
                     "residual, 1/|w|, condition factor)" % DIGITS,
               poses={n: hexes(p) + hexes(quaternion(mp, p)) for n, p in poses.items()})
    for kind, key, clusters in ((K.EDGE, "edge", K.edge_clusters()), (K.SURFACE, "surface", K.surface_clusters())):
        maps, placed = {}, []
        for c in clusters:
            name, family, group, pts, target, cposes = c[:6]
            at = maps.setdefault(group, [])
            if kind == K.EDGE:
                i, o = len([p for p in placed if p[2] == group]), K.EDGE_ORIGIN[group]
                centre = [o[0] + K.SPACING * (i % 6), o[1] + K.SPACING * (i // 6), o[2]]
                pts = [[p[a] + centre[a] for a in range(3)] for p in pts]
                target = [target[a] + centre[a] for a in range(3)]
            placed.append((name, family, group, len(at), len(pts), target, cposes, c[6] if kind == K.SURFACE else None))
            at.extend(pts)
        maps = {g: np.asarray(p, np.float32) for g, p in maps.items()}
        rows = []
        for name, family, group, first, k, target, cposes, zero in placed:
            for pn in cposes:
                p0 = scan_point(poses[pn], target)
                q, _ = K.query_of(poses[pn], p0)
                got, kth, nxt = K.nearest_exact(maps[group], q, k)
                assert sorted(got) == list(range(first, first + k)), (name, pn, got)
                assert nxt is None or nxt > 16 * kth or kth == 0, (name, pn, float(kth), float(nxt))
                nb = maps[group][got]
                if kind == K.EDGE:
                    r = edge_row(mp, nb, p0, poses[pn])
                    e = hexes(r["u"]) + [short(r["kappa"]), int(r["fallback"])]
                else:
                    r = surface_row(mp, nb, p0, poses[pn])
                    assert r["zero"] == zero and (r["pivot_ratio"] < mp.mpf("1e-10") or r["pivot_ratio"] > mp.mpf("1e-8")), (name, r["pivot_ratio"])
                    e = [1] if r["zero"] else [0] + hexes(r["u"]) + [float.hex(float(r["residual"])), short(r["inv_norm_w"]), short(r["condition"])]
                rows.append([name, family, group, pn, k, first, K.f32_hex(p0), e])
        doc[key + "_maps"] = {g: K.f32_hex(p) for g, p in maps.items()}
        doc[key + "_rows"] = rows
    ties = []
    for kind, pts in ((K.EDGE, K.TIE_POINTS), (K.SURFACE, K.TIE_SURFACE_POINTS)):
        for rev in (0, 1):
            m = np.asarray(pts[::-1] if rev else pts, np.float32)
            q, _ = K.query_of(poses["identity"], K.TIE_QUERY)
            got, kth, nxt = K.nearest_exact(m, q, K.TIE_K)
            assert kth == nxt and got[-1] == (0 if rev else 4), (got, kth, nxt)
            if kind == K.EDGE:
                r = edge_row(mp, m[got], K.TIE_QUERY, poses["identity"])
                e = hexes(r["u"]) + [short(r["kappa"]), int(r["fallback"])]
            else:
                r = surface_row(mp, m[got], K.TIE_QUERY, poses["identity"])
                e = [0] + hexes(r["u"]) + [float.hex(float(r["residual"])), short(r["inv_norm_w"]), short(r["condition"])]
            ties.append([kind, rev, K.f32_hex(m), K.TIE_K, K.f32_hex(K.TIE_QUERY), got, e])
    doc["ties"] = ties
    return doc


def text():
    """the file's contents: one line per map and per row"""
    doc = build(_mp())
    js = lambda v: json.dumps(v, separators=(",", ":"))  # noqa: E731
    out = ["{", ' "about":%s,' % json.dumps(doc["about"]), ' "poses":{']
    out += ["  %s:%s%s" % (json.dumps(n), js(v), "," if i + 1 < len(doc["poses"]) else "") for i, (n, v) in enumerate(doc["poses"].items())]
    out.append(" },")
    for key in ("edge", "surface"):
        m = doc[key + "_maps"]
        out.append(' "%s_maps":{' % key)
        out += ["  %s:%s%s" % (json.dumps(g), js(v), "," if i + 1 < len(m) else "") for i, (g, v) in enumerate(m.items())]
        out.append(" },")
        rows = doc[key + "_rows"]
        out.append(' "%s_rows":[' % key)
        out += ["  %s%s" % (js(r), "," if i + 1 < len(rows) else "") for i, r in enumerate(rows)]
        out.append(" ],")
    out.append(' "ties":[')
    out += ["  %s%s" % (js(r), "," if i + 1 < len(doc["ties"]) else "") for i, r in enumerate(doc["ties"])]
    out += [" ]", "}"]
    return "\n".join(out) + "\n"


def main(argv):
    if "--check" in argv:
        with open(K.PATH) as f:
            same = f.read() == text()
        print("the file is what this tool writes" if same else "the file differs from what this tool writes")
        return 0 if same else 1
    with open(K.PATH, "w") as f:
        f.write(text())
    print("wrote", K.PATH)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
