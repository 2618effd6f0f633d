"""What the tests of the edge and surface rows share (row_from_neighbours, lfx_kernels_localize.hpp): the cases, the
fixture tests/golden/row_reference.json that tools/row_reference.py writes from them at 50 digits, and the exact
(rational) evaluation of everything in a row that needs no root.

A CASE is one scan point against one small cluster of map points under one pose.  Every cluster has exactly k points and
lies in a map with the other clusters of its group, each far further from the others than its own radius, so the k
nearest map points of the case's query are the cluster: the tests assert that from exact distances and against
lfx_map_nearest.  The clusters are made from integers (a linear congruential generator and rational frames), rounded to
float32 once; the poses are made by the tool (correctly rounded), so the fixture can be written again byte for byte.

What the fixture holds beside the inputs is only what takes a root to compute: each pose's quaternion, an edge row's
principal direction and kappa = l1 / (l1 - l2), a surface row's unit normal, signed distance, 1 / |w| and condition
factor.  Everything else in a row -- the query R p + t, the mean, DRpDq, Hat(2 u) DRpDq, 2 u x (q - mean), and the sums of
the absolute values of the terms each entry is made of -- is rational in the inputs and is evaluated here with
fractions.Fraction: no rounding at all, so the device's u can be put in for the eigenvector without a second error."""
import json
import os
from fractions import Fraction as Fr

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_reference.json")
EPS = 2.0 ** -53
EDGE, SURFACE = 0, 1

# ---- what the device and the oracle are held to (the units: 2^-53 x the sum of the absolute values of the entry's terms
# for an edge row evaluated with the row's own u; 2^-53 x the condition factor x the entry's scale for a surface row).
# ORACLE_WORST: orc_loc_edge_residuals / orc_loc_surface_residuals measured on these cases (tests/test_row_reference_expect.py
# measures again and holds the figures); C = 8 x that: room for another order of summation, none for a wrong term.
ORACLE_WORST = {EDGE: 3.51, SURFACE: 0.78}
C_BOUND = {k: 8.0 * v for k, v in ORACLE_WORST.items()}


def direction_bound(kappa):
    """|sin(u_dev, u_ref)| allowed: 2^-53 (8 kappa + 4 kappa^2)"""
    return EPS * (8.0 * kappa + 4.0 * kappa * kappa)


class Lcg:
    """integers only: x <- (a x + c) mod 2^32; a value is the top 20 bits as a fraction in [-1, 1)"""

    def __init__(self, seed):
        self.x = seed & 0xFFFFFFFF

    def unit(self):
        self.x = (1664525 * self.x + 1013904223) & 0xFFFFFFFF
        return ((self.x >> 12) - (1 << 19)) / float(1 << 19)

    def vector(self, scale=1.0):
        return [scale * self.unit() for _ in range(3)]


# rational orthonormal frames (rows): of the quaternion (1, 2, 3, 4) / sqrt 30, of thirds, and the axes
TILT = [[-20 / 30., 4 / 30., 22 / 30.], [20 / 30., -10 / 30., 20 / 30.], [10 / 30., 28 / 30., 4 / 30.]]
THIRDS = [[1 / 3., 2 / 3., 2 / 3.], [2 / 3., 1 / 3., -2 / 3.], [2 / 3., -2 / 3., 1 / 3.]]
AXES = [[1., 0., 0.], [0., 1., 0.], [0., 0., 1.]]
H = 0.7071067811865476

# name: (axis or None, angle as text, translation); "turn_111" is the exact permutation matrix (trace 0, equal diagonal: every
# branch gives (1, 1, 1, 1) / 2 there, so it runs the tie but cannot tell which branch ran); "turn_1m10", the half turn about
# (1, -1, 0), is exact too: trace -1, M00 = M11 = 0 > M22, and x y < 0, so the branch of M00 gives (0, h, -h, 0) and the
# branch of M11 would give (0, -h, h, 0) -- the tie rule decides the sign of the four quaternion columns
POSES = {
    "identity": (None, "0", (0., 0., 0.)),
    "rot005": ((3., -2., 6.), "0.05", (0.125, -0.0625, 0.1875)),
    "x179": ((1., 0., 0.), "179deg", (0.5, -0.25, 0.125)),
    "y179": ((0., 1., 0.), "179deg", (0.5, -0.25, 0.125)),
    "z179": ((0., 0., 1.), "179deg", (0.5, -0.25, 0.125)),
    "turn_111": (None, "120deg", (0.25, 0.5, -0.125)),
    "turn_1m10": (None, "180deg", (-0.25, 0.125, 0.5)),
    "general": ((2., -1., 2.), "2.5", (30., -36., 18.)),                # |t| = 50.2
}
BASE = "rot005"
OTHER_POSES = ("identity", "x179", "y179", "z179", "turn_111", "turn_1m10", "general")


def _combine(frame, abc):
    """a e0 + b e1 + c e2 (e_i the frame's rows), plain double sums in a fixed order"""
    return [abc[0] * frame[0][i] + abc[1] * frame[1][i] + abc[2] * frame[2][i] for i in range(3)]


def _line(k, step, noise, seed, direction=(1 / 3., 2 / 3., 2 / 3.)):
    """k points along `direction`, `step` apart, centred; noise as a fraction of the line's length"""
    rng, length = Lcg(seed), step * (k - 1)
    out = []
    for j in range(k):
        t, n = step * (j - (k - 1) / 2.), rng.vector(noise * length)
        out.append([t * direction[i] + n[i] for i in range(3)])
    return out


def _disc(aspect, thick):
    """8 points on the ellipse (aspect cos, sin) in the plane of TILT's first two rows: l1 / l2 = aspect^2; thickness +-thick"""
    ring = [(1., 0.), (H, H), (0., 1.), (-H, H), (-1., 0.), (-H, -H), (0., -1.), (H, -H)]
    return [_combine(TILT, (aspect * c, s, thick * (1. if j % 2 == 0 else -1.))) for j, (c, s) in enumerate(ring)]


def edge_clusters():
    """[(name, family, group, local points, local target of the query, poses)]"""
    C = []
    add = lambda name, family, pts, target=(0.3, -0.2, 0.4), group="near", poses=(BASE,): C.append((name, family, group, pts, target, poses))  # noqa: E731
    add("k1", "k", [[0., 0., 0.]])
    add("k2", "k", [[-0.5, -1., 0.25], [0.5, 1., -0.25]])
    add("k3", "k", _line(3, 1.0, 1e-2, 11))
    add("k5", "k", _line(5, 0.5, 1e-2, 12), poses=(BASE,) + OTHER_POSES)
    add("k15", "k", _line(15, 0.25, 1e-2, 13))
    add("k16", "k", _line(16, 0.25, 1e-2, 14))
    add("iso_axes", "isotropic", [[s * (a == i) for a in range(3)] for i in range(3) for s in (1., -1.)], (0.125, 0.25, 0.375), poses=("identity", BASE))
    add("iso_cube", "isotropic", [[sx, sy, sz] for sx in (1., -1.) for sy in (1., -1.) for sz in (1., -1.)], (0.125, 0.25, 0.375), poses=("identity", BASE))
    for i, n in enumerate("xyz"):
        add("axis_" + n, "axis line", [[t * (a == i) for a in range(3)] for t in (-2., -1., 0., 1., 2.)], poses=("identity", BASE))
    for n, d in (("diag_110", (1., 1., 0.)), ("diag_111", (1., 1., 1.)), ("diag_1m12", (1., -1., 2.))):
        add(n, "diagonal line", [[t * d[a] for a in range(3)] for t in (-1., -0.5, 0., 0.5, 1.)])
    for n, noise in (("0", 0.), ("1e-5", 1e-5), ("1e-3", 1e-3), ("1e-1", 1e-1), ("0.3", 0.3)):
        add("line_noise_" + n, "noisy line", _line(9, 0.5, noise, 20 + len(n)))
    for n, a in (("0.5", 0.5), ("1e-1", 1e-1), ("1e-2", 1e-2), ("1e-3", 1e-3), ("1e-5", 1e-5)):
        add("disc_flat_" + n, "disc", _disc(1. + a, 0.))
        add("disc_thick_" + n, "disc", _disc(1. + a, 0.125), poses=(BASE,) + (OTHER_POSES if n == "0.5" else ()))
    # covariance diag(4, 1, 1) exactly: l2 = l3, the discriminant is exactly 0, and |m11| = |m22| (the d1 >= d2 tie)
    add("l2_equals_l3", "l2 = l3", [[4., 0., 0.], [-4., 0., 0.], [0., 2., 0.], [0., -2., 0.], [0., 0., 2.], [0., 0., -2.], [0., 0., 0.], [0., 0., 0.]],
        poses=("identity", BASE))
    for group in ("off100", "off5000"):
        add("line_noise_1e-3_" + group, "offset", _line(9, 0.5, 1e-3, 31), group=group)
        add("disc_thick_0.5_" + group, "offset", _disc(1.5, 0.125), group=group)
        add("disc_flat_1e-1_" + group, "offset", _disc(1.1, 0.), group=group)
    return C


EDGE_ORIGIN = {"near": (0., 0., 0.), "off100": (100., -100., 100.), "off5000": (5000., -5000., 5000.)}
SPACING = 25.0


def _patch(k, frame, normal, distance, shift, noise, seed, extent=1.0):
    """k points of the plane (frame[normal] . x = distance) around distance n + shift, spread over `extent`, off the plane
    by noise x extent"""
    rng = Lcg(seed)
    e = [frame[(normal + 1) % 3], frame[(normal + 2) % 3], frame[normal]]
    out = []
    for j in range(k):
        a, b, c = rng.unit(), rng.unit(), rng.unit()
        if j < 3:                                   # three corners first, so that no patch is nearly a line
            a, b = ((1., 0.), (-0.5, 0.875), (-0.5, -0.875))[j]
        out.append(_combine(e, (shift[0] + extent * a, shift[1] + extent * b, distance + noise * extent * c)))
    return out


def surface_clusters():
    """[(name, family, group, points (map frame), target of the query (map frame), poses, zero row expected)]"""
    S = []

    def add(name, family, pts, off=(0.1, -0.2, 0.3), group="near", poses=(BASE,), zero=False, first=None):
        # the query: beside the first point (so that it is the first neighbour) where asked, else beside the centre
        at = pts[first] if first is not None else [sum(p[i] for p in pts) / len(pts) for i in range(3)]
        S.append((name, family, group, pts, [at[i] + off[i] for i in range(3)], poses, zero))
    for k, shift in ((3, (0., 0.)), (5, (30., 0.)), (15, (0., 30.)), (16, (30., 30.))):
        add("k%d" % k, "k", _patch(k, THIRDS, 0, 10., shift, 1e-4, 40 + k), poses=(BASE,) + (OTHER_POSES if k == 5 else ()))
    # plane z = 5 around (60, 1): the first neighbour has x = 0 / x < 0 exactly; a first column that is zero below its pivot
    add("first_x_zero", "pivot", [[0., 61., 5.], [1., 60., 5.], [-1., 60.5, 5.], [0.5, 62., 5.], [-0.75, 61.5, 5.]], (0.01, 0.02, 0.3), first=0)
    add("first_x_negative", "pivot", [[-0.5, 91., 5.], [1., 90., 5.], [-1., 90.5, 5.], [0.5, 92., 5.], [0.75, 91.5, 5.]], (0.01, 0.02, 0.3), first=0)
    add("column_zero_below", "pivot", [[1., 120., 5.], [0., 121., 5.], [0., 119., 5.], [0., 122., 5.], [0., 120.5, 5.]], (0.01, 0.02, 0.3), first=0)
    # every x = 0: the first column is zero (vv == 0, no reflection) and the plane x = 0 holds the origin: no solution
    add("column_all_zero", "no plane", [[0., 150., 1.], [0., 151., 2.], [0., 149., 1.5], [0., 150.5, 3.], [0., 152., 1.]], (0.3, 0.02, 0.1), zero=True)
    planes = (("d0.1_thirds", 0.1, THIRDS, 0, 0.), ("d1_tilt", 1., TILT, 2, 1e-4), ("d10_axes", 10., AXES, 2, 1e-2),
              ("d0.1_tilt", 0.1, TILT, 0, 1e-2), ("d1_thirds", 1., THIRDS, 1, 0.), ("d10_tilt", 10., TILT, 1, 1e-4))
    for j, (n, d, frame, normal, noise) in enumerate(planes):
        add("plane_" + n, "plane", _patch(6, frame, normal, d, (-40. - 30. * j, 25. * (j % 2)), noise, 60 + j), poses=(BASE,) + (OTHER_POSES if n == "d1_tilt" else ()))
    t = [-2., -1., 0., 1., 2.]
    add("coincident", "no plane", [[-30., 2., 1.]] * 5, zero=True)
    add("exact_line", "no plane", [[-60. + v, 2., 0.] for v in t], zero=True)
    add("line_thick_1e-11", "no plane", [[-90. + v, 2., 4e-11 * s] for v, s in zip(t, (1., -1., 1., -1., 0.))], zero=True)
    add("line_thick_1e-6", "thin plane", [[-120. + v, 2., 4e-6 * s] for v, s in zip(t, (1., -1., 1., -1., 0.))])
    for j, noise in enumerate((0., 1e-4, 1e-2)):
        add("plane_d1000_%d" % j, "far plane", _patch(6, TILT, 2, 1000., (30. * j, 0.), noise, 80 + j, extent=2.0), group="far")
    return S


# ---- ties: k + 1 map points, the k-th and (k + 1)-th mirrored in y and so equidistant from a query on y = 0, exactly
TIE_K = 5
TIE_POINTS = [[0.25, 0., 2.], [-0.25, 0.125, 2.5], [0.5, -0.125, 1.5], [1., 0.25, 2.25], [1.5, 2., 3.], [1.5, -2., 3.]]
TIE_QUERY = [0.375, 0., 2.125]
TIE_SURFACE_POINTS = [[0.25, 0., 2.], [-0.25, 0.125, 2.25], [0.5, -0.125, 2.5], [1., 0.25, 1.75], [1.5, 2., 2.25], [1.5, -2., 2.25]]


# ---------------------------------------------------------------------------------------------- exact arithmetic
def fr(v):
    return [Fr(float(x)) for x in v]


def query_of(pose, p0):
    """q = R p0 + t exactly, and the sums of the absolute values of its four terms"""
    P, p = fr(pose), fr(p0)
    q = [P[4 * r] * p[0] + P[4 * r + 1] * p[1] + P[4 * r + 2] * p[2] + P[4 * r + 3] for r in range(3)]
    a = [abs(P[4 * r] * p[0]) + abs(P[4 * r + 1] * p[1]) + abs(P[4 * r + 2] * p[2]) + abs(P[4 * r + 3]) for r in range(3)]
    return q, a


def nearest_exact(points, q, k):
    """indices of the k nearest of `points` ([n][3] floats) to the exact q: ascending distance, equal ones by the index;
    and the squared distances of the k-th and of the next one"""
    d = sorted((sum((Fr(float(p[i])) - q[i]) ** 2 for i in range(3)), j) for j, p in enumerate(points))
    return [j for _, j in d[:k]], d[k - 1][0], (d[k][0] if len(d) > k else None)


def drp_dq_exact(quat, p0):
    """rotationlib::DRpDq, 3 x 4, from the quaternion's doubles and the float32 point: the values and the term sums"""
    w, v, p = Fr(float(quat[0])), fr(quat[1:]), fr(p0)
    cr = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]  # noqa: E731
    cra = lambda a, b: [abs(a[1] * b[2]) + abs(a[2] * b[1]), abs(a[2] * b[0]) + abs(a[0] * b[2]), abs(a[0] * b[1]) + abs(a[1] * b[0])]  # noqa: E731
    vxp, vxpa = cr(v, p), cra(v, p)
    vp, vpa = sum(v[i] * p[i] for i in range(3)), sum(abs(v[i] * p[i]) for i in range(3))
    K = [[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]]
    d, a = [[0] * 4 for _ in range(3)], [[0] * 4 for _ in range(3)]
    for r in range(3):
        d[r][0], a[r][0] = 2 * (w * p[r] + vxp[r]), 2 * (abs(w * p[r]) + vxpa[r])
        for c in range(3):
            d[r][1 + c] = 2 * ((vp if r == c else 0) + v[r] * p[c] - p[r] * v[c] - w * K[r][c])
            a[r][1 + c] = 2 * ((vpa if r == c else 0) + abs(v[r] * p[c]) + abs(p[r] * v[c]) + abs(w * K[r][c]))
    return d, a


def mean_exact(nb):
    k = len(nb)
    return [sum(Fr(float(p[i])) for p in nb) / k for i in range(3)], [sum(abs(Fr(float(p[i]))) for p in nb) / k for i in range(3)]


def edge_row_exact(nb, p0, pose, quat, u):
    """The edge row with `u` for the eigenvector, exactly: residual (q - p1) x (q - p2), p1 / p2 = mean -/+ u, and the 3 x 7
    Jacobian [Hat(2 u) DRpDq | Hat(2 u)], each with its scale -- the first-order running error of the entry per 2^-53:
    the sum of the absolute values of the terms of q, the mean and DRpDq, carried through the products."""
    uu = fr(u)
    q, qa = query_of(pose, p0)
    m, ma = mean_exact(nb)
    a = [q[i] - m[i] + uu[i] for i in range(3)]
    b = [q[i] - m[i] - uu[i] for i in range(3)]
    s = [qa[i] + ma[i] + abs(uu[i]) for i in range(3)]
    res, rs = [], []
    for i in range(3):
        j, l = (i + 1) % 3, (i + 2) % 3
        res.append(a[j] * b[l] - a[l] * b[j])
        rs.append(s[j] * abs(b[l]) + abs(a[j]) * s[l] + s[l] * abs(b[j]) + abs(a[l]) * s[j] + abs(a[j] * b[l]) + abs(a[l] * b[j]))
    d, da = drp_dq_exact(quat, p0)
    e = [2 * x for x in uu]
    K = [[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]]
    J, Js = [], []
    for r in range(3):
        for c in range(4):
            J.append(sum(K[r][t] * d[t][c] for t in range(3)))
            Js.append(sum(abs(K[r][t]) * da[t][c] for t in range(3)))
        for c in range(3):
            J.append(K[r][c])
            Js.append(Fr(0))
    f = lambda v: np.array([float(x) for x in v])  # noqa: E731
    return f(res), f(rs), f(J), f(Js)


def surface_row_exact(p0, pose, quat, u, inv_norm_w):
    """The entries of a surface row that follow from its unit normal u (the fixture's, rounded to doubles): J[0:4] = u^T
    DRpDq, and every entry's scale -- u is known to (condition factor) 2^-53 in each component, and that error is carried by
    |DRpDq| into J[0:4] and by |q| and 1 / |w| into the residual u . q + 1 / |w|."""
    uu = fr(u)
    q, qa = query_of(pose, p0)
    d, da = drp_dq_exact(quat, p0)
    J = [sum(uu[t] * d[t][c] for t in range(3)) for c in range(4)]
    Js = [sum(da[t][c] for t in range(3)) for c in range(4)]
    rs = sum(qa) + Fr(float(inv_norm_w))
    return np.array([float(x) for x in J]), np.array([float(x) for x in Js] + [1.0, 1.0, 1.0]), float(rs)


# ---------------------------------------------------------------------------------------------- the fixture
def f32_hex(points):
    return "".join("%08x" % int(v) for v in np.asarray(points, np.float32).reshape(-1).view(np.uint32))


def f32_unhex(text, cols=3):
    return np.array([int(text[i:i + 8], 16) for i in range(0, len(text), 8)], np.uint32).view(np.float32).reshape(-1, cols)


def unhex(values):
    return np.array([float.fromhex(v) for v in values])


_LOADED = {}


def load():
    """the fixture as dicts of arrays:
    poses[name] = (pose [12], quaternion [4]); maps[(kind, group)] = points [n][4] float32 (w = 1);
    rows = [dict(kind, name, family, group, pose, k, first (of the cluster in its map), p0 [3] float32, and what is expected)];
    ties = [dict(kind, reversed, map [6][4], k, p0, neighbours (original indices, in order), expected)]"""
    if _LOADED:
        return _LOADED
    with open(PATH) as f:
        doc = json.load(f)
    poses = {n: (unhex(v[:12]), unhex(v[12:])) for n, v in doc["poses"].items()}
    maps, rows = {}, []

    def expected(kind, e, row):
        if kind == EDGE:
            row.update(u=unhex(e[:3]), kappa=float(e[3]), fallback=bool(e[4]))
        else:
            row.update(zero=bool(e[0]))
            if not row["zero"]:
                row.update(u=unhex(e[1:4]), residual=float.fromhex(e[4]), inv_norm_w=float(e[5]), condition=float(e[6]))
    for kind, key in ((EDGE, "edge"), (SURFACE, "surface")):
        for group, text in doc[key + "_maps"].items():
            xyz = f32_unhex(text)
            maps[(kind, group)] = np.ascontiguousarray(np.hstack([xyz, np.ones((len(xyz), 1), np.float32)]))
        for name, family, group, pose, k, first, p0, e in doc[key + "_rows"]:
            row = dict(kind=kind, name=name, family=family, group=group, pose=pose, k=k, first=first, p0=f32_unhex(p0)[0])
            expected(kind, e, row)
            rows.append(row)
    ties = []
    for kind, rev, text, k, p0, nbrs, e in doc["ties"]:
        xyz = f32_unhex(text)
        row = dict(kind=kind, reversed=bool(rev), map=np.ascontiguousarray(np.hstack([xyz, np.ones((len(xyz), 1), np.float32)])), k=k,
                   p0=f32_unhex(p0)[0], neighbours=nbrs, pose="identity", name="tie_%s%s" % ("edge" if kind == EDGE else "surface", "_reversed" if rev else ""),
                   family="tie")
        expected(kind, e, row)
        ties.append(row)
    _LOADED.update(poses=poses, maps=maps, rows=rows, ties=ties)
    return _LOADED


def neighbours_of(row, data=None):
    """the float32 neighbours of a row, [k][3], in the order of the map"""
    data = data or load()
    if "map" in row:
        return row["map"][row["neighbours"], :3]
    return data["maps"][(row["kind"], row["group"])][row["first"]:row["first"] + row["k"], :3]


# ---------------------------------------------------------------------------------------------- measuring a row
def hat_to_u(J):
    """u of J[:, 4:7] = Hat(2 u) (J [3][7]), and whether the block is antisymmetric with a zero diagonal, exactly"""
    K = J[:, 4:7]
    exact = K[0, 0] == 0 and K[1, 1] == 0 and K[2, 2] == 0 and K[0, 1] == -K[1, 0] and K[0, 2] == -K[2, 0] and K[1, 2] == -K[2, 1]
    return np.array([K[2, 1], K[0, 2], K[1, 0]]) / 2.0, bool(exact)


def norm_units(u):
    """| |u| - 1 | in units of 2^-53: (|u|^2 - 1) / 2 from the exact sum of squares (second order in the difference apart)"""
    return abs(float((sum(Fr(float(x)) ** 2 for x in u) - 1) / 2)) / EPS


def edge_row_units(row, res, J, data=None):
    """An edge row (res [3], J [21]) measured: its own u, | |u| - 1 | / 2^-53, |sin(u, u_ref)| over the direction bound, and
    the worst |entry - exact entry with that u| / (2^-53 x the entry's scale)"""
    data = data or load()
    pose, quat = data["poses"][row["pose"]]
    u, exact = hat_to_u(np.asarray(J).reshape(3, 7))
    wres, rs, wJ, Js = edge_row_exact(neighbours_of(row, data), row["p0"], pose, quat, u)
    worst = 0.0
    for got, want, scale in ((np.asarray(res), wres, rs), (np.asarray(J).reshape(21), wJ, Js)):
        diff = np.abs(got - want)
        if np.any(diff[scale == 0] != 0):
            return dict(u=u, hat_exact=exact, norm=np.inf, direction=np.inf, rest=np.inf)
        worst = max(worst, float((diff[scale > 0] / (EPS * scale[scale > 0])).max()))
    sin = float(np.linalg.norm(np.cross(u, row["u"]))) / float(np.linalg.norm(u))
    if row["fallback"]:                                                        # the isotropic row: (0, 0, 1) itself, or nothing
        direction = 0.0 if np.array_equal(u, [0.0, 0.0, 1.0]) else np.inf
    else:
        direction = sin / direction_bound(row["kappa"])
    return dict(u=u, hat_exact=exact, norm=norm_units(u), direction=direction, rest=worst, sin=sin)


def surface_row_units(row, res, J, data=None):
    """A surface row (res, J [7]) measured against the fixture: zero rows by bits; else | |u| - 1 | / 2^-53 and the worst
    |entry - expected| / (2^-53 x condition x scale), the factor C_BOUND left out"""
    data = data or load()
    J = np.asarray(J).reshape(7)
    if row["zero"]:
        return dict(zero_ok=bool(res == 0.0 and not J.any()))
    pose, quat = data["poses"][row["pose"]]
    wJ, Js, rs = surface_row_exact(row["p0"], pose, quat, row["u"], row["inv_norm_w"])
    want = np.concatenate([wJ, row["u"]])
    worst = max(float((np.abs(J - want) / (EPS * row["condition"] * Js)).max()), abs(float(res) - row["residual"]) / (EPS * row["condition"] * rs))
    return dict(zero_ok=None, norm=norm_units(J[4:7]), worst=worst)
