"""The scans lfx_align_report is checked at (tests/test_align_report_expect.py on the host, tests/test_align_report_edges_gpu.py
on the device), the smallest shapes that reach each edge, and the tolerance's constants beside them.

SELECTION cases (align_report_scale_kernel's copy of ComputeErrors / Scale / ComputeWeights): align_step_cases' family B --
n3 = 40 .. 43 with n1 = 100 .. 103, the tiny ones (n3, n1 = 0 .. 3), n3 + n1 = 6 144 and 6 145 (the keys in LDS / passing
through the weights' place) and the scan with a majority of zero rows.

HAND scenes, laid as test_align_report_gpu._corridor is: exact lattices in float32, the map at 0.2 m, the scan at 0.25 m
shifted, 0.75 m kept clear of the corners, so that the 15 nearest map points of every scan point lie in ONE plane.  Every
scene is mirror-symmetric about the sensor where it can be, and its scan stands off the walls by the SAME inset on both sides:
the gradient at the start pose is zero up to rounding, so the pose the alignment returns is the start pose (or, where D is
degenerate, the update is refused and it is the start pose to the bit) and what the host claims of a scene holds where the
device reports.  No population of equal errors is a majority of a scan's rows: the robust scale is then one population's
error and not the rounding noise within one (exact coordinates have no noise to set a scale from).

THE TOLERANCES.  A sum of the record (information, error, sigma2, the rms values) is held to C_SUM * MARGIN * 2^-53 * its
largest term (`units` below: for H, sum_i w_i |J_i|^2 |M|^2); C_SUM is the worst ratio over the cases, measured on the host
alone, of report_restatement.restate (float64, numpy's order) to the 50-digit reference; MARGIN = 4 is for the device's other
order of summation (matrix-unit tiles, waves then slices), as pose_graph_marginal_cases.MARGIN.  The eigen-solves'
restatement (align_report_reference.algorithm) is held to the 50-digit reference by C_EIG * 2^-53 |H|_2 (eigenvalues; vectors
and spans divided by their gap) and C_COV * 2^-53 cond max |C| (the floored cond), measured the same way; the device is held
to the restatement bit for bit.  `python -m tests.align_report_cases` prints the three."""
import functools

import numpy as np

from tests import align_report_reference as RR
from tests import align_step_cases as AC
from tests.report_restatement import restate

U = 2.0 ** -53
MARGIN = 4.0
CAP = 1e10
K = AC.K_NEIGHBOURS
HUBER_MARGIN = 1e-6                                      # restate's rule: a normalised error this close to 1.345^2 (relative) decides nothing
# Measured by measure() on the host (python -m tests.align_report_cases), rounded up to two digits
C_SUM, C_EIG, C_COV = 11.0, 18.0, 0.30
EPSILON = {"converging_above_floor": 4.253e-4, "converging_below_floor": 4.253e-5}      # wall tilts, from solve_epsilon()
WINDOW = {"converging_above_floor": (3e-9, 3e-8), "converging_below_floor": (3e-11, 3e-10)}
LONG_COND = 3.584e4                                        # cond_2(H) of long_corridor, recorded (capped at CAP)

X, Y, Z = np.eye(3)
IDENTITY = AC.IDENTITY


def lattice(half, step, offset=0.0):
    """+-(offset + step k) up to `half`: a lattice that is its own mirror image"""
    pos = offset + step * np.arange(0, int((half - offset) / step + 1e-9) + 1)
    return np.unique(np.concatenate([-pos, pos]))


def _quantile_insets(key, insets):
    """insets = ((fraction, inset), ...) handed out by ascending `key`: the first fraction of the points (those with the
    smallest keys) stand off by the first inset, and so on.  A point's place is the number of points with a smaller key, so
    points with equal keys share one inset.  surface() and line() make the key a function of |u| and |v| alone: a point and
    its mirror images have equal keys and therefore equal insets, which keeps a symmetric scene symmetric.  surface()'s key
    max(|u|, |v|) + 0.37 min(|u|, |v|) (both scaled to 1) orders the points by square rings about the centre; the second term
    tells the points of one ring apart -- with max alone a whole ring would share one key and fall into one population
    whatever the fractions ask for -- and is the same under u <-> v, which the wall at 45 degrees needs of its floor."""
    if len(insets) == 1:
        return np.full(len(key), insets[0][1])
    rank = np.searchsorted(np.sort(key), key, side="left") / float(len(key))
    out, lo = np.zeros(len(key)), 0.0
    for fraction, inset in insets:
        out[(rank >= lo - 1e-12) & (rank < lo + fraction)] = inset
        lo += fraction
    out[rank >= lo] = insets[-1][1]
    return out


def surface(origin, a, b, inward, map_u, map_v, scan_u, scan_v, insets=((1.0, 0.0),)):
    """One plane origin + u a + v b: (map points, scan points), [n][4] float32; the scan stands `inset` off it along `inward`"""
    def lay(u, v):
        g = np.stack(np.meshgrid(u, v, indexing="ij"), -1).reshape(-1, 2)
        return g, np.asarray(origin, np.float64) + g[:, :1] * a + g[:, 1:] * b
    _, m = lay(map_u, map_v)
    g, s = lay(scan_u, scan_v)
    mid = 0.5 * (np.min(scan_v) + np.max(scan_v))
    ku, kv = np.abs(g[:, 0]) / np.abs(scan_u).max(), np.abs(g[:, 1] - mid) / max(np.abs(scan_v - mid).max(), 1e-9)
    key = np.maximum(ku, kv) + 0.37 * np.minimum(ku, kv)         # (few ties beyond the mirror images; the same under u <-> v)
    s = s + _quantile_insets(key, insets)[:, None] * np.asarray(inward, np.float64)
    return _pad(m), _pad(s)


def _pad(p):
    out = np.zeros((len(p), 4), np.float32)
    out[:, :3] = p
    return out


def line(origin, inward, half, insets=((1.0, 0.1),), step=0.125):
    """One edge line along x through `origin`: map points every 0.2 m, scan points every `step`, off it along `inward`"""
    xm, xs = lattice(half, 0.2), lattice(half - 0.5, step, 0.5 * step)
    m = np.asarray(origin, np.float64) + xm[:, None] * X
    s = np.asarray(origin, np.float64) + xs[:, None] * X
    s = s + _quantile_insets(np.abs(xs), insets)[:, None] * np.asarray(inward, np.float64)
    return _pad(m), _pad(s)


WALL_Z_MAP, WALL_Z_SCAN = np.arange(-1.8, 1.201, 0.2), np.arange(-1.03, 0.7, 0.25)
THREE = ((0.4, 0.0), (0.4, 0.1), (0.2, 0.2))


def _floor(half, insets=((1.0, 0.0),), step=0.25, width=3.0, scan_width=1.5):
    return surface((0, 0, -1.8), X, Y, Z, lattice(half, 0.2), lattice(width, 0.2), lattice(half - 0.75, step, 0.5 * step),
                   lattice(scan_width, 0.25, 0.125), insets)


def _wall(side, half, insets=((1.0, 0.1),), tilt=0.0, step=0.25):
    """The wall y = side * 3, its far end turned towards the corridor's axis by `tilt` (rad): y = side * (3 - tilt x)"""
    a = np.array([1.0, -side * tilt, 0.0]) / np.hypot(1.0, tilt)
    inward = np.array([-tilt, -side, 0.0]) / np.hypot(1.0, tilt)
    return surface((0, 3.0 * side, 0), a, Z, inward, lattice(half, 0.2), WALL_Z_MAP, lattice(half - 0.75, step, 0.5 * step),
                   WALL_Z_SCAN, insets)


def _end_wall(half):
    return surface((half, 0, 0), Y, Z, -X, lattice(3.0, 0.2), WALL_Z_MAP, lattice(2.25, 0.25, 0.125), WALL_Z_SCAN)


def _corridor(half, end_wall, tilt=0.0, step=0.25, line_step=0.125):
    s = [_floor(half, step=step), _wall(1.0, half, tilt=tilt, step=step), _wall(-1.0, half, tilt=tilt, step=step)]
    if end_wall:
        s.append(_end_wall(half))
    e = [line((0, 3.0, -1.8), -Y, half, step=line_step), line((0, -3.0, -1.8), Y, half, step=line_step)]
    return s, e


def _box(a, b, c, inset_x, inset_y):
    """A closed box centred on the sensor, |x| <= a, |y| <= b, |z| <= c; the faces z = +-c carry no inset"""
    def face(axis, sign, half_u, half_v, insets):
        normal = np.eye(3)[axis] * sign
        u_axis, v_axis = [np.eye(3)[k] for k in range(3) if k != axis]
        return surface(normal * (a, b, c)[axis], u_axis, v_axis, -normal, lattice(half_u, 0.2), lattice(half_v, 0.2),
                       lattice(half_u - 0.75, 0.25, 0.125), lattice(half_v - 0.75, 0.25, 0.125), insets)
    s = []
    for sign in (1.0, -1.0):
        s += [face(0, sign, b, c, inset_x), face(1, sign, a, c, inset_y), face(2, sign, a, b, ((1.0, 0.0),))]
    return s


ROTATED_POSE = np.ascontiguousarray(np.hstack([AC._rotation(2.5 * np.array([0.36, -0.48, 0.8])), np.array([[0.5], [-0.25], [0.125]])]))
HAND = {                                                 # name -> expected rank
    "floor": 3, "floor_wall": 5, "corridor": 5, "corridor_end": 6, "two_lines": 5, "one_line": 4, "corridor_end_rotated": 6,
    "box": 6, "box_square": 6, "wall_at_45": 5, "converging_above_floor": 6, "converging_below_floor": 5, "long_corridor": 6}
HALF = 6.0


def _surfaces_and_lines(name, epsilon=None):
    none_s, none_e = [_floor(HALF)[0]], [line((0, 3.0, -1.8), -Y, HALF)[0]]          # (a map for the kind without rows)
    if name == "floor":
        return [_floor(HALF, THREE)], [(none_e[0], np.zeros((0, 4), np.float32))]
    if name == "floor_wall":
        return [_floor(HALF, ((0.5, 0.0), (0.5, 0.1))), _wall(1.0, HALF, ((1.0, 0.2),))], [(none_e[0], np.zeros((0, 4), np.float32))]
    if name == "corridor":
        return _corridor(HALF, False)
    if name in ("corridor_end", "corridor_end_rotated"):
        return _corridor(HALF, True)
    if name == "two_lines":
        return [(none_s[0], np.zeros((0, 4), np.float32))], [line((0, 3.0, -1.8), -Y, HALF, THREE), line((0, -3.0, -1.8), Y, HALF, THREE)]
    if name == "one_line":
        return [(none_s[0], np.zeros((0, 4), np.float32))], [line((0, 3.0, -1.8), -Y, HALF, ((1.0, 0.0),))]
    if name == "box":                                    # y and z faces: equal counts, both inliers; the x faces are down-weighted
        return _box(3.0, 2.2, 2.2, ((1.0, 0.2),), ((1.0, 0.1),)), [(none_e[0], np.zeros((0, 4), np.float32))]
    if name == "box_square":
        half = ((0.5, 0.1), (0.5, 0.2))
        return _box(3.0, 3.0, 2.0, half, half), [(none_e[0], np.zeros((0, 4), np.float32))]
    if name == "wall_at_45":
        n = (X + Y) / np.sqrt(2.0)
        wall = surface(3.0 * n, (X - Y) / np.sqrt(2.0), Z, -n, lattice(3.0, 0.2), WALL_Z_MAP, lattice(2.25, 0.25, 0.125), WALL_Z_SCAN, ((1.0, 0.2),))
        floor = surface((0, 0, -1.8), X, Y, Z, lattice(6.0, 0.2), lattice(6.0, 0.2), lattice(1.5, 0.25, 0.125), lattice(1.5, 0.25, 0.125),
                        ((0.5, 0.0), (0.5, 0.1)))
        return [floor, wall], [(none_e[0], np.zeros((0, 4), np.float32))]
    if name in EPSILON:
        return _corridor(HALF, False, tilt=EPSILON[name] if epsilon is None else epsilon)
    if name == "long_corridor":
        return _corridor(100.0, True, step=4.0, line_step=2.0)
    raise ValueError(name)


def hand_case(name, epsilon=None):
    s, e = _surfaces_and_lines(name, epsilon)
    pose = ROTATED_POSE if name.endswith("_rotated") else IDENTITY
    out = dict(name=name, edge_map=np.concatenate([p[0] for p in e]), surface_map=np.concatenate([p[0] for p in s]),
               edge=np.concatenate([p[1] for p in e]), surface=np.concatenate([p[1] for p in s]), pose=pose, rank=HAND[name])
    if pose is not IDENTITY:                             # the scan in the sensor's frame: R^T (p - t), rounded to float32
        for k in ("edge", "surface"):
            p = out[k][:, :3].astype(np.float64)
            out[k] = _pad((p - pose[:, 3]) @ pose[:, :3])
    out["n3"], out["n1"] = len(out["edge"]), len(out["surface"])
    return out


@functools.lru_cache(maxsize=None)
def hand_cases():
    return [hand_case(n) for n in HAND]


@functools.lru_cache(maxsize=None)
def selection_scene():
    return AC.mixed_scene()


@functools.lru_cache(maxsize=None)
def selection_cases():
    """align_step_cases' family B with the maps each case goes against; (0, 0), the empty scan, included"""
    scene = selection_scene()
    out = [dict(c, edge_map=scene["edge_map"], surface_map=scene["surface_map"]) for c in AC.mixed_cases(scene)]
    out.append(dict(AC.zero_row_case(scene), edge_map=scene["edge_map"], surface_map=scene["coincident_map"]))
    return out


def is_tiny(c):
    return (c["n3"], c["n1"]) in AC.TINY_COUNTS


def oracle_rows(c, pose=None):
    """(r3, J3, r1, J1) of a case at its start pose from the CPU oracle"""
    pose = c["pose"] if pose is None else pose
    r3, J3 = AC.oracle_rows(c["edge_map"], 0, pose, c["edge"], K)
    r1, J1 = AC.oracle_rows(c["surface_map"], 1, pose, c["surface"], K)
    return r3, J3, r1.reshape(-1), J1


# ---- the bounds -------------------------------------------------------------------------------------------------------------

SUM_FIELDS = ("information", "error", "sigma2", "rms_edge", "rms_surface")


def units(ref):
    """2^-53 * the largest term of each sum of the record, from the 50-digit reference.  sigma2 is a quotient whose
    denominator sum w dim - 6 cancels: its relative error is the numerator's plus the denominator's sum over what is left."""
    s2 = abs(ref["sigma2"]) * (1.0 + ref["sum_w_dim"] / abs(ref["dim"])) if ref["dim"] > 0 else np.nan
    return dict(information=U * ref["sum_w_j2"] * ref["norm_m2"], error=U * ref["error"], sigma2=U * s2,
                rms_edge=U * ref["rms_edge"], rms_surface=U * ref["rms_surface"])


def sum_ratios(got, ref):
    """|got - reference| of every sum in its unit (0 where the reference's term is 0 and so is got's; NaN sigma2 left out)"""
    un, out = units(ref), {}
    for k in SUM_FIELDS:
        if k == "sigma2" and not ref["dim"] > 0:
            continue
        d = float(np.abs(np.asarray(got[k], np.float64) - ref[k]).max())
        out[k] = 0.0 if d == 0.0 else d / un[k]
    return out


def eigen_ratios(got, ref):
    """algorithm()'s (or the device's) eigenvalues, vectors / spans and covariance against the reference, in units of 2^-53
    |H|_2 (vectors and spans: over their gap to the rest) and of 2^-53 cond max |C|"""
    lam, top = ref["eigenvalues"], ref["norm_h"]
    out = dict(eigenvalues=float(np.abs(got["eigenvalues"] - lam).max()) / (U * top), vectors=0.0)
    for first, last in RR.clusters(lam):
        near = [lam[first] - lam[first - 1]] if first else []
        near += [lam[last] - lam[last - 1]] if last < 6 else []
        gap = min(near) / top if near else 1.0
        if last - first == 1:
            v, r = got["eigenvectors"][first], ref["eigenvectors"][first]
            d = min(np.abs(v - r).max(), np.abs(v + r).max())      # (the sign rule is checked on its own: a tie may turn it)
        else:
            P = lambda rows: rows[first:last].T @ rows[first:last]   # noqa: E731
            d = np.abs(P(got["eigenvectors"]) - P(ref["eigenvectors"])).max()
        out["vectors"] = max(out["vectors"], float(d) * gap / U)
    if ref["dim"] > 0:
        top_c = float(np.abs(ref["covariance"]).max())
        d = float(np.abs(got["covariance"] - ref["covariance"]).max())
        out["covariance"] = 0.0 if d == 0.0 else d / (U * ref["cond"] * top_c)
    return out


def d_bound(ref):
    """min_eigenvalue_d against the reference's, and the margin IsDegenerate's 0.1 is kept clear by: C_EIG 2^-53 |D|_2"""
    return C_EIG * U * ref["norm_d"]


@functools.lru_cache(maxsize=None)
def host_reference(name):
    c = [c for c in selection_cases() + hand_cases() if c["name"] == name][0]
    rows = oracle_rows(c)
    return rows, RR.reference(c["pose"], *rows)


def all_names():
    return [c["name"] for c in selection_cases() + hand_cases() if c["n3"] + c["n1"] > 0]


@functools.lru_cache(maxsize=None)
def measure():
    """{name: (sum ratios of restate, eigen ratios of algorithm, D's ratio, near the Huber threshold)} on the oracle's rows.
    The sums are held in a near case too (the Huber weight is continuous at the threshold); only the counts are not."""
    out = {}
    for c in selection_cases() + hand_cases():
        if c["n3"] + c["n1"] == 0:
            continue
        rows, ref = host_reference(c["name"])
        near = ref["huber_margin"] <= HUBER_MARGIN
        sums = sum_ratios(restate(c["pose"], *rows), ref)
        alg = RR.algorithm(ref["information"], ref["sigma2"])
        eig = eigen_ratios(alg, ref)
        dmin, _ = RR.algorithm_d(ref["D"])
        out[c["name"]] = (sums, eig, abs(dmin - ref["min_eigenvalue_d"]) / (U * ref["norm_d"]), near)
    return out


def solve_epsilon(name):
    """The wall tilt that puts lambda_0 / lambda_5 at the (geometric) middle of the case's window: the ratio grows as the
    tilt's square, so one evaluation at 1e-3 rad gives it"""
    c = hand_case(name, epsilon=1e-3)
    lam = restate(c["pose"], *oracle_rows(c))["eigenvalues"]
    lo, hi = WINDOW[name]
    return 1e-3 * float(np.sqrt(np.sqrt(lo * hi) / (lam[0] / lam[5])))


if __name__ == "__main__":
    for n in EPSILON:
        print("EPSILON[%r] = %.3e (recorded %.3e)" % (n, solve_epsilon(n), EPSILON[n]))
    seen = measure()
    worst = lambda f: max([(f(v), k) for k, v in seen.items()])   # noqa: E731
    for name, (sums, eig, d, near) in seen.items():
        print("%-28s sums %s eigen %s D %.3g%s" % (name, {k: float("%.3g" % v) for k, v in sums.items()},
                                                  {k: float("%.3g" % v) for k, v in eig.items()}, d, "  (near the Huber threshold)" if near else ""))
    print("C_SUM = %.3g (%s)" % worst(lambda v: max(list(v[0].values()) + [0.0])))
    print("C_EIG = %.3g (%s)" % worst(lambda v: max(v[1]["eigenvalues"], v[1]["vectors"], v[2])))
    print("C_COV = %.3g (%s)" % worst(lambda v: v[1].get("covariance", 0.0)))
    print("LONG_COND = %.3e" % host_reference("long_corridor")[1]["cond"])
