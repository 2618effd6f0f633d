"""Deterministic builders of the one-iteration alignment cases (tests/test_align_step_expect.py, tests/test_align_step_gpu.py).
Seeded, no GPU, nothing read from outside the repository.

Family A: point-pair problems whose residuals at the initial pose are EXACTLY (a_i, 0, 0).  The pose is the identity or a
pure translation with dyadic entries, X has dyadic coordinates of 16 bits, a_i has at most 27 significant bits: y = x + t -
(a, 0, 0) is exact, the residual the library computes (m0 x + m1 y + m2 z + m3 - Y with m = the identity's rows) is a_i bit
for bit, and the error e_i = a_i^2 is exact whatever the order of operations.  For the kinds named in EXACT_SUM_KINDS every
partial sum of the e_i is exact too (they are multiples of one power of two u and their total stays below 2^53 u), so the
error of the scan is one number whatever the order of the additions.

Family B: clouds sliced from the features of synthetic scans against maps made of other scans' features, with counts that
put the boundary between 3-row and 1-row residuals, and the end of the rows, at every place inside a group of four."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np

COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 6143, 6144, 6145, 12289)
BIG_COUNT = 200001                                     # runs once: generic, shuffled
KINDS = ("generic", "low-byte", "last-byte", "all-equal", "two-valued-split", "two-valued-tied", "majority-zero",
         "majority-equal", "wide-exponent", "near-overflow")
ARRANGEMENTS = ("ascending", "descending", "runs-of-64", "runs-shifted", "shuffled")
EXACT_SUM_KINDS = ("generic", "all-equal", "two-valued-split", "two-valued-tied", "majority-zero", "majority-equal")
ZERO_SCALE_KINDS = ("all-equal", "two-valued-tied", "majority-zero", "majority-equal", "near-overflow")
IDENTITY = np.ascontiguousarray(np.hstack([np.eye(3), np.zeros((3, 1))]))


def translation(t):
    return np.ascontiguousarray(np.hstack([np.eye(3), np.asarray(t, np.float64).reshape(3, 1)]))


def makes_sense(kind, n):
    """near-overflow: three residuals of 2^511 among enough 0.5s to carry a step of their own."""
    return n >= 63 if kind == "near-overflow" else True


def _seed(kind, n, attempt=0):
    return [2024, KINDS.index(kind), int(n), int(attempt)]


def _generic(rng, n, total):
    """n distinct dyadics k 2^-20 with sum of k^2 over `total` of them < 2^53: the squares' sum is exact in any order."""
    kmax = min(2 ** 20 - 1, math.isqrt(2 ** 53 // max(total, 1)))
    return rng.choice(np.arange(1, kmax + 1), n, replace=False).astype(np.float64) * 2.0 ** -20


def values(kind, n, attempt=0):
    """The a_i of a case, before they are arranged."""
    rng = np.random.default_rng(_seed(kind, n, attempt))
    if kind == "generic":
        return _generic(rng, n, n)
    if kind == "low-byte":                               # e = 1 + k 2^-25 + k^2 2^-52: 53 bits, duplicates from n > 200
        return 1.0 + rng.integers(0, 200, n).astype(np.float64) * 2.0 ** -26
    if kind == "last-byte":
        return np.ones(n)
    if kind == "all-equal":
        return np.full(n, 0.375)
    if kind in ("two-valued-split", "two-valued-tied"):   # split: the two middle values of an even count differ
        low = n // 2 + (1 if kind == "two-valued-tied" else 0)
        return np.concatenate([np.full(low, 0.25), np.full(n - low, 0.5)])
    if kind == "majority-zero":
        return np.concatenate([np.zeros(n // 2 + 1), _generic(rng, n - (n // 2 + 1), n)])
    if kind == "majority-equal":
        return np.concatenate([np.full(n // 2 + 1, 0.375), _generic(rng, n - (n // 2 + 1), n)])
    if kind == "wide-exponent":
        # e = 2^-16j, j = 0 .. 62: one value per bin of the top byte (the biased exponent >> 4 = 63 .. 1); bin 0 holds the
        # subnormal e = 2^-1060 and the exact zeros
        pool = [2.0 ** (-8 * j) for j in range(63)] + [2.0 ** -530, 0.0, 0.0]
        return np.array([pool[i % len(pool)] for i in rng.permutation(n)], np.float64) if n > len(pool) else \
            np.array([pool[i] for i in rng.permutation(len(pool))[:n]], np.float64)
    if kind == "near-overflow":
        return np.concatenate([np.full(3, 2.0 ** 511), np.full(n - 3, 0.5)])
    raise ValueError(kind)


def second_values(kind, n, attempt=0):
    """The second residual component: 0 except for `last-byte`, whose residuals are (1, k 2^-26, 0): e = 1 + k^2 2^-52, all
    errors share their six leading bytes and differ in the last two."""
    if kind != "last-byte":
        return np.zeros(n)
    rng = np.random.default_rng(_seed(kind, n, attempt) + [2])
    return rng.integers(0, 200, n).astype(np.float64) * 2.0 ** -26


def arrange(keys, arrangement, seed):
    """A permutation of range(len(keys)): where the values sit decides which waves see one digit and what the tail wave holds."""
    n = len(keys)
    order = np.argsort(keys, kind="stable")
    if arrangement == "ascending":
        return order
    if arrangement == "descending":
        return order[::-1].copy()
    if arrangement in ("runs-of-64", "runs-shifted"):
        # the sorted values in runs of 64, full runs taken alternately from both ends (neighbouring runs then carry
        # different values), the partial run last; aligned to the waves, or shifted by one place
        full = [order[i:i + 64] for i in range(0, n - n % 64, 64)]
        picked = []
        while full:
            picked.append(full.pop(0))
            if full:
                picked.append(full.pop())
        perm = np.concatenate(picked + [order[n - n % 64:]]).astype(np.int64) if n else order
        return np.roll(perm, 1) if arrangement == "runs-shifted" else perm
    if arrangement == "shuffled":
        return np.random.default_rng(seed + [7]).permutation(n)
    raise ValueError(arrangement)


def exact_in_any_order(errors):
    """True if every partial sum of `errors` (non-negative doubles) is a double: all are multiples of one power of two u
    and the total is below 2^53 u."""
    fr = [Fraction(float(e)) for e in errors if e != 0.0]
    if not fr:
        return True
    den = max(f.denominator for f in fr)                 # (a power of two, as every double's)
    ks = [int(f * den) for f in fr]
    low = min(k & -k for k in ks)                         # the lowest set bit over all terms: they are multiples of it
    return sum(ks) // low < 2 ** 53


def near_huber_threshold(errors):
    """A normalised error within 1e-6 k^2 of the Huber threshold k^2 (the weight of that row is then a matter of rounding)."""
    if not len(errors):
        return False
    k2 = 1.345 * 1.345
    scale = 1.482602218505602 * np.median(np.abs(errors - np.median(errors)))
    with np.errstate(over="ignore"):
        return bool((np.abs(errors / (scale + 1e-16) - k2) <= 1e-6 * k2).any())


def pair_case(kind, n, arrangement="shuffled", degenerate_x=False):
    """One family-A problem: dict(X, Y, pose, a, a2, kind, n, arrangement, exact_sum, name).  Asserts that the residuals are
    (a_i, a2_i, 0) bit for bit."""
    seed = _seed(kind, n)
    rng = np.random.default_rng(seed + [1])
    for attempt in range(16):                           # (drawn again until no error sits at the Huber threshold)
        a, a2 = values(kind, n, attempt), second_values(kind, n, attempt)
        if not near_huber_threshold(a * a + a2 * a2):
            break
    else:
        raise AssertionError("no draw of %s, n = %d keeps clear of the Huber threshold" % (kind, n))
    wide = kind in ("wide-exponent", "near-overflow")
    # (the wide-exponent kinds: 0 in X's first coordinate and in t's, so that y = -a survives; the others alternate between
    # the identity and a dyadic translation)
    t = np.array([0.0, -1.25, 2.0]) if wide else (np.zeros(3) if n % 2 == 0 else np.array([0.5, -1.25, 2.0]))
    X = rng.integers(-32 * 1024, 32 * 1024 + 1, (n, 3)).astype(np.float64) / 1024.0
    if wide:
        X[:, 0] = 0.0
    if degenerate_x:
        X[:] = 0.0
    perm = arrange(a * a + a2 * a2, arrangement, seed)
    a, a2, X = a[perm], a2[perm], X[perm]                  # (whole pairs move: every arrangement holds the same set of rows)
    Y = X + t
    Y[:, 0] -= a
    Y[:, 1] -= a2
    pose = translation(t)
    r = np.stack([pose[i, 0] * X[:, 0] + pose[i, 1] * X[:, 1] + pose[i, 2] * X[:, 2] + pose[i, 3] - Y[:, i] for i in range(3)], 1)
    want = np.stack([a, a2, np.zeros(n)], 1)
    assert r.tobytes() == want.tobytes(), (kind, n, arrangement)
    e = a * a + a2 * a2
    assert all(Fraction(float(x)) == Fraction(float(p)) ** 2 + Fraction(float(s)) ** 2 for x, p, s in zip(e[:64], a[:64], a2[:64]))
    return dict(X=X, Y=Y, pose=pose, a=a, a2=a2, errors=e, kind=kind, n=n, arrangement=arrangement,
                exact_sum=exact_in_any_order(e), key=(kind, n, bool(degenerate_x)), name="%s, n = %d, %s%s" % (kind, n, arrangement, ", X = 0" if degenerate_x else ""))


_EXPECTED = {}


def expected(case):
    """The restatement's step for a family-A case.  The arrangements of one (kind, n) hold the same pairs in another order,
    and the restatement's sums are exact, so one evaluation serves them all.  What depends on the order of the rows does not
    go into the shared record: `weights` is dropped and `errors` is replaced by `errors_sorted`."""
    from tests.align_step_restatement import pair_rows, restate_step
    key = case.get("key")
    if key is None or key not in _EXPECTED:
        want = restate_step(case["pose"], *pair_rows(case["X"], case["Y"], case["pose"]))
        want["errors_sorted"] = np.sort(want.pop("errors"))
        want.pop("weights")
        if key is None:
            return want
        _EXPECTED[key] = want
    return _EXPECTED[key]


def pair_cases(kind, arrangement):
    """The problems of one (kind, arrangement): every count where the kind makes sense."""
    return [pair_case(kind, n, arrangement) for n in COUNTS if makes_sense(kind, n)]


def big_case():
    return pair_case("generic", BIG_COUNT, "shuffled")


def degenerate_cases():
    """No step: X = 0 (D has rank 3), and n = 1, 2 (rank 3 and 6 of 7)."""
    return [pair_case("generic", 64, "shuffled", degenerate_x=True), pair_case("two-valued-split", 1025, "shuffled", degenerate_x=True),
            pair_case("generic", 1), pair_case("generic", 2), pair_case("wide-exponent", 2)]


def _rotation(axis_angle):
    th = np.asarray(axis_angle, np.float64)
    k = np.linalg.norm(th)
    u = th / k
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + np.sin(k) * K + (1 - np.cos(k)) * K @ K


ROTATED_COUNTS = (5, 6, 7, 8, 1023, 1024, 1025, 6144, 6145)


def rotated_cases():
    """Problems at generic rotated poses, with noise and outliers (the errors are no longer exact): n mod 4, the 3 072-row
    sweep of the update kernel and both sides of 6 144 for the sums."""
    out = []
    for n in ROTATED_COUNTS:
        rng = np.random.default_rng([2025, n])
        X = rng.uniform(-20, 20, (n, 3))
        true = np.hstack([_rotation(rng.normal(0, 0.3, 3)), rng.normal(0, 2, (3, 1))])
        Y = X @ true[:, :3].T + true[:, 3] + rng.normal(0, 0.02, (n, 3))
        if n > 10:
            bad = rng.choice(n, n // 10, replace=False)
            Y[bad] += rng.normal(0, 3.0, (len(bad), 3))
        start = np.ascontiguousarray(np.hstack([_rotation(rng.normal(0, 0.2, 3)), rng.normal(0, 1, (3, 1))]))
        out.append(dict(X=X, Y=Y, pose=start, kind="rotated", n=n, arrangement="as drawn", exact_sum=False, name="rotated, n = %d" % n))
    return out


def bits(x):
    return np.float64(x).tobytes()


# ---- the CPU oracle's side (oracle/lfx_oracle_loc.cpp), for both test files ---------------------------------------------------

PD, PF = C.POINTER(C.c_double), C.POINTER(C.c_float)


def oracle_pairs(case, max_iter=1):
    """orc_loc_optimize_pairs on a family-A case."""
    from oracle import binding as OB
    X, Y, pose = (np.ascontiguousarray(case[k], np.float64) for k in ("X", "Y", "pose"))
    out, err, scale, it, code = np.zeros(12), C.c_double(), C.c_double(), C.c_int(), C.c_int()
    OB.lib().orc_loc_optimize_pairs.restype = C.c_int
    ok = OB.lib().orc_loc_optimize_pairs(OB.ptr(X, PD), OB.ptr(Y, PD), len(X), OB.ptr(pose, PD), max_iter, OB.ptr(out, PD),
                                         C.byref(err), C.byref(scale), C.byref(it), C.byref(code))
    return dict(pose=out.reshape(3, 4), error=err.value, error_scale=scale.value, iteration=it.value, code=code.value, success=bool(ok))


def oracle_scale(errors):
    from oracle import binding as OB
    e = np.ascontiguousarray(errors, np.float64)
    OB.lib().orc_loc_scale.restype = C.c_double
    return float(OB.lib().orc_loc_scale(OB.ptr(e, PD), len(e)))


def oracle_rows(scene_map, kind, pose, points, k=15):
    """orc_loc_edge_residuals (kind 0) / orc_loc_surface_residuals (kind 1) of a cloud at a pose."""
    from oracle import binding as OB
    pts, m = np.ascontiguousarray(points, np.float32), np.ascontiguousarray(scene_map, np.float32)
    pose = np.ascontiguousarray(pose, np.float64)
    width = 3 if kind == 0 else 1
    r, J = np.zeros((len(pts), width)), np.zeros((len(pts), 7 * width))
    f = OB.lib().orc_loc_edge_residuals if kind == 0 else OB.lib().orc_loc_surface_residuals
    if len(pts):
        f(OB.ptr(m, PF), len(m), OB.ptr(pose, PD), k, OB.ptr(pts, PF), len(pts), OB.ptr(r, PD), OB.ptr(J, PD))
    return r, J


def check_result(case, got, want, what, ratios):
    """One family-A result `got` (the oracle's, or the device's) against the restatement `want`: Scale bit for bit and the
    error bit for bit where every order of the additions gives one number (case["exact_sum"]; relative n 2^-53 otherwise) for
    the exact-error kinds, both to 1e-7 at a rotated pose; code and iteration; the pose within the derived bound.  The ratio
    of the pose's difference to B goes to `ratios`."""
    n = case["n"]
    assert np.isfinite(got["pose"]).all() and math.isfinite(got["error"]) and math.isfinite(got["error_scale"]), (what, got)
    if case["kind"] == "rotated":
        assert abs(got["error"] - want["error"]) <= 1e-7 * abs(want["error"]) + 1e-18, (what, got["error"], want["error"])
        assert abs(got["error_scale"] - want["error_scale"]) <= 1e-7 * abs(want["error_scale"]) + 1e-18, what
    else:
        assert bits(got["error_scale"]) == bits(want["error_scale"]), (what, got["error_scale"], want["error_scale"])
        if case["exact_sum"]:
            assert bits(got["error"]) == bits(want["error"]), (what, got["error"], want["error"])
        else:
            assert abs(got["error"] - want["error"]) <= 2.0 ** -53 * n * want["error"], (what, got["error"], want["error"])
    assert not want["excluded"], (what, "a family-A case may not be excluded", want["near_threshold"], want["near_degenerate"], want["near_convergence"])
    assert (got["code"], got["iteration"]) == (want["code"], want["iteration"]), (what, got, want["code"], want["iteration"])
    diff = float(np.abs(got["pose"] - want["pose"]).max())
    assert diff <= want["pose_bound"], (what, diff, want["pose_bound"], want["cond"], want["dx_norm"])
    if want["bound"] > 0:
        ratios.append((diff / want["bound"], what))


# ---- family B -------------------------------------------------------------------------------------------------------------

K_NEIGHBOURS = 15
MIXED_COUNTS = [(n3, n1) for n3 in (40, 41, 42, 43) for n1 in (100, 101, 102, 103)]        # all 16 residues of (3 n3, 3 n3 + n1) mod 4
TINY_COUNTS = [(n3, n1) for n3 in range(4) for n1 in range(4)]                              # (0, 0): the empty scan
SPLIT_COUNTS = [(2100, 4044), (2100, 4045)]                                                # n3 + n1 = 6 144, 6 145


def _features(rings, cols, seeds):
    from lidar_feature_extraction_amd import make_scan
    from oracle import binding as OB
    return [OB.extract(make_scan(rings, cols, seed=s), canonical_ties=False) for s in seeds]


def mixed_scene():
    """Maps (the features of three scans of a 32 x 1024 scene), the clouds every case is sliced from (two other scans') and a
    surface map in which a part of the points is replaced by clusters of 16 coincident ones: a scan point whose 15 nearest
    neighbours coincide has no plane, its row is the zero row."""
    maps = _features(32, 1024, [7590, 7591, 7592])
    scans = _features(32, 1024, [7600, 7601])
    edge_map = np.ascontiguousarray(np.concatenate([m["edge_points"] for m in maps]), np.float32)
    surf_map = np.ascontiguousarray(np.concatenate([m["surface_points"] for m in maps]), np.float32)
    edge = np.ascontiguousarray(np.concatenate([s["edge_points"] for s in scans]), np.float32)
    surf = np.ascontiguousarray(np.concatenate([s["surface_points"] for s in scans]), np.float32)
    assert len(edge) >= 2100 and len(surf) >= 4045, (len(edge), len(surf))
    # coincident clusters: every 16th point of the y > 0 half repeated 16 times, the rest of that half dropped
    half = surf_map[:, 1] > 0
    kept = surf_map[~half]
    seeds = surf_map[half][::16]
    coincident = np.ascontiguousarray(np.concatenate([kept, np.repeat(seeds, 16, axis=0)]), np.float32)
    return dict(edge_map=edge_map, surface_map=surf_map, coincident_map=coincident, edge=edge, surface=surf)


def mixed_cases(scene):
    """Family B: (name, edge cloud, surface cloud, initial pose) per scan.  Poses are pure dyadic translations."""
    edge, surf = scene["edge"], scene["surface"]
    rng = np.random.default_rng(2026)
    shifts = [(1 / 32, -1 / 64, 1 / 128), (-1 / 64, 1 / 32, 0.0), (1 / 128, 1 / 128, -1 / 64), (0.0, -1 / 32, 1 / 64)]
    out = []
    for i, (n3, n1) in enumerate(MIXED_COUNTS + TINY_COUNTS + SPLIT_COUNTS):
        e0, s0 = int(rng.integers(0, len(edge) - n3 + 1)), int(rng.integers(0, len(surf) - n1 + 1))
        if n3 + n1 > 1000:
            e_pts, s_pts = edge[e0:e0 + n3], surf[s0:s0 + n1]
        else:                                            # short clouds: spread over the scan, not a corner of it
            e_pts, s_pts = edge[rng.permutation(len(edge))[:n3]], surf[rng.permutation(len(surf))[:n1]]
        out.append(dict(name="n3 = %d, n1 = %d" % (n3, n1), edge=np.ascontiguousarray(e_pts), surface=np.ascontiguousarray(s_pts),
                        pose=translation(shifts[i % 4]), n3=n3, n1=n1))
    return out


def zero_row_case(scene):
    """The scan that goes against the coincident map: few edge points and the surface points of the y > 0 half first, so that
    the zero rows are the majority of ALL its rows (scale exactly 0)."""
    surf = scene["surface"]
    upper, lower = surf[surf[:, 1] > 0], surf[surf[:, 1] <= 0]
    s_pts = np.ascontiguousarray(np.concatenate([upper[:900], lower[:300]]), np.float32)
    e_pts = np.ascontiguousarray(scene["edge"][:41], np.float32)
    return dict(name="zero rows, n3 = 41, n1 = %d" % len(s_pts), edge=e_pts, surface=s_pts, pose=translation((1 / 64, 1 / 128, -1 / 128)),
                n3=41, n1=len(s_pts))
