"""Voxel-grid Downsample (lfx_voxel_downsample, orc_voxel_downsample): a numpy float32 restatement of the rules of lfx.h,
independent of both implementations, and the edge clouds the CPU and the GPU tests run through them.  Helper module:
no tests here."""
import ctypes as C

import numpy as np

F = np.float32
INT_MAX = 2 ** 31 - 1


def cloud(xyz):
    """(n, 3) coordinates -> (n, 4) float32 records (x, y, z, 1)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    c = np.ones((len(xyz), 4), np.float32)
    c[:, :3] = xyz
    return c


def geometry(points, leaf):
    """(status, finite indices, keys): status 1 where the leaf is too small; the keys (uint32) of the finite points."""
    pts = np.asarray(points, np.float32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        keep = np.nonzero(np.isfinite(pts[:, :3]).all(axis=1))[0]
        q = pts[keep, :3]
        if len(q) == 0:
            return 0, keep, np.zeros(0, np.uint32)
        inv = F(1) / F(leaf)
        lo, hi = q.min(axis=0), q.max(axis=0)
        ext = (hi - lo) * inv
        if not all(e >= 0 and e < F(2.0 ** 63) for e in ext):
            return 1, keep, None
        d = [int(e) + 1 for e in ext]
        if max(d) > INT_MAX or d[0] * d[1] > INT_MAX or d[0] * d[1] * d[2] > INT_MAX:
            return 1, keep, None
        flo, fhi = np.floor(lo * inv), np.floor(hi * inv)
        if not all(a >= F(-2.0 ** 31) and b < F(2.0 ** 31) for a, b in zip(flo, fhi)):
            return 1, keep, None
        min_b = [int(a) for a in flo]
        div = [int(b) - a + 1 for a, b in zip(min_b, fhi)]
        if div[0] * div[1] * div[2] > 2 ** 32:
            return 1, keep, None
        terms = np.floor(q * inv) - np.array(min_b, np.float64).astype(np.float32)   # float32, each >= 0 and < 2^32
        assert (terms >= 0).all() and (terms < F(2.0 ** 32)).all()
        i = terms.astype(np.uint64)
        mul1, mul2 = np.uint64(div[0] % 2 ** 32), np.uint64(div[0] * div[1] % 2 ** 32)
        key = (i[:, 0] + i[:, 1] * mul1 + i[:, 2] * mul2) % np.uint64(2 ** 32)    # (uint64 wraps mod 2^64: the same mod 2^32)
    return 0, keep, key.astype(np.uint32)


def restate(points, leaf):
    """(status, centroids (m, 4) float32): cells in ascending key, the points of a cell summed sequentially in float32 in
    input order from 0.0f, then / (float)count."""
    pts = np.asarray(points, np.float32).reshape(-1, 4)
    st, keep, key = geometry(pts, leaf)
    if st or len(keep) == 0:
        return st, np.zeros((0, 4), np.float32)
    order = np.argsort(key, kind="stable")                  # ascending cell, input order inside a cell
    k = key[order]
    vals = pts[keep[order], :3]
    heads = np.nonzero(np.concatenate([[True], k[1:] != k[:-1]]))[0]
    counts = np.diff(np.append(heads, len(k)))
    s = np.zeros((len(heads), 3), np.float32)
    for r in range(int(counts.max())):                      # one float32 addition per member, in order
        a = counts > r
        s[a] = s[a] + vals[heads[a] + r]
    out = np.ones((len(heads), 4), np.float32)
    out[:, :3] = s / counts.astype(np.float32)[:, None]
    return 0, out


def oracle(points, leaf):
    """orc_voxel_downsample: (rc, centroids)."""
    from oracle import binding as OB
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    out = np.zeros((max(len(pts), 1), 4), np.float32)
    n = C.c_int(0)
    rc = OB.lib().orc_voxel_downsample(OB.ptr(pts, C.POINTER(C.c_float)), len(pts), C.c_float(leaf),
                                       OB.ptr(out, C.POINTER(C.c_float)), C.byref(n))
    return rc, out[:n.value].copy()


def check_against_float64(cloud, leaf, got):
    """One centroid per distinct float32 cell (all points finite, no key wraps), in ascending linear cell index, each within
    a count-scaled rounding bound of the float64 mean of its members (n - 1 float32 additions and one division)."""
    inv = np.float32(1) / np.float32(leaf)
    cells = np.floor(cloud[:, :3] * inv).astype(np.int64)
    cells -= cells.min(axis=0)
    div = cells.max(axis=0) + 1
    lin = cells[:, 0] + cells[:, 1] * div[0] + cells[:, 2] * div[0] * div[1]
    uniq, inverse, counts = np.unique(lin, return_inverse=True, return_counts=True)
    assert len(got) == len(uniq)
    sums = np.zeros((len(uniq), 3))
    amax = np.zeros((len(uniq), 3))
    x = cloud[:, :3].astype(np.float64)
    np.add.at(sums, inverse, x)
    np.maximum.at(amax, inverse, np.abs(x))
    mean = sums / counts[:, None]
    bound = (counts[:, None] + 1) * 2.0 ** -24 * amax * 1.01 + 1e-45
    assert (np.abs(got[:, :3].astype(np.float64) - mean) <= bound).all()
    assert (got[:, 3] == 1).all()


# ------------------------------------------------------------------------------------------------ the edge clouds
def limit_cases():
    """(name, cloud, leaf): the limits of "leaf too small" and of the index arithmetic."""
    f32max = float(np.finfo(np.float32).max)
    rng = np.random.default_rng(7)
    z_axis = lambda z_top, extra: cloud([[0.9, 0.9, 0.0], [1.1, 0.9, 0.0], [0.9, 1.1, z_top], [1.1, 1.1, z_top]]
                                        + [[0.9 + 0.2 * (j % 2), 0.9 + 0.2 * (j // 2 % 2), z] for j, z in enumerate(extra)])
    mid = list(rng.uniform(0, 1.0e9, 20).astype(np.float32))
    yield "straddle", cloud([[0.5] * 3, [1290.2] * 3, [1290.1] * 3]), 1.0
    yield "product_1290_cubed", cloud([[0, 0, 0], [1289.5] * 3, [645.2, 17.0, 1200.0], [3.0, 1289.0, 0.5]]), 1.0
    yield "product_1291_cubed", cloud([[0, 0, 0], [1290.5] * 3, [645.2, 17.0, 1200.0]]), 1.0
    yield "axis_int_max", cloud([[0, 0, 0], [2147483000.0, 0, 0], [1.0e9, 0, 0], [1.0e9 + 64, 0, 0], [123456789.0, 0, 0]]), 1.0
    yield "axis_above_int_max", cloud([[-1.0e9, 0, 0], [1.2e9, 0, 0]]), 1.0
    yield "axis_both_signs_rounding", cloud([[-1.0e9, 0, 0], [1.0e9, 0, 0], [-999999936.0, 0, 0], [999999872.0, 0, 0], [0.5, 0, 0],
                                             [-0.5, 0, 0], [17.0, 0, 0]]), 1.0
    yield "div_product_below_2_32", z_axis(1073741760.0, mid + [1073741760.0 - 64]), 1.0
    yield "div_product_2_32", z_axis(1073741760.0 + 64.0, mid), 1.0                     # 4 * (2^30 + 1) cells: above 2^32
    yield "div_product_above_2_32", z_axis(1.1e9, mid), 1.0
    yield "leaf_1e-30", cloud([[0, 0, 0], [1, 0, 0]]), 1e-30
    yield "leaf_1e-30_one_point", cloud([[0.5, 0.25, -0.125]]), 1e-30
    yield "leaf_denormal_one_point", cloud([[0.5, 0.25, -0.125]]), 1e-40
    yield "leaf_denormal_origin", cloud([[0, 0, 0]]), 1e-40
    yield "leaf_flt_max", cloud([[-3.0, 2.0, 1.0], [5.0, -7.0, 0.0], [0.0, 0.0, -0.0], [1e30, -1e30, 3.0]]), f32max
    yield "leaf_inf", cloud([[-3.0, 2.0, 1.0], [5.0, -7.0, 0.0], [1e30, -1e30, 3.0]]), float("inf")
    yield "leaf_inf_huge_extent", cloud([[-3e38, 0, 0], [3e38, 0, 0]]), float("inf")
    yield "leaf_flt_max_huge_extent", cloud([[-3e38, 1, 0], [3e38, 2, 0], [0, 0, 0]]), f32max
    for leaf in (1.0, 0.5, 0.01):
        for sign in (1, -1):
            c = 3e9 * leaf * sign
            yield "far_%g_%d" % (leaf, sign), cloud([[c, 0, 0], [c + 64 * sign, 1, 1], [c, 0.5, 0.25]]), leaf
            yield "far_y_%g_%d" % (leaf, sign), cloud([[0, c, 0], [0, c, 1]]), leaf
    # just inside int32 at the far end: the cell arithmetic rounds, the cloud is filtered
    yield "near_int_max_cell", cloud([[2147483000.0, 0, 0], [2147483520.0, 0, 0], [2147483136.0, 3, 0]]), 1.0
    yield "near_int_min_cell", cloud([[-2147483648.0, 0, 0], [-2147483000.0, 0, 0], [-2147483136.0, 3, 0]]), 1.0


def boundary_cases():
    """Points at exact multiples of the leaf, one ulp either side, negative values and -0.0."""
    rng = np.random.default_rng(5)
    for leaf in (0.1, 0.3, 1.0 / 3.0, 0.01, 0.25, 1.0, 2.0):
        lf = F(leaf)
        ks = np.arange(-6, 7, dtype=np.float32)
        on = ks * lf
        vals = np.concatenate([on, np.nextafter(on, F(np.inf)), np.nextafter(on, F(-np.inf)), [F(0.0), F(-0.0)]]).astype(np.float32)
        pts = vals[rng.integers(0, len(vals), (900, 3))]
        pts[:len(vals), 0] = vals                               # every value once on each axis
        pts[:len(vals), 1] = vals[::-1]
        pts[:len(vals), 2] = vals
        pts[-4:] = [[-0.0, -0.0, -0.0], [0.0, -0.0, 0.0], [-0.0, 0.0, -0.0], [-0.0, -0.0, -0.0]]
        yield "boundary_%g" % leaf, cloud(pts), leaf
        yield "boundary_negative_zero_%g" % leaf, cloud([[-0.0, -0.0, -0.0], [-0.0, -0.0, -0.0]]), leaf


def far_cases():
    """coordinate / leaf above 2^24: the float cell arithmetic rounds, the cloud is within the limits."""
    rng = np.random.default_rng(9)
    for leaf, centre in ((0.01, 2.0e5), (1.0, 3.0e7), (0.1, -5.0e6), (0.25, 1.0e8)):
        p = centre + rng.normal(0, 40 * leaf, (3000, 3))
        yield "far_%g_%g" % (leaf, centre), cloud(p), leaf


def _cells_cloud(rng, n_cells, n, leaf=1.0, shape=(40, 40, 40)):
    """n points (n >= n_cells) over exactly n_cells distinct cells of a grid of `shape`, in random order."""
    ids = rng.choice(int(np.prod(shape)), n_cells, replace=False)
    pick = np.concatenate([np.arange(n_cells), rng.integers(0, n_cells, n - n_cells)])
    rng.shuffle(pick)
    ijk = np.stack(np.unravel_index(ids[pick], shape), axis=1).astype(np.float32)
    return cloud((ijk + rng.uniform(0.05, 0.95, (n, 3)).astype(np.float32)) * F(leaf))


def form_cases():
    """The small form (<= 12 288 points) against the general one, and cell heads in LDS (< 2 048 cells) or in memory."""
    rng = np.random.default_rng(13)
    for n in (1023, 1024, 1025, 12287, 12288, 12289):
        yield "n_%d" % n, cloud(rng.normal(0, 6.0, (n, 3))), 0.5
    yield "one_cell_12288", cloud(rng.uniform(2.0, 2.999, (12288, 3))), 1.0
    ijk = np.stack(np.unravel_index(rng.permutation(12288), (16, 24, 32)), axis=1).astype(np.float32)
    yield "distinct_12288", cloud(ijk + F(0.5)), 1.0
    yield "distinct_12289", cloud(np.concatenate([ijk + F(0.5), [[100.5, 0.5, 0.5]]])), 1.0
    for cells in (2046, 2047, 2048, 2049):
        yield "cells_%d" % cells, _cells_cloud(rng, cells, 9000), 1.0
        yield "cells_%d_general" % cells, _cells_cloud(rng, cells, 14000), 1.0


def radix_cases():
    """Largest keys at 255 / 256, 65 535 / 65 536 and 2^24 - 1 / 2^24, in both forms: 1, 2, 3 and 4 radix passes."""
    rng = np.random.default_rng(17)
    for top in (255, 256, 65535, 65536, 2 ** 24 - 1, 2 ** 24):
        for n in (3000, 14000):
            # key = x + 256 y (x in cells 0 .. 255): 0, the largest, both sides of every byte boundary below it, then random
            edges = [0, top, 255] + [v + e for v in (256, 65536, 2 ** 24) if v <= top for e in (-1, 0)]
            key = np.concatenate([edges, rng.integers(0, top + 1, n - len(edges))])
            c = np.stack([key % 256, key // 256, np.zeros(n)], axis=1) + 0.5
            yield "key_%d_n%d" % (top, n), cloud(c[rng.permutation(n)]), 1.0


def nonfinite_cases():
    """NaN and +-inf in each coordinate, as the first point, the last point and as every point."""
    rng = np.random.default_rng(19)
    base = {"small": cloud(rng.normal(0, 5, (500, 3))), "general": cloud(rng.normal(0, 5, (13000, 3)))}
    for form, c in base.items():
        for bad in (np.nan, np.inf, -np.inf):
            for axis in range(3):
                for where in ("first", "last"):
                    d = c.copy()
                    d[0 if where == "first" else -1, axis] = bad
                    yield "%s_%s_%s_%d" % (form, where, bad, axis), d, 0.5
    for bad in (np.nan, np.inf, -np.inf):
        for n in (1, 7, 13000):
            d = cloud(rng.normal(0, 5, (n, 3)))
            d[np.arange(n), rng.integers(0, 3, n)] = bad
            yield "all_%s_%d" % (bad, n), d, 0.5
    d = cloud(rng.normal(0, 5, (40, 3)))
    d[::2, 0] = np.nan
    d[1::2, 2] = -np.inf
    yield "all_mixed", d, 0.5


def insert_nonfinite(rng, c, count):
    """The cloud with `count` non-finite points inserted at random places (the clean cloud is a subsequence of it)."""
    bad = rng.normal(0, 5, (count, 4)).astype(np.float32)
    bad[:, 3] = 1
    kinds = np.array([np.nan, np.inf, -np.inf], np.float32)
    for j in range(count):
        axes = rng.random(3) < 0.5
        axes[rng.integers(0, 3)] = True
        bad[j, :3][axes] = kinds[rng.integers(0, 3, axes.sum())]
    at = np.sort(rng.integers(0, len(c) + 1, count))
    return np.insert(c, at, bad, axis=0)


def all_cases():
    for gen in (limit_cases, boundary_cases, far_cases, form_cases, radix_cases, nonfinite_cases):
        yield from gen()


def draw(rng):
    """One random cloud and leaf over the generators above (tools/stress_downsample.py, a slice in the GPU test)."""
    kind = rng.choice(["gauss", "far", "cells", "lattice", "nonfinite", "line"])
    n = int(rng.choice([int(rng.integers(1, 3000)), int(rng.integers(3000, 12289)), int(rng.integers(12289, 30000))]))
    leaf = float(F(10.0 ** rng.uniform(-2.5, 0.7)))
    if kind == "gauss":
        return cloud(rng.normal(0, 10.0 ** rng.uniform(-1, 2), (n, 3))), leaf
    if kind == "far":
        centre = rng.choice([-1, 1]) * 10.0 ** rng.uniform(4, 8.5) * leaf
        return cloud(centre + rng.normal(0, 30 * leaf, (n, 3))), leaf
    if kind == "cells":
        cells = int(rng.integers(1, min(n, 5000) + 1))
        return _cells_cloud(rng, cells, n, leaf, shape=(30, 30, 30)), leaf
    if kind == "lattice":                                       # points on multiples of the leaf and one ulp off
        on = np.arange(-20, 21, dtype=np.float32) * F(leaf)
        vals = np.concatenate([on, np.nextafter(on, F(np.inf)), np.nextafter(on, F(-np.inf))])
        return cloud(vals[rng.integers(0, len(vals), (n, 3))]), leaf
    if kind == "nonfinite":
        c = cloud(rng.normal(0, 5, (n, 3)))
        return insert_nonfinite(rng, c, int(rng.integers(1, 50))), leaf
    t = rng.uniform(0, 1, n)[:, None]                           # a long line: large keys
    return cloud(t * rng.uniform(-1, 1, 3) * 10.0 ** rng.uniform(2, 5)), leaf
