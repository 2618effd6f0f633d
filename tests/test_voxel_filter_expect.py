"""The voxel filter's restatement (tests/voxel_filter_restatement.py) held to cases written out by hand, and two properties that
follow from the model (include/lfx.h, the voxel filter section).  No GPU."""
import numpy as np

from tests import voxel_filter_restatement as VF

F = np.float32


def _one(points, leaf, **kw):
    return VF.filtered(np.asarray(points, np.float32).reshape(-1, 4), leaf, **kw)


def test_records_on_and_beside_a_voxel_boundary():
    """leaf 0.5: inv is 2.0 exactly.  A record at k * leaf opens voxel k, one float below it lies in voxel k - 1, one float above
    it in voxel k again; a lone record comes back as it went in (q is exact for these)."""
    leaf = 0.5
    assert VF.inverse(leaf) == F(2.0)
    for k in (-3, 0, 5):
        at = F(k * leaf)
        below, above = np.nextafter(at, F(-np.inf)), np.nextafter(at, F(np.inf))
        assert below < at < above
        v = VF.voxel(np.array([below, at, above], F), VF.inverse(leaf))
        assert v.tolist() == [k - 1, k, k], (k, v)
        # x varies, y and z sit in voxel 0: `below` alone in its voxel, `at` and `above` together
        pts = [[below, 0.1, 0.2, 9.0], [at, 0.1, 0.2, 9.0], [above, 0.1, 0.2, 9.0]]
        cloud, counts, res = _one(pts, leaf)
        assert counts.tolist() == [1, 2] and res["n_voxels"] == 2 and res["n_accumulated"] == 3
        # (k = 0: `below` is the smallest negative float, 2^-149; its q rounds to 2^24 and it comes back as 0 -- last lines)
        assert cloud[0, 0] == (below if k else 0.0) and cloud[:, 3].tolist() == [1.0, 1.0]
        # the pair's centroid: (at + above) / 2 in exact arithmetic, rounded once
        assert cloud[1, 0] == F((np.float64(at) + np.float64(above)) / 2.0)
    # the smallest negative float lies in voxel -1 with q = 2^24 exactly, and comes back as 0
    tiny = np.nextafter(F(0), F(-1))
    assert VF.q_of(tiny, F(2.0), -1) == 1 << 24
    cloud, counts, _ = _one([[tiny, 0.1, 0.1, 0.0]], leaf)
    assert cloud[0, 0] == 0.0 and counts.tolist() == [1]


def test_signed_zeros_share_voxel_zero_and_give_plus_zero():
    cloud, counts, res = _one([[0.0, -0.0, 0.0, 1.0], [-0.0, 0.0, -0.0, 2.0]], 0.4)
    assert counts.tolist() == [2] and res["n_voxels"] == 1
    assert cloud.tobytes() == np.array([[0.0, 0.0, 0.0, 1.0]], F).tobytes()


def test_the_voxel_limit():
    """leaf 1: voxel 2^20 - 1 is the last one kept, 2^20 is out of range; -(2^20 - 1) is kept, -2^20 is out of range"""
    top = float(VF.LIMIT)
    pts = [[top - 0.5, 0.5, 0.5, 0.0], [top, 0.5, 0.5, 0.0], [0.5, -(top - 1.0), 0.5, 0.0], [0.5, -(top - 0.5), 0.5, 0.0],
           [0.5, 0.5, 3.0e38, 0.0]]
    assert VF.voxel(F(top - 0.5), F(1.0)) == VF.LIMIT - 1 and VF.voxel(F(-(top - 0.5)), F(1.0)) == -VF.LIMIT
    cloud, counts, res = _one(pts, 1.0)
    assert res["n_records"] == 5 and res["n_accumulated"] == 2 and res["n_out_of_range"] == 3 and res["n_nonfinite"] == 0
    assert cloud.tolist() == [[top - 0.5, 0.5, 0.5, 1.0], [0.5, -(top - 1.0), 0.5, 1.0]]
    # a finite record whose product with inv overflows is out of range, not non-finite
    _, _, res = _one([[3.0e38, 0.0, 0.0, 0.0]], 0.2)
    assert res["n_out_of_range"] == 1 and res["n_nonfinite"] == 0
    # the key keeps the sign of every axis: 21 bits each, bit 63 set
    assert VF.key(-1, 0, 1) == (1 << 63) | 0x1FFFFF | (1 << 42)


def test_records_that_are_not_finite_are_skipped_and_take_a_rank():
    bad = []
    for axis in range(3):
        for value in (np.nan, np.inf, -np.inf):
            p = [1.0, 1.0, 1.0, 5.0]
            p[axis] = value
            bad.append(p)
    pts = bad[:4] + [[1.1, 1.1, 1.1, np.nan]] + bad[4:] + [[7.0, 7.0, 7.0, np.inf]]
    f = VF.Filter(4, len(pts))
    f.reset(1.0)
    assert f.add(pts) is None
    status, cloud, counts, res = f.emit()
    assert status == "ok" and res == dict(n_records=11, n_accumulated=2, n_nonfinite=9, n_out_of_range=0, n_table_full=0, n_voxels=2, n_written=2)
    assert cloud.tolist() == [[F(1.1), F(1.1), F(1.1), 1.0], [7.0, 7.0, 7.0, 1.0]] and counts.tolist() == [1, 1]
    # ranks were consumed by the skipped records: the ninth record may still come, the twelfth may not
    assert f.add([[0.0, 0.0, 0.0, 0.0]]) == "capacity" and f.base == 11


def test_min_points_and_counts_by_hand():
    a, b, c = [0.5, 0.5, 0.5, 0.0], [1.5, 0.5, 0.5, 0.0], [2.5, 0.5, 0.5, 0.0]
    pts = [c, b, c, a, c, b]                       # first appearance: c, b, a with 3, 2, 1 records
    for min_points, want in ((1, [3, 2, 1]), (2, [3, 2]), (3, [3]), (4, [])):
        cloud, counts, res = _one(pts, 1.0, min_points=min_points)
        assert counts.tolist() == want and res["n_voxels"] == 3 and res["n_written"] == len(want)
        assert cloud[:, 0].tolist() == [2.5, 1.5, 0.5][:len(want)]


def test_a_full_table_loses_records_and_refuses_the_emit():
    """16 entries: 16 voxels of 3 records fit; of 17 the last to appear finds no entry, and its 3 records are counted"""
    for n_voxels, full in ((16, 0), (17, 3)):
        pts = np.tile(VF.centre_points([(k, 0, 0) for k in range(n_voxels)]), (3, 1))
        f = VF.Filter(4, len(pts))
        f.reset(1.0)
        assert f.add(pts) is None
        status, cloud, _, res = f.emit()
        assert res["n_table_full"] == full and res["n_voxels"] == 16 and res["n_accumulated"] == len(pts) - full
        assert (status, len(cloud)) == (("ok", 16) if not full else ("capacity", 0))
    f.reset(1.0)                                   # more voxels than capacity_points: refused as well, nothing lost
    f.add(VF.centre_points([(0, 0, 0), (1, 0, 0)]))
    assert f.emit(capacity=1)[0] == "capacity" and f.emit(capacity=2)[0] == "ok"


def test_the_hash_is_the_kernels():
    """vf_home: the top bits of key * 0x9E3779B97F4A7C15 mod 2^64; by hand for the origin's key 2^63: the product is
    2^63 * (odd) mod 2^64 = 2^63, whose top 4 bits are 8"""
    assert VF.home(VF.key(0, 0, 0), 4) == 8 and VF.home(VF.key(0, 0, 0), 10) == 512
    got = VF.sharing_home(4, 15, 8)
    assert len(set(got)) == 8 and all(VF.home(VF.key(*v), 4) == 15 for v in got)


def _cloud(seed, n=4000):
    rng = np.random.default_rng(seed)
    p = rng.normal(0, 3, (n, 4)).astype(F)
    p[::7, :3] *= F(40.0)
    return p


def test_a_lone_record_comes_back_within_the_q_rounding_and_one_ulp():
    """|centroid - p| <= leaf 2^-25 (the rounding of q) + 1 ulp of the coordinate (the final rounding to float)"""
    for leaf in (0.2, 0.4, 0.5, 1.0):
        inv = VF.inverse(leaf)
        p = np.concatenate([_cloud(3)[:, :3].reshape(-1), np.array([0.0, -0.0, 1e-30, -1e-30, 209715.1, -209715.1], F)])
        v = VF.voxel(p, inv).astype(np.int64)
        got = VF.centroid(v, VF.q_of(p, inv, v), np.ones(len(p), np.int64), inv)
        err = np.abs(got.astype(np.float64) - p.astype(np.float64))
        bound = np.float64(F(leaf)) * 2.0 ** -25 + np.spacing(np.abs(p)).astype(np.float64)
        assert (err <= bound).all(), (leaf, float((err / bound).max()))


def test_the_set_is_invariant_under_permutation_and_the_order_follows_it():
    pts = _cloud(11)
    pts[5] = [np.nan, 0, 0, 0]
    leaf = 0.4
    cloud, counts, res = VF.filtered(pts, leaf)
    assert 500 < len(cloud) < len(pts) and counts.max() > 3 and int(counts.sum()) == res["n_accumulated"] == len(pts) - 1
    rows = {c.tobytes(): int(n) for c, n in zip(cloud, counts)}
    assert len(rows) == len(cloud)
    rng = np.random.default_rng(12)
    for _ in range(3):
        perm = rng.permutation(len(pts))
        c2, n2, r2 = VF.filtered(pts[perm], leaf)
        assert {c.tobytes(): int(n) for c, n in zip(c2, n2)} == rows and r2 == res
        # the order: voxels by their first appearance in the permuted input, worked out apart from the filter
        v = VF.voxel(pts[perm][:, :3], VF.inverse(leaf))
        ok = np.isfinite(v).all(axis=1)
        _, first = np.unique(v[ok], axis=0, return_index=True)
        order_in = np.nonzero(ok)[0][np.sort(first)]                 # the record that opened each voxel, in order
        # each voxel's place in the emit of the unpermuted input (its first appearance there)
        orig_first = {}
        v0 = VF.voxel(pts[:, :3], VF.inverse(leaf))
        for i, x in enumerate(map(tuple, v0.tolist())):
            if np.isfinite(x).all():
                orig_first.setdefault(x, len(orig_first))
        want = np.array([orig_first[tuple(x)] for x in v[order_in].tolist()])
        assert c2.tobytes() == cloud[want].tobytes() and n2.tolist() == counts[want].tolist()
