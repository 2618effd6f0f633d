"""The segmentation section of include/lfx.h without a device: the numpy restatement (tests/segment_restatement.py) pinned
by cases written out by hand -- a 2 x 4 image with every class in it, the column boundaries, the ground test at equality,
the join test, the class thresholds, two records in one cell -- the host-only entry points, and a scene check."""
import ctypes as C

import numpy as np
import pytest

from tests import segment_restatement as R

f32 = np.float32


def _seg(cfg, records):
    c = R.cloud_of(records)
    return R.segment_cloud(cfg, c)


def test_defaults_tables_and_refusals():
    from lidar_feature_extraction_amd import binding as B
    L = B.load()
    cfg = B.SegmentConfig()
    L.lfx_segment_default_config(C.byref(cfg))
    L.lfx_segment_default_config(None)                     # a no-op
    got = [getattr(cfg, n) for n, _ in B.SegmentConfig._fields_]
    assert got == [16, 1800, f32(0.034906585), 1.0, 100.0, 0, 7, f32(0.17632698), f32(1.7320508), 30, 5, 3]
    assert (B.SEG_NONE, B.SEG_GROUND, B.SEG_SEGMENT, B.SEG_CLUTTER) == (0, 1, 2, 3)
    assert B.SEG_EDGE_MASK_DEFAULT == 4 and B.SEG_SURFACE_MASK_DEFAULT == 6
    cs, sn, consts = R.segment_tables(cfg)
    W = 1800
    m = np.arange(W, dtype=np.float64)
    angle = -np.pi + ((2.0 * np.pi) * m) / float(W)
    assert np.abs(cs - np.cos(angle)).max() < 1e-15 and np.abs(sn - np.sin(angle)).max() < 1e-15
    step = (2.0 * np.pi) / float(W)
    assert np.allclose(consts, [np.sin(step), np.cos(step), np.sin(float(f32(0.034906585))), np.cos(float(f32(0.034906585)))], rtol=0, atol=1e-15)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    a, b, c4 = np.zeros(4096), np.zeros(4096), np.zeros(4)
    assert L.lfx_segment_tables(None, p(a), p(b), p(c4)) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_segment_tables(C.byref(cfg), None, p(b), p(c4)) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_segment_tables(C.byref(cfg), p(a), None, p(c4)) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_segment_tables(C.byref(cfg), p(a), p(b), None) == B.ERR_INVALID_ARGUMENT
    nan, inf = float("nan"), float("inf")
    for fields in (dict(n_rows=0), dict(n_rows=129), dict(n_columns=2), dict(n_columns=1801), dict(n_columns=4098), dict(row_step=0.0),
                   dict(row_step=-0.1), dict(row_step=nan), dict(row_step=inf), dict(min_range=0.0), dict(min_range=-1.0), dict(min_range=100.0),
                   dict(min_range=nan), dict(max_range=inf), dict(max_range=nan), dict(ground_first_row=8), dict(ground_last_row=16),
                   dict(ground_tan=-0.1), dict(ground_tan=nan), dict(ground_tan=inf), dict(segment_tan=0.0), dict(segment_tan=nan),
                   dict(segment_tan=inf), dict(segment_min_points=0), dict(small_min_points=0), dict(small_min_rows=0)):
        a[:] = 7.0
        assert L.lfx_segment_tables(C.byref(R.config(**fields)), p(a), p(b), p(c4)) == B.ERR_INVALID_ARGUMENT, fields
        assert (a == 7.0).all(), fields
    for fields in (dict(n_rows=1, ground_last_row=0), dict(n_rows=128), dict(n_columns=4), dict(n_columns=4096), dict(ground_tan=0.0),
                   dict(ground_first_row=7), dict(ground_last_row=15)):
        assert L.lfx_segment_tables(C.byref(R.config(**fields)), p(a), p(b), p(c4)) == 0, fields
    null = C.c_void_p(0)
    assert L.lfx_segment_batch(null, C.byref(cfg), 1, null, null, null, null) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_pack_features_segmented(null, null, 4, 6, null, null, null, null, 0, null) == B.ERR_INVALID_ARGUMENT
    with pytest.raises(TypeError):
        R.config(no_such_field=1)


def test_a_two_by_four_image_with_every_class():
    """W = 4: columns of 90 degrees from -pi, so +x with y = +0.0 opens column 2 and equal ranges do not join across columns
    (cot 45 degrees < tan 60 degrees); the rows join (2 degrees apart)."""
    cfg = R.config(n_rows=2, n_columns=4, ground_first_row=0, ground_last_row=1, small_min_points=2, small_min_rows=2)
    az = lambda col: -np.pi + (2.0 * np.pi) * (col + 0.5) / 4.0
    at = lambda col, rho, z, row: (f32(rho * np.cos(az(col))), f32(rho * np.sin(az(col))), f32(z), row)
    records = [
        at(0, 5.0, -1.0, 0), at(0, 10.0, -1.0, 1),        # column 0: flat between the rows -- ground
        at(1, 10.0, 0.0, 0), at(1, 10.01, 0.3, 1),        # column 1: steep, and close in range -- one component over two rows
        at(2, 10.0, 0.0, 0),                              # column 2: alone -- clutter
        at(3, 200.0, 0.0, 0),                             # out of range
        (f32(np.nan), f32(1.0), f32(0.0), 1),             # not finite
        at(2, 10.0, 0.0, 2),                              # a row the image does not have
        at(1, 30.0, 0.0, 0),                              # a second record in cell (0, 1): loses, inherits
        (f32(0.0), f32(0.0), f32(5.0), 0),                # on the z axis
    ]
    cls, ids, counts = _seg(cfg, records)
    assert cls.tolist() == [1, 1, 2, 2, 3, 0, 0, 0, 2, 0]
    n = R.NO_ID
    assert ids.tolist() == [n, n, 1, 1, 2, n, n, n, 1, n]
    assert counts.tolist() == [4, 2, 3, 1]
    assert [a.tolist() for a in _seg(cfg, [])] == [[], [], [0, 0, 0, 0]]                # an empty scan
    # the same records in another order: the same classes, record for record
    order = [9, 8, 7, 6, 5, 4, 3, 2, 1, 0]
    cls2, ids2, _ = _seg(cfg, [records[i] for i in order])
    assert cls2.tolist() == [cls[i] for i in order] and ids2.tolist() == [ids[i] for i in order]


def test_column_boundaries():
    cfg = R.config(n_rows=1, n_columns=4, ground_last_row=0)
    t = 1e-30
    cases = [((1, t), 2), ((1, -t), 1), ((1, 0.0), 2), ((1, -0.0), 2), ((-1, 0.0), 3), ((-1, -0.0), 3), ((-1, -t), 0), ((-1, t), 3),
             ((1e-3, 1), 2), ((-1e-3, 1), 3), ((1e-3, -1), 1), ((-1e-3, -1), 0), ((5, 5), 2), ((-5, 5), 3), ((-5, -5), 0), ((5, -5), 1)]
    xy = np.array([c[0] for c in cases], np.float32)
    assert R.columns(cfg, xy[:, 0], xy[:, 1]).tolist() == [c[1] for c in cases]
    # the axes themselves land where the table's rounded cos(+-pi/2) says: one of the two columns that meet there
    for (x, y), either in (((0, 1), (2, 3)), ((0, -1), (0, 1))):
        assert int(R.columns(cfg, [f32(x)], [f32(y)])[0]) in either
    # centre_record lands in its cell for every column of a fine grid
    fine = R.config(n_columns=1800)
    recs = [R.centre_record(fine, 0, c, 10.0) for c in range(1800)]
    assert R.columns(fine, [r[0] for r in recs], [r[1] for r in recs]).tolist() == list(range(1800))


@pytest.mark.parametrize("W", [4, 60, 1800, 4096])
def test_the_bisection_is_the_plain_count(W):
    """On 10^5 random records the bisection gives m0 + #{ m in m0+1 .. m0+W/2-1 : cross(m) >= 0 }: the crosses of a record
    change sign once over its half circle."""
    rng = np.random.default_rng(W)
    n = 100000
    x, y = rng.normal(0, 20, n).astype(np.float32), rng.normal(0, 20, n).astype(np.float32)
    y[:1000] = rng.choice(np.array([0.0, -0.0], np.float32), 1000)
    x[1000:2000] = 0.0
    cfg = R.config(n_columns=W)
    got = R.columns(cfg, x, y)
    differ = 0
    for a in range(0, n, 4000):
        ge = R.cross_signs(cfg, x[a:a + 4000], y[a:a + 4000])
        upper = y[a:a + 4000] >= f32(0.0)
        count = np.where(upper, W // 2 + ge[:, W // 2 + 1:].sum(axis=1), ge[:, 1:W // 2].sum(axis=1))
        differ += int((count != got[a:a + 4000]).sum())
    print("W = %d: %d of %d records where the bisection and the count differ" % (W, differ, n))
    assert differ == 0
    assert got.min() >= 0 and got.max() <= W - 1


def test_ground_at_equality():
    """ground_tan = 0.5 (g2 = 0.25 exactly), dx = 2, dz = 1: 1 <= 0.25 * 4 holds; one float more of dz and it does not."""
    cfg = R.config(n_rows=2, n_columns=4, ground_first_row=0, ground_last_row=1, ground_tan=0.5)
    above = np.nextafter(f32(1.0), f32(2.0))
    assert _seg(cfg, [(f32(3), f32(0), f32(0), 0), (f32(5), f32(0), f32(1), 1)])[0].tolist() == [1, 1]
    assert _seg(cfg, [(f32(3), f32(0), f32(0), 0), (f32(5), f32(0), above, 1)])[0].tolist() == [3, 3]
    assert _seg(cfg, [(f32(5), f32(0), f32(1), 1), (f32(3), f32(0), f32(0), 0)])[0].tolist() == [1, 1]       # (whichever comes first)
    # one cell of the pair empty; the pair in another column
    assert _seg(cfg, [(f32(3), f32(0), f32(0), 0)])[0].tolist() == [3]
    assert _seg(cfg, [(f32(3), f32(0), f32(0), 0), (f32(-5), f32(0), f32(0), 1)])[0].tolist() == [3, 3]
    # first = last: no pairs
    none = R.config(n_rows=2, n_columns=4, ground_first_row=0, ground_last_row=0, ground_tan=0.5)
    assert _seg(none, [(f32(3), f32(0), f32(0), 0), (f32(5), f32(0), f32(1), 1)])[0].tolist() == [3, 3]
    none = R.config(n_rows=2, n_columns=4, ground_first_row=1, ground_last_row=1, ground_tan=0.5)
    assert _seg(none, [(f32(3), f32(0), f32(0), 0), (f32(5), f32(0), f32(1), 1)])[0].tolist() == [3, 3]
    # rows outside first .. last are not tested: the pair (1, 2) with first = 0, last = 1
    three = R.config(n_rows=3, n_columns=4, ground_first_row=0, ground_last_row=1, ground_tan=0.5)
    assert _seg(three, [(f32(3), f32(0), f32(0), 1), (f32(5), f32(0), f32(1), 2)])[0].tolist() == [3, 3]
    assert _seg(three, [(f32(3), f32(0), f32(0), 0), (f32(5), f32(0), f32(1), 1), (f32(7), f32(0), f32(2), 2)])[0].tolist() == [1, 1, 3]


def test_join_test():
    """W = 64: adjacent columns 5.6 degrees apart join up to d1 / d2 = sin a / tan 60 + cos a = 1.0518."""
    base = dict(n_rows=2, n_columns=64, ground_first_row=0, ground_last_row=0, small_min_points=2, small_min_rows=1)
    cfg = R.config(**base)
    _, _, consts = R.segment_tables(cfg)
    limit = consts[0] / float(f32(1.7320508)) + consts[1]
    assert abs(limit - 1.0518) < 1e-4
    pair = lambda ra, rb, ca=10, cb=11, rowa=0, rowb=0: [R.centre_record(cfg, rowa, ca, ra), R.centre_record(cfg, rowb, cb, rb)]
    assert _seg(cfg, pair(10.0, 10.4))[0].tolist() == [2, 2] and _seg(cfg, pair(10.0, 10.4))[1].tolist() == [10, 10]
    assert _seg(cfg, pair(10.4, 10.0))[0].tolist() == [2, 2]
    assert _seg(cfg, pair(10.0, 10.7))[0].tolist() == [3, 3] and _seg(cfg, pair(10.0, 10.7))[1].tolist() == [10, 11]
    assert _seg(cfg, pair(10.7, 10.0))[0].tolist() == [3, 3]
    assert _seg(cfg, pair(10.0, 10.0))[0].tolist() == [2, 2]                                   # d1 == d2
    assert _seg(cfg, pair(10.0, 10.0, ca=10, cb=12))[0].tolist() == [3, 3]                     # not neighbours
    assert _seg(cfg, pair(10.0, 10.0, ca=10, cb=11, rowb=1))[0].tolist() == [3, 3]             # diagonal
    # the rows: 2 degrees apart, d1 / d2 up to sin / tan 60 + cos = 1.0195
    assert _seg(cfg, pair(10.0, 10.1, ca=10, cb=10, rowb=1))[0].tolist() == [2, 2]
    assert _seg(cfg, pair(10.0, 10.3, ca=10, cb=10, rowb=1))[0].tolist() == [3, 3]
    # the seam pair (W - 1, 0), once, in either order of the records; the label is column 0's
    for recs in (pair(10.0, 10.2, ca=63, cb=0), pair(10.0, 10.2, ca=0, cb=63)):
        cls, ids, _ = _seg(cfg, recs)
        assert cls.tolist() == [2, 2] and ids.tolist() == [0, 0]
    cls, ids, _ = _seg(cfg, pair(10.0, 10.2, ca=63, cb=0, rowa=1, rowb=1))
    assert cls.tolist() == [2, 2] and ids.tolist() == [64, 64]
    # W = 4: columns 90 degrees apart never join at equal range (the seam neither)
    four = R.config(**dict(base, n_columns=4))
    assert _seg(four, [R.centre_record(four, 0, c, 10.0) for c in range(4)])[0].tolist() == [3, 3, 3, 3]


def test_class_thresholds():
    cfg = R.config(n_rows=4, n_columns=64, ground_first_row=0, ground_last_row=0)
    run = lambda n: [(0, c) for c in range(20, 20 + n)]
    assert set(R.segment_cloud(cfg, R.image_cloud(cfg, run(29)))[0].tolist()) == {3}
    cls, ids, counts = R.segment_cloud(cfg, R.image_cloud(cfg, run(30)))
    assert set(cls.tolist()) == {2} and set(ids.tolist()) == {20} and counts.tolist() == [0, 0, 30, 0]
    four = [(0, 5), (1, 5), (2, 5), (2, 6)]
    assert set(R.segment_cloud(cfg, R.image_cloud(cfg, four))[0].tolist()) == {3}
    cls, ids, _ = R.segment_cloud(cfg, R.image_cloud(cfg, four + [(2, 7)]))
    assert set(cls.tolist()) == {2} and set(ids.tolist()) == {5}
    two_rows = [(0, 5), (0, 6), (0, 7), (1, 5), (1, 6)]
    assert set(R.segment_cloud(cfg, R.image_cloud(cfg, two_rows))[0].tolist()) == {3}
    three_rows = [(1, 5), (1, 6), (2, 6), (3, 6), (3, 7)]
    cls, ids, _ = R.segment_cloud(cfg, R.image_cloud(cfg, three_rows))
    assert set(cls.tolist()) == {2} and set(ids.tolist()) == {64 + 5}


def test_two_records_in_one_cell():
    cfg = R.config(n_rows=1, n_columns=64, ground_last_row=0, small_min_points=2, small_min_rows=1)
    near, far, side = R.centre_record(cfg, 0, 10, 10.0), R.centre_record(cfg, 0, 10, 12.0), R.centre_record(cfg, 0, 11, 10.2)
    # the nearer one wins the cell: its neighbour at 10.2 m joins 10 m and would not join 12 m
    for recs, want in (([near, far, side], [2, 2, 2]), ([far, near, side], [2, 2, 2]), ([far, side], [3, 3])):
        cls, ids, _ = _seg(cfg, recs)
        assert cls.tolist() == want, recs
        assert ids.tolist() == ([10] * 3 if len(recs) == 3 else [10, 11])
    # equal floats of r: the lower index
    a = R.centre_record(cfg, 0, 10, 10.0)
    b = (a[0], a[1], f32(1e-6), 0)
    for recs in ([a, b], [b, a]):
        c = R.cloud_of(recs)
        keep, cell, r = R.project(cfg, c["x"], c["y"], c["z"], R.rows_of(c))
        assert r[0] != r[1] and f32(r[0]) == f32(r[1]) and keep.all()
        assert R.winners(cfg, keep, cell, r)[10] == 0


def test_scene_check():
    """The synthetic room, 16 x 900, ground rows 0 .. 7: most of what lies on the floor is ground, and little else is."""
    from lidar_feature_extraction_amd import make_scan
    cfg = R.config(n_rows=16, n_columns=900, ground_first_row=0, ground_last_row=7)
    for s in range(5):
        c = make_scan(16, 900, seed=700 + s)
        cls, _, counts = R.segment_cloud(cfg, c)
        in_range = cls != R.NONE
        floor = in_range & (c["z"] < -1.7)
        ground = cls == R.GROUND
        recall = (ground & floor).sum() / max(floor.sum(), 1)
        high = (ground & (c["z"] > -1.5)).sum() / max(ground.sum(), 1)
        print("seed %d: %.3f of the floor records are ground, %.2f %% of the ground records lie above -1.5 m, counts %s" %
              (700 + s, recall, 100.0 * high, counts.tolist()))
        assert floor.sum() > 1000 and recall >= 0.8 and high <= 0.05
        assert counts.sum() == len(c) and counts[R.SEGMENT] > 0
