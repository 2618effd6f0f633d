"""The place recognition section of include/lfx.h without a device: the numpy restatement (tests/scan_context_restatement.py)
on a cloud written out by hand, its sectors against the atan2 formula, the host-only functions' argument checks, the
distance restatement's fixed points, and the condition the GPU tests rely on -- the 24 revisits of the prototype name
their keyframes with the yaw within one sector."""
import ctypes as C

import numpy as np
import pytest

from lidar_feature_extraction_amd import binding as B
from tests import scan_context_restatement as R


def test_a_cloud_written_out_by_hand():
    """2 rings x 4 sectors out to 10 m (ring_r2 = 0, 25, 100; sectors from -pi in quarter turns), sensor_height 2."""
    cfg = R.config(n_rings=2, n_sectors=4, max_radius=10.0, min_radius=0.1, sensor_height=2.0)
    cs, sn, r2 = R.scan_context_tables(cfg)
    assert r2.tolist() == [0.0, 25.0, 100.0]
    assert cs[0] == -1.0 and cs[2] == 1.0 and abs(sn[2]) < 1e-15 and abs(cs[1]) < 1e-15 and sn[1] == -1.0 and sn[3] == 1.0
    nan = float("nan")
    pts = np.array([
        (1.0, 1.0, 0.5),        # ring 0, sector 2: 2.5
        (-1.0, 1.0, -1.0),      # ring 0, sector 3: 1.0
        (-1.0, -1.0, -3.0),     # ring 0, sector 0: below the ground, 0
        (6.0, -1.0, 1.0),       # ring 1, sector 1: 3.0
        (6.0, -2.0, 0.25),      # the same cell, lower
        (0.0, 7.0, 0.0),        # ring 1, on the +y axis: sector 3, 2.0
        (3.0, 4.0, 1.5),        # r2 = 25 = ring_r2[1]: ring 1, sector 2, 3.5
        (20.0, 0.0, 5.0),       # out of range
        (8.0, 6.0, 9.0),        # r2 = 100 = ring_r2[R]: out of range
        (0.0, 0.0, 0.0),        # under min_radius
        (nan, 1.0, 1.0), (1.0, 1.0, nan),
    ], np.float32)
    got = R.descriptor(cfg, pts[:, 0], pts[:, 1], pts[:, 2])
    want = np.array([[0.0, 0.0, 2.5, 1.0], [0.0, 3.0, 3.5, 2.0]], np.float32)
    assert got.tobytes() == want.tobytes(), got


def test_sectors_agree_with_atan2_on_synthetic_scans():
    """0 differences expected, as in the prototype (the counts are the definition; atan2 is the check).  The sector counts
    are ones whose boundaries fall between the 900 columns of the scans, not on them (S = 120 puts every other boundary on a
    ray, where the rounding of a coordinate decides)."""
    from lidar_feature_extraction_amd import make_scan
    for cfg in (R.config(), R.config(n_rings=16, max_radius=16.0), R.config(n_sectors=100), R.config(n_sectors=50)):
        n = 0
        for seed in (100, 101, 902, 903, 915):
            c = make_scan(R.RINGS, R.COLS, seed=seed, sensor_pose=(0.3 * (seed % 7), -0.2 * (seed % 5), 0.01 * seed))
            keep, _ring, sector = R.cells(cfg, c["x"], c["y"])
            assert keep.sum() > 0.8 * len(c)
            differ = int((sector[keep] != R.atan2_sectors(cfg, c["x"], c["y"])[keep]).sum())
            assert differ == 0, (seed, differ)
            n += int(keep.sum())
        assert n > 50000


def test_host_only_functions_check_their_arguments():
    L = B.load()
    cfg = B.ScanContextConfig()
    L.lfx_scan_context_default_config(C.byref(cfg))
    assert (cfg.n_rings, cfg.n_sectors, cfg.max_radius, cfg.sensor_height) == (20, 60, 80.0, 2.0) and cfg.min_radius == np.float32(0.1)
    L.lfx_scan_context_default_config(None)            # a no-op
    pd = C.POINTER(C.c_double)
    guard = 123.25
    cs, sn, r2 = np.full(121, guard), np.full(121, guard), np.full(42, guard)
    p = lambda a: a.ctypes.data_as(pd)                 # noqa: E731
    assert L.lfx_scan_context_tables(C.byref(cfg), p(cs), p(sn), p(r2)) == 0
    assert cs[60] == guard and sn[60] == guard and r2[21] == guard and r2[20] == 6400.0 and r2[0] == 0.0
    assert L.lfx_scan_context_tables(None, p(cs), p(sn), p(r2)) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_scan_context_tables(C.byref(cfg), None, p(sn), p(r2)) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_scan_context_tables(C.byref(cfg), p(cs), None, p(r2)) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_scan_context_tables(C.byref(cfg), p(cs), p(sn), None) == B.ERR_INVALID_ARGUMENT
    bad = [dict(n_rings=0), dict(n_rings=41), dict(n_sectors=2), dict(n_sectors=61), dict(n_sectors=122), dict(n_sectors=3),
           dict(max_radius=float("inf")), dict(max_radius=float("nan")), dict(min_radius=float("nan")), dict(min_radius=-0.5),
           dict(min_radius=80.0), dict(min_radius=90.0), dict(max_radius=0.0, min_radius=0.0), dict(sensor_height=float("inf"))]
    for fields in bad:
        cs[:], sn[:], r2[:] = guard, guard, guard
        assert L.lfx_scan_context_tables(C.byref(R.config(**fields)), p(cs), p(sn), p(r2)) == B.ERR_INVALID_ARGUMENT, fields
        assert (cs == guard).all() and (sn == guard).all() and (r2 == guard).all(), fields
    for fields in (dict(n_rings=1, n_sectors=4), dict(n_rings=40, n_sectors=120), dict(min_radius=0.0)):
        assert L.lfx_scan_context_tables(C.byref(R.config(**fields)), p(cs), p(sn), p(r2)) == 0, fields
    # the index's host-only calls
    n = C.c_uint32(7)
    assert L.lfx_place_db_size(None, C.byref(n)) == B.ERR_INVALID_ARGUMENT
    L.lfx_place_db_destroy(None)                       # a no-op
    null = C.c_void_p(0)
    assert L.lfx_scan_context_batch(null, C.byref(cfg), 1, null, null) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_place_db_create(null, C.byref(cfg), 4, None) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_place_db_add(null, null, null, 1, null) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_place_db_add_host(null, null, null, 1, null) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_place_db_download(null, null, 0, 1, null, null) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_place_db_query(null, null, null, 1, 0, 1, 1, None, null) == B.ERR_INVALID_ARGUMENT


def test_distance_restatement_fixed_points():
    """d(0) of a descriptor with itself is 0 where every column is occupied; rolled by s columns it gives shift s and
    distance 0 (to the rounding of S quotients near 1: 1e-15); empty columns do not count; nothing valid gives 1."""
    rng = np.random.default_rng(3)
    d = rng.uniform(0.1, 5.0, (20, 60)).astype(np.float32)
    assert abs(R.shift_distances(d, d[None])[0, 0]) < 1e-15
    for s in (1, 7, 30, 31, 59):
        # the sensor turned by +s sectors: what was in column j + s is seen in column j
        q = np.roll(d, -s, axis=1)
        (entry, shift, dist, yaw), = R.query(q, d[None], 1)
        assert (entry, shift) == (0, s) and abs(dist) < 1e-15
        assert yaw == pytest.approx(np.deg2rad(6.0 * s if s <= 30 else 6.0 * (s - 60)), abs=1e-12)
    holes = d.copy()
    holes[:, 5:9] = 0.0
    assert abs(R.shift_distances(holes, holes[None])[0, 0]) < 1e-15
    zero = np.zeros_like(d)
    assert (R.shift_distances(zero, d[None]) == 1.0).all() and (R.shift_distances(d, zero[None]) == 1.0).all()
    # duplicates: the lower entry first; fewer entries than k: the rest are empty
    other = rng.uniform(0.1, 5.0, (20, 60)).astype(np.float32)
    got = R.query(d, np.stack([other, d, d]), 4)
    assert [g[0] for g in got] == [1, 2, 0, None] and got[0][2] == got[1][2] < got[2][2] < got[3][2] == float("inf")
    assert R.query(d, np.stack([other, d, d]), 2, first=2, count=0) == [(None, 0, float("inf"), 0.0)] * 2


@pytest.mark.parametrize("fields", [dict(), dict(n_rings=16, max_radius=16.0)], ids=["R20-80m", "R16-16m"])
def test_the_prototype_revisits_name_their_keyframes(fields):
    """The six keyframes and 24 revisits of the prototype: every revisit's best entry is its keyframe, with
    |yaw - truth| <= 2 pi / S.  The GPU tests rely on this (the device's descriptors are these bits)."""
    cfg = R.config(**fields)
    keys = np.stack([R.descriptor_of_cloud(cfg, c) for c in R.keyframes()])
    worst_hit, best_other = 0.0, np.inf
    for cloud, place, yaw in R.revisits():
        (e0, _s0, d0, y0), (_e1, _s1, d1, _y1) = R.query(R.descriptor_of_cloud(cfg, cloud), keys, 2)
        assert e0 == place, (place, yaw, e0, d0, d1)
        assert R.yaw_error(y0, yaw) <= 2.0 * np.pi / cfg.n_sectors, (place, yaw, y0)
        worst_hit, best_other = max(worst_hit, d0), min(best_other, d1)
    print("revisits %s: distance of the keyframe <= %.3f, of the runner-up >= %.3f" % (fields, worst_hit, best_other))
    assert worst_hit < best_other
