"""The rolling voxel map's restatement (tests/rolling_map_restatement.py) pinned on cases written out by hand, and what of
lfx_rolling_map_* runs without a device: the default config, the constants, null arguments."""
import ctypes as C

import numpy as np

from lidar_feature_extraction_amd import RollingMap as DeviceRollingMap
from lidar_feature_extraction_amd import binding as LB
from tests.rolling_map_restatement import RollingMap, Store, compose, inverse, inverse_leaf, key, voxels

I = np.eye(4)[:3]


def rec(x, y=0.1, z=0.1, w=1.0):
    return [x, y, z, w]


def cloud(*rows):
    return np.array(rows, np.float32).reshape(-1, 4)


def test_voxel_floor_not_truncation():
    """leaf 0.5: inv = 2 exactly.  Negative coordinates go down, not towards zero; -0.0 is voxel 0; a point on a voxel's face
    belongs to the voxel above; |voxel| >= 2^20 and non-finite coordinates have no voxel."""
    inv = inverse_leaf(0.5)
    assert inv == np.float32(2.0)
    p = cloud(rec(-0.1), rec(-0.5), rec(-0.50001), rec(-0.0), rec(0.0), rec(0.5), rec(1.0), rec(0.49999997))
    v, ok = voxels(p, inv)
    assert ok.all()
    assert v[:, 0].tolist() == [-1, -1, -2, 0, 0, 1, 2, 0]
    assert v[:, 1].tolist() == [0] * 8
    bad = cloud(rec(np.nan), rec(np.inf), rec(-np.inf), rec(1e30), rec(524288.0), rec(-524288.5), rec(0.0, np.nan), rec(0.0, 0.0, 3e38))
    assert not voxels(bad, inv)[1].any()
    assert not voxels(cloud(rec(-524288.0)), inv)[1].any()        # floorf = -2^20 exactly: |.| >= 2^20
    edge = cloud(rec(524287.97), rec(-524287.5))
    v, ok = voxels(edge, inv)
    assert ok.all() and v[:, 0].tolist() == [2 ** 20 - 1, -(2 ** 20 - 1)]
    # a leaf whose inverse is not exact: 1.0f / 0.2f = 5.0 in float, and 0.6f * 5.0f = 3.0000002 -> voxel 3
    assert inverse_leaf(0.2) == np.float32(1.0) / np.float32(0.2)
    assert voxels(cloud(rec(0.6)), inverse_leaf(0.2))[0][0, 0] == int(np.floor(np.float32(0.6) * inverse_leaf(0.2)))


def test_key_and_slot():
    assert key((1, 2, 3)) == (1 << 63) | 1 | (2 << 21) | (3 << 42)
    assert key((-1, 0, 0)) == (1 << 63) | 0x1FFFFF
    assert key((0, -2, 0)) == (1 << 63) | (0x1FFFFE << 21)
    assert key((0, 0, 0)) == 1 << 63 and key((0, 0, 0)) != 0
    assert key((-2 ** 20, 2 ** 20 - 1, -1)) == (1 << 63) | 0x100000 | (0x0FFFFF << 21) | (0x1FFFFF << 42)
    s = Store(0.5, (5, 3, 2))
    assert s.o == (-2, -1, -1)                # -(N / 2), integer division
    assert s.slot((-2, -1, -1)) == (1 * 3 + 2) * 5 + 3 == 28      # the modulus of a negative is not negative
    assert s.slot((2, 1, 0)) == (0 * 3 + 1) * 5 + 2 == 7
    assert s.slot((-1, 0, 0)) == 4
    assert s.slot((3, 2, 1)) == s.slot((-2, -1, -1))              # one window further: the same slot
    assert s.inside((-2, -1, -1)) and s.inside((2, 1, 0)) and not s.inside((3, 0, 0)) and not s.inside((0, 0, 1))
    inside = [(x, y, z) for z in range(-1, 1) for y in range(-1, 2) for x in range(-2, 3)]
    assert sorted(s.slot(v) for v in inside) == list(range(30))   # injective inside the window


def test_insert_rule_and_counters():
    s = Store(0.5, (4, 4, 2))                 # x, y in [-1, 1), z in [-0.5, 0.5)
    a = cloud([0.1, 0.1, 0.1, 7.0], [0.2, 0.2, 0.2, 8.0], [-0.9, -0.9, -0.4, 9.0], [1.0, 0.0, 0.0, 1.0], [np.nan, 0, 0, 1.0])
    s.insert([a], [I])
    assert s.counts == dict(inserted=2, merged=1, outside=1, nonfinite=1)
    assert s.live((0, 0, 0)) and s.live((-2, -2, -1)) and not s.live((1, 0, 0))
    assert s.points[s.slot((0, 0, 0))].tolist() == a[0].tolist()              # the first one stays, 4th float and all
    s.insert([cloud([0.3, 0.3, 0.3, 5.0])], [I])
    assert s.counts == dict(inserted=2, merged=2, outside=1, nonfinite=1)
    assert s.points[s.slot((0, 0, 0))].tolist() == a[0].tolist()
    # rank is (cloud, index): the first cloud's record wins wherever the clouds lie in memory; the pose applies
    t = Store(0.5, (4, 4, 2))
    shift = I.copy()
    shift[0, 3] = 0.5
    t.insert([cloud([0.1, 0.1, 0.1, 1.0]), cloud([-0.3, 0.2, 0.2, 2.0], [0.2, 0.2, 0.2, 3.0])], [I, shift])
    assert t.points[t.slot((0, 0, 0))].tolist() == [np.float32(0.1)] * 3 + [1.0]
    assert t.points[t.slot((1, 0, 0))].tolist() == [np.float32(0.2) + np.float32(0.5), np.float32(0.2), np.float32(0.2), 3.0]
    assert t.counts == dict(inserted=2, merged=1, outside=0, nonfinite=0)


def centre(c):
    return [c * 0.5 + 0.25, 0.25, 0.25]


def test_recentring():
    """A window of 4 voxels along x (leaf 0.5), voxels -2 .. 1 filled; the window moved by 1, N - 1, N, past N and back."""
    s = Store(0.5, (4, 1, 1))
    assert s.o == (-2, 0, 0)
    pts = cloud(*[rec(0.5 * v + 0.1, w=float(v)) for v in (-2, -1, 0, 1)])
    s.insert([pts], [I])
    assert s.extract_all()[:, 3].tolist() == [-2.0, -1.0, 0.0, 1.0]
    s.recenter(centre(1))                     # by 1: voxel -2 leaves, voxel 2 enters on its slot and reads empty
    assert s.o == (-1, 0, 0) and s.slot((2, 0, 0)) == s.slot((-2, 0, 0))
    assert s.extract_all()[:, 3].tolist() == [-1.0, 0.0, 1.0]
    s.recenter(centre(3))                     # by N - 1
    assert s.o == (1, 0, 0) and s.extract_all()[:, 3].tolist() == [1.0]
    s.recenter(centre(4))                     # by N: every slot holds a voxel that has left
    assert s.o == (2, 0, 0) and len(s.extract_all()) == 0
    s.recenter(centre(9))                     # past N
    assert s.o == (7, 0, 0) and len(s.extract_all()) == 0
    s.recenter(centre(0))                     # back: nothing was written meanwhile, every voxel reappears
    assert s.extract_all()[:, 3].tolist() == [-2.0, -1.0, 0.0, 1.0]
    s.recenter(centre(4))
    s.insert([cloud(rec(0.5 * 2 + 0.1, w=20.0))], [I])            # voxel 2 takes the slot of voxel -2
    assert s.counts["inserted"] == 5 and s.extract_all()[:, 3].tolist() == [20.0]
    s.recenter(centre(0))                     # back: voxel -2 does not reappear, its slot was taken
    assert s.extract_all()[:, 3].tolist() == [-1.0, 0.0, 1.0]
    s.insert([pts], [I])                      # ... and is inserted again over the stale slot; the others merge
    assert s.counts == dict(inserted=6, merged=3, outside=0, nonfinite=0)
    assert s.extract_all()[:, 3].tolist() == [-2.0, -1.0, 0.0, 1.0]
    # both stores of a map move together, each by its own leaf
    m = RollingMap(0.5, 1.0, (4, 4, 2), (4, 4, 2))
    m.recenter([3.2, -3.2, 0.0])
    assert m.stores["edge"].o == (6 - 2, -7 - 2, 0 - 1) and m.stores["surface"].o == (3 - 2, -4 - 2, 0 - 1)


def test_extract_order_and_boxes():
    s = Store(0.5, (5, 3, 2))                 # x in [-1, 1.5), y in [-0.5, 1), z in [-0.5, 0.5)
    vox = [(1, 0, 0), (-2, -1, -1), (0, 1, -1), (2, 1, 0), (-1, 0, -1), (0, 0, 0)]
    pts = cloud(*[[0.5 * x + 0.2, 0.5 * y + 0.2, 0.5 * z + 0.2, float(i)] for i, (x, y, z) in enumerate(vox)])
    s.insert([pts], [I])
    order = sorted(range(len(vox)), key=lambda i: (vox[i][2], vox[i][1], vox[i][0]))
    assert order == [1, 4, 2, 5, 0, 3]
    assert s.extract_all()[:, 3].tolist() == [float(i) for i in order]
    assert s.extract([-100, -100, -100], [100, 100, 100])[:, 3].tolist() == [float(i) for i in order]      # clipped
    assert s.extract([0.0, 0.0, 0.0], [0.49, 0.49, 0.49])[:, 3].tolist() == [5.0]                        # one voxel
    assert s.extract([0.0, 0.0, 0.0], [0.5, 0.0, 0.0])[:, 3].tolist() == [5.0, 0.0]                      # hi's voxel is included
    assert len(s.extract([0.5, 0.0, 0.0], [0.0, 0.49, 0.49])) == 0                                        # hi < lo
    assert len(s.extract([5.0, 5.0, 5.0], [9.0, 9.0, 9.0])) == 0                                          # outside
    assert len(s.extract([0.0, 0.5, -0.5], [0.2, 0.7, -0.1])) == 1 and len(s.extract([0.5, 0.5, -0.5], [0.7, 0.7, -0.1])) == 0
    assert s.extract([-1e300, -1e300, -1e300], [1e300, 1e300, 1e300])[:, 3].tolist() == [float(i) for i in order]


def test_pose_composition_and_the_recentring_rule():
    """compose and inverse on poses whose sums can be done by hand; C = pose x odom^-1 gives pose back as C x odom; the
    windows follow a pose whose voxel is MORE than a quarter window off the centre voxel, on any axis of either store."""
    rz = np.array([[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 2.0], [0.0, 0.0, 1.0, 3.0]])       # a quarter turn about z, t = (1, 2, 3)
    shift = np.array([[1.0, 0.0, 0.0, 10.0], [0.0, 1.0, 0.0, 20.0], [0.0, 0.0, 1.0, 30.0]])
    assert compose(rz, shift).tolist() == [[0.0, -1.0, 0.0, -19.0], [1.0, 0.0, 0.0, 12.0], [0.0, 0.0, 1.0, 33.0]]
    assert compose(shift, rz).tolist() == [[0.0, -1.0, 0.0, 11.0], [1.0, 0.0, 0.0, 22.0], [0.0, 0.0, 1.0, 33.0]]
    assert (inverse(rz) + 0.0).tolist() == [[0.0, 1.0, 0.0, -2.0], [-1.0, 0.0, 0.0, 1.0], [0.0, 0.0, 1.0, -3.0]]
    assert (compose(rz, inverse(rz)) + 0.0).tolist() == np.eye(4)[:3].tolist()
    # (a0 b0 + a1 b1) + a2 b2, not a0 b0 + (a1 b1 + a2 b2): 1e16 + 1 is lost before -1e16 comes
    a = np.array([[1.0, 1.0, 1.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])
    b = np.array([[1e16, 0.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0], [-1e16, 0.0, 1.0, 0.0]])
    assert compose(a, b)[0, 0] == 0.0
    m = RollingMap(0.5, 1.0, (16, 16, 8), (8, 8, 4))      # centre voxels 0: quarters of 4, 4, 2 and 2, 2, 1 voxels
    assert not m.wants_recentre([0.0, 0.0, 0.0])
    assert not m.wants_recentre([2.4, -2.0, 1.2])          # edge voxels 4, -4, 2 and surface voxels 2, -2, 1: a quarter, not more
    assert m.wants_recentre([2.5, 0.0, 0.0])               # edge voxel 5
    assert m.wants_recentre([0.0, -2.01, 0.0])             # edge voxel -5, surface voxel -3
    assert m.wants_recentre([0.0, 0.0, 1.5])               # edge voxel 3
    loose = RollingMap(0.5, 1.0, (64, 64, 32), (8, 8, 4))
    assert loose.wants_recentre([3.0, 0.0, 0.0]) and not loose.wants_recentre([2.9, 0.0, 0.0])        # the surface store alone asks
    # the loop: a first scan is placed at the initial pose without an alignment; a failed alignment places nothing
    scan = (cloud(rec(0.1), rec(0.7)), cloud(rec(0.1), rec(1.2)))
    never = lambda *a: (_ for _ in ()).throw(AssertionError("aligned against an empty map"))      # noqa: E731
    r = loose.update(scan, never, odom=shift)
    assert (r["aligned"], r["inserted"], r["recentered"], r["code"]) == (False, True, True, 6) and r["pose"].tolist() == shift.tolist()
    assert loose.stores["surface"].o == (10 - 4, 20 - 4, 30 - 2) and loose.stores["edge"].counts["inserted"] == 2
    few = RollingMap(0.5, 1.0, (64, 64, 32), (8, 8, 4), n_neighbors=2)
    few.update(scan, never)
    moved = shift.copy()
    moved[:, 3] = [0.1, 0.0, 0.0]
    fail = lambda eb, sb, s, initial: dict(pose=rz, code=3, success=False)      # noqa: E731
    r = few.update(scan, fail, odom=moved)
    assert (r["aligned"], r["inserted"], r["code"]) == (True, False, 3) and few.pose.tolist() == moved.tolist()
    assert few.correction.tolist() == np.eye(4)[:3].tolist() and few.stores["edge"].counts["inserted"] == 2
    good = lambda eb, sb, s, initial: dict(pose=rz, code=0, success=True)       # noqa: E731
    r = few.update(scan, good, odom=moved)
    assert r["inserted"] and few.pose.tolist() == rz.tolist() and few.correction.tolist() == compose(rz, inverse(moved)).tolist()
    assert compose(few.correction, moved).tolist() == rz.tolist()


def test_library_side_without_a_device():
    """The default config, the constants and the refusals that come before any device work."""
    L = LB.load()
    cfg = LB.RollingMapConfig()
    L.lfx_rolling_map_default_config(C.byref(cfg))
    assert (cfg.edge_leaf, cfg.surface_leaf) == (np.float32(0.2), np.float32(0.4))
    assert tuple(cfg.edge_dims) == (512, 512, 128) and tuple(cfg.surface_dims) == (256, 256, 64)
    # 32 bytes a slot: 1.2 GB at the defaults
    assert 32 * (512 * 512 * 128 + 256 * 256 * 64) == 1207959552
    assert (LB.ROLLING_EDGE, LB.ROLLING_SURFACE) == (0, 1) and DeviceRollingMap.KINDS == dict(edge=0, surface=1)
    null = C.c_void_p(0)
    out, n = C.c_void_p(), C.c_uint64()
    assert L.lfx_rolling_map_create(null, C.byref(cfg), C.byref(out)) == LB.ERR_INVALID_ARGUMENT
    assert L.lfx_rolling_map_recenter(null, None) == LB.ERR_INVALID_ARGUMENT
    assert L.lfx_rolling_map_insert(null, null, 0, null, null, null, 1, 1, 0, None, null) == LB.ERR_INVALID_ARGUMENT
    assert L.lfx_rolling_map_insert_host(null, null, 0, null, 0, None, null) == LB.ERR_INVALID_ARGUMENT
    assert L.lfx_rolling_map_extract(null, null, 0, None, None, null, 0, C.byref(n), null) == LB.ERR_INVALID_ARGUMENT
    assert L.lfx_rolling_map_view(null, null, None, null) == LB.ERR_INVALID_ARGUMENT
    assert L.lfx_rolling_map_save(null, null, b"/nowhere", None, null) == LB.ERR_INVALID_ARGUMENT
    L.lfx_rolling_map_destroy(null)           # a no-op
