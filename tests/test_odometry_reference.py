"""(CPU) The reference's own odometry vectors, as data (tests/golden/odometry_vectors.json): RecentScans
(test_recent_scans.cpp:36-111), Odometry with the stub updater (test_odometry.cpp:90-115) and TransformPointCloud
(test_pcl_utils.cpp:51-74) pin the test-side restatement in tests/odometry_restatement.py, which tests/test_odometry_gpu.py
holds the device to.  Also: the moving-sensor sequences of synth.py, the C++ caller's build and the ABI's defaults."""
import ctypes as C
import json
import os

import numpy as np

from tests.odometry_restatement import EdgeSurfaceMap, Odometry, RecentScans, transform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = json.load(open(os.path.join(ROOT, "tests", "golden", "odometry_vectors.json")))


def _pose(rotation, translation):
    return np.hstack([np.asarray(rotation, np.float64), np.asarray(translation, np.float64).reshape(3, 1)])


def _records(points):
    p = np.asarray(points, np.float32).reshape(-1, 3)
    return np.hstack([p, np.ones((len(p), 1), np.float32)])


def test_recent_scans_vectors():
    v = VECTORS["recent_scans"]
    scans = RecentScans()
    assert scans.is_empty()
    for s in v["scans"]:
        scans.add(_pose(s["rotation"], s["translation"]), _records(s["points"]))
    assert not scans.is_empty()
    assert np.array_equal(scans.get_all()[:, :3], np.asarray(v["get_all"], np.float32))
    for n, want in v["get_recent"].items():
        got = scans.get_recent(int(n))
        assert len(got) == len(want) and np.array_equal(got[:, :3], np.asarray(want, np.float32)), n


def test_odometry_with_the_stub_updater():
    v = VECTORS["odometry"]
    step = np.asarray(v["updater_step"], np.float64)

    class Map:                                # test_odometry.cpp's Map: points pushed as pose * point
        def __init__(self):
            self.points = []

        def is_empty(self):
            return not self.points

        def add(self, pose, point):
            self.points.append(pose[:, :3] @ point + pose[:, 3])

        def get_recent(self):
            return list(self.points)

    def updater(_recent):                     # PoseUpdater: dpose (identity, step) * pose
        def run(_scan, pose):
            out = pose.copy()
            out[:, 3] = pose[:, 3] + step
            return out
        return run
    m = Map()
    odo = Odometry(updater, m)
    for scan, t, size in zip(v["scans"], v["translations_after_update"], v["map_sizes_after_update"]):
        odo.update(np.asarray(scan, np.float64))
        assert np.linalg.norm(odo.pose[:, 3] - np.asarray(t, np.float64)) == 0.0
        assert len(m.points) == size
    assert np.array_equal(np.stack(m.get_recent()), np.asarray(v["merged"], np.float64))


def test_transform_point_cloud():
    v = VECTORS["transform_point_cloud"]
    w, x, y, z = np.asarray(v["quaternion_wxyz"], np.float64) / np.linalg.norm(v["quaternion_wxyz"])
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    t = np.asarray(v["translation"], np.float64)
    cloud = _records(v["points"])
    got = transform(_pose(R, t), cloud)
    for p, g in zip(cloud, got):
        assert np.linalg.norm(R @ p[:3].astype(np.float64) + t - g[:3].astype(np.float64)) <= v["tolerance"]
    assert np.array_equal(got[:, 3], cloud[:, 3])          # the other fields are copied


def test_edge_surface_map_windows_both_clouds():
    m = EdgeSurfaceMap(2)
    assert m.is_empty()
    ident = np.eye(4)[:3]
    for k in range(3):
        m.add(ident, (_records([[k, 0, 0]]), _records([[0, k, 0], [0, k, 1]])))
    e, s = m.get_recent()
    assert e[:, 0].tolist() == [1, 2] and s[:, 1].tolist() == [1, 1, 2, 2]


def test_moving_sensor_sequences():
    from lidar_feature_extraction_amd import make_scan, make_sequence
    # the keyword's default, and a sensor that does not move, give the bytes the scan always had
    assert make_scan(16, 900, seed=5).tobytes() == make_scan(16, 900, seed=5, sensor_pose=None).tobytes()
    assert make_scan(16, 900, seed=5).tobytes() == make_scan(16, 900, seed=5, sensor_pose=(0.0, 0.0, 0.0)).tobytes()
    clouds, poses = make_sequence(3, 16, 900, seed=7, step=0.05, yaw_step_deg=0.5)
    assert len(clouds) == 3 and poses.shape == (3, 3, 4)
    assert np.array_equal(poses[0], np.eye(4)[:3])
    assert np.allclose(poses[2][:, 3], [0.1, 0.0, 0.0]) and np.isclose(np.arctan2(poses[2][1, 0], poses[2][0, 0]), np.deg2rad(1.0))
    # a wall seen from two places: the far wall (x = 10 m in the room) moves 5 cm closer per scan in the sensor's frame
    a, b = make_scan(16, 900, seed=9, sensor_pose=(0.0, 0.0, 0.0), sigma=0.0, n_pillars=0, spikes=False, out_of_range=False), \
        make_scan(16, 900, seed=9, sensor_pose=(0.05, 0.0, 0.0), sigma=0.0, n_pillars=0, spikes=False, out_of_range=False)
    assert abs(float(a["x"].max()) - float(b["x"].max()) - 0.05) < 1e-4


def test_odometry_example_builds_without_a_gpu():
    exe = os.path.join(ROOT, "lidar_feature_extraction_amd", "_lib", "odometry_scans")
    if not os.path.exists(exe):
        import __graft_entry__
        __graft_entry__.build()
    assert os.access(exe, os.X_OK)


def test_default_config_and_refusals_without_a_device():
    """lfx_odometry_default_config gives the reference's settings; the entry points refuse null arguments."""
    from lidar_feature_extraction_amd import binding as LB
    lib = LB.load()
    cfg = LB.OdometryConfig()
    lib.lfx_odometry_default_config(C.byref(cfg))
    assert (cfg.n_local_scans, cfg.n_neighbors, cfg.max_iter, cfg.surface_leaf) == (7, 15, 20, 1.0)
    assert list(cfg.initial_pose) == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    null = C.c_void_p(0)
    assert lib.lfx_odometry_create(null, C.byref(cfg), C.byref(C.c_void_p())) == -1
    assert lib.lfx_odometry_update_batch(null, null, 1, None, null) == -1
    assert lib.lfx_odometry_update(null, null, null, 0, null, 0, None, null) == -1
    assert lib.lfx_odometry_update_host(null, null, null, 0, null, 0, None, null) == -1
    assert lib.lfx_odometry_add(null, null, None, null, 0, null, 0, null) == -1
    assert lib.lfx_odometry_pose(null, None) == -1
    assert lib.lfx_odometry_view(null, None) == -1
    lib.lfx_align_message.restype = C.c_char_p
    assert lib.lfx_align_message(6) == b"The scan was not aligned"
