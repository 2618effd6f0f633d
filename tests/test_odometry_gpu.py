"""lfx_odometry_* (the odometry row): Odometry::Update over EdgeSurfaceMap with the store and the window maps on
the device.  The store is held to the test-side restatement (tests/odometry_restatement.py, pinned by the reference's own
vectors in tests/test_odometry_reference.py) bit for bit; every alignment to the oracle's Optimizer::Run under the tolerance
rule of tests/test_align_gpu.py::test_localize_batch_against_the_oracle (parity unpinned: Eigen / nanoflann / PCL arithmetic)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests.odometry_restatement import RecentScans, downsample, optimize_scan, oracle_chain, trajectory_error, transform

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = json.load(open(os.path.join(ROOT, "tests", "golden", "odometry_vectors.json")))
K, MAX_ITER = 15, 20


def _dev():
    import torch
    return torch.device("cuda", 0)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1, 4).copy()).to(_dev())


def _d2h(ptr, n):
    """n records of 4 floats from device address ptr."""
    import torch
    out = np.zeros((int(n), 4), np.float32)
    if n:
        torch.cuda.synchronize()
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(out.ctypes.data, int(ptr), out.nbytes, 2) == 0
    return out


def _rotation(axis_angle):
    th = np.asarray(axis_angle, np.float64)
    k = np.linalg.norm(th)
    if k == 0:
        return np.eye(3)
    u = th / k
    Kx = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + np.sin(k) * Kx + (1 - np.cos(k)) * Kx @ Kx


def _pose(axis_angle, t):
    return np.ascontiguousarray(np.hstack([_rotation(axis_angle), np.asarray(t, np.float64).reshape(3, 1)]))


def _records(points):
    p = np.asarray(points, np.float32).reshape(-1, 3)
    return np.hstack([p, np.ones((len(p), 1), np.float32)])


def _fx(rings, cols, batch):
    from lidar_feature_extraction_amd import FeatureExtraction
    return FeatureExtraction(device=0, max_points_per_scan=rings * cols, max_batch=batch, max_points_per_ring=cols, max_rings=rings)


def _extract(fx, clouds):
    """clouds through the device path; returns the device buffer (kept alive by the caller) and the host copies of the
    scans' clouds (lfx_download_scan: the bits the device holds)."""
    from lidar_feature_extraction_amd import concat
    import torch
    d = torch.from_numpy(concat(clouds).view(np.uint8).copy()).to(_dev())
    fx.extract_batch_device(d.data_ptr(), [len(c) for c in clouds], _stream())
    return d, [fx.download(s, _stream()) for s in range(len(clouds))]


def _same_bits(a, b):
    return a["pose"].tobytes() == b["pose"].tobytes() and (a["code"], a["iteration"], a["aligned"]) == (b["code"], b["iteration"], b["aligned"]) \
        and (np.isnan(a["error"]) and np.isnan(b["error"]) or a["error"] == b["error"])


def _store(odo):
    v = odo.view()
    return v, _d2h(v["edge_points"], v["n_edge"]), _d2h(v["surface_points"], v["n_surface"])


@pytest.mark.parametrize("n_local", [2, 4])
def test_reference_vectors_through_the_device(n_local):
    """test_recent_scans.cpp:36-111 through lfx_odometry_add + lfx_odometry_view: GetAll and GetRecent(n), exactly."""
    v = VECTORS["recent_scans"]
    fx = _fx(16, 64, 1)
    odo = fx.odometry(n_local_scans=n_local, edge_capacity_points=64, surface_capacity_points=64)
    keep = []
    for s in v["scans"]:
        d = _up(_records(s["points"]))
        keep.append(d)
        odo.add(np.hstack([np.asarray(s["rotation"], np.float64), np.asarray(s["translation"], np.float64).reshape(3, 1)]),
                d.data_ptr(), 1, d.data_ptr(), 1, _stream())
    view, edge, surface = _store(odo)
    want_all = np.asarray(v["get_all"], np.float32)
    assert np.array_equal(edge[:, :3], want_all) and np.array_equal(surface[:, :3], want_all)
    recent = np.asarray(v["get_recent"][str(n_local)], np.float32)
    assert view["n_window_scans"] == len(recent) and view["n_edge_window"] == len(recent) == view["n_surface_window"]
    assert np.array_equal(_d2h(view["edge_window"], view["n_edge_window"])[:, :3], recent)
    assert np.array_equal(_d2h(view["surface_window"], view["n_surface_window"])[:, :3], recent)
    assert view["edge_offsets"].tolist() == [0, 1, 2, 3] and (view["n_scans"], view["n_added"], view["dropped_scans"]) == (3, 3, 0)
    assert np.array_equal(odo.pose(), np.eye(4)[:3])          # Add leaves the pose alone
    odo.close()
    fx.close()


def test_transform_bits():
    """RecentScans::Add's transform on the device equals the restatement bit for bit: random poses (large angles, far
    translations), clouds of random sizes (empty ones, one point, around a workgroup's 256, several thousand), the 4th
    float of every record copied."""
    rng = np.random.default_rng(3)
    fx = _fx(16, 64, 1)
    odo = fx.odometry(n_local_scans=3, edge_capacity_points=1 << 18, surface_capacity_points=1 << 18)
    sizes = [0, 1, 7, 255, 256, 257, 5000, 20011]
    want_e, want_s, keep = [], [], []
    for i in range(12):
        ne, ns = int(rng.choice(sizes)), int(rng.choice(sizes))
        if i == 3:
            ne, ns = 0, 0
        pose = _pose(rng.normal(0, 1.5, 3), rng.normal(0, 60, 3))
        e = rng.normal(0, 40, (ne, 4)).astype(np.float32)
        s = rng.normal(0, 40, (ns, 4)).astype(np.float32)
        de, ds = _up(e) if ne else None, _up(s) if ns else None
        keep += [de, ds]
        odo.add(pose, de.data_ptr() if ne else 0, ne, ds.data_ptr() if ns else 0, ns, _stream())
        want_e.append(transform(pose, e))
        want_s.append(transform(pose, s))
    view, edge, surface = _store(odo)
    assert edge.tobytes() == np.concatenate(want_e).tobytes()
    assert surface.tobytes() == np.concatenate(want_s).tobytes()
    assert view["edge_offsets"].tolist() == np.concatenate([[0], np.cumsum([len(a) for a in want_e])]).tolist()
    assert view["surface_offsets"].tolist() == np.concatenate([[0], np.cumsum([len(a) for a in want_s])]).tolist()
    odo.close()
    fx.close()


def test_first_scan_small_windows_and_empty_clouds():
    """The first update does not align and keeps the initial pose; a window map under n_neighbors points gives aligned = 0
    with the pose carried over (the scan is still added); a scan with empty clouds is aligned as lfx_localize_* handles it
    (LFX_ALIGN_EMPTY_INPUT, the initial pose handed back) and added."""
    from lidar_feature_extraction_amd import make_sequence
    rings, cols = 32, 1024
    clouds, _ = make_sequence(2, rings, cols, seed=8300)
    fx = _fx(rings, cols, 1)
    P0 = _pose([0.01, -0.02, 0.3], [1.5, -2.0, 0.25])
    odo = fx.odometry(initial_pose=P0)
    d, got = _extract(fx, clouds[:1])
    r = odo.update_batch(1, _stream())[0]
    assert (r["aligned"], r["code"], r["iteration"], r["n_edge_map"], r["n_surface_map"]) == (False, 6, 0, 0, 0), r
    assert r["message"] == "The scan was not aligned" and not r["success"]
    assert r["pose"].tobytes() == P0.tobytes() and odo.pose().tobytes() == P0.tobytes()
    view, edge, surface = _store(odo)
    assert (view["n_scans"], view["n_added"]) == (1, 1)
    assert edge.tobytes() == transform(P0, got[0].edge_points).tobytes()
    assert surface.tobytes() == transform(P0, got[0].surface_points).tobytes()
    # a scan of empty clouds against a full window: EmptyInput, pose unchanged, added
    r = odo.update(0, 0, 0, 0, _stream())
    assert (r["aligned"], r["code"], r["iteration"]) == (True, 4, 0), r
    assert r["n_edge_map"] == len(got[0].edge_points) and r["n_surface_map"] == len(got[0].surface_points)
    # the pose is result.pose whatever the code: Optimizer::Run hands the initial pose back through its quaternion (to rounding)
    assert odo.pose().tobytes() == r["pose"].tobytes() and np.abs(r["pose"] - P0).max() < 1e-15
    assert odo.view()["n_scans"] == 2
    odo.close()
    # a window of 5 points: not aligned, pose carried over, the scan added
    odo = fx.odometry()
    tiny = _up(np.random.default_rng(5).normal(0, 3, (5, 4)))
    odo.add(np.eye(4)[:3], tiny.data_ptr(), 5, tiny.data_ptr(), 5, _stream())
    d, got = _extract(fx, clouds[1:2])
    r = odo.update_batch(1, _stream())[0]
    assert (r["aligned"], r["code"], r["iteration"], r["n_edge_map"], r["n_surface_map"]) == (False, 6, 0, 5, 5), r
    assert np.array_equal(odo.pose(), np.eye(4)[:3])
    view = odo.view()
    assert (view["n_scans"], view["n_edge"]) == (2, 5 + len(got[0].edge_points))
    odo.close()
    fx.close()


def _sequence_run(rings, cols, n, seed):
    from lidar_feature_extraction_amd import make_sequence
    clouds, truth = make_sequence(n, rings, cols, seed=seed)
    fx = _fx(rings, cols, n)
    odo = fx.odometry()
    d, got = _extract(fx, clouds)
    res = odo.update_batch(n, _stream())
    view, edge, surface = _store(odo)
    odo.close()
    fx.close()
    return clouds, truth, got, res, view, edge, surface


def test_step_parity_against_the_oracle():
    """12 scans of a moving 32 x 1024 sensor through one update_batch.  The device's store equals the restatement built from
    the device's own poses, bit for bit (so every window it aligned against did); at every step the oracle's Optimizer::Run
    on that window, the scan's downsampled surface and the device's previous pose agrees with the device's alignment."""
    from oracle import binding as OB
    rings, cols, n = 32, 1024, 12
    clouds, truth, got, res, view, edge, surface = _sequence_run(rings, cols, n, 8100)
    want = [OB.extract(c, canonical_ties=False) for c in clouds]
    for s in range(n):
        assert np.array_equal(got[s].edge_points[:, :3], want[s]["edge_points"][:, :3])
        assert np.array_equal(got[s].surface_points[:, :3], want[s]["surface_points"][:, :3])
    es, ss = RecentScans(), RecentScans()
    for s in range(n):
        es.add(res[s]["pose"], got[s].edge_points)
        ss.add(res[s]["pose"], got[s].surface_points)
    assert edge.tobytes() == es.get_all().tobytes() and surface.tobytes() == ss.get_all().tobytes()
    assert (view["n_scans"], view["n_window_scans"], view["dropped_scans"]) == (n, 7, 0)
    assert not res[0]["aligned"] and res[0]["pose"].tobytes() == np.eye(4)[:3].tobytes()
    for k in range(1, n):
        lo = max(0, k - 7)
        ew, sw = np.concatenate(es.scans[lo:k]), np.concatenate(ss.scans[lo:k])
        g = res[k]
        assert g["aligned"] and (g["n_edge_map"], g["n_surface_map"]) == (len(ew), len(sw)), (k, g)
        w = optimize_scan(ew, sw, K, want[k]["edge_points"], downsample(want[k]["surface_points"], 1.0), res[k - 1]["pose"], MAX_ITER)
        if (g["code"], g["iteration"]) != (w["code"], w["iteration"]):
            assert abs(g["iteration"] - w["iteration"]) <= 1, (k, g, w)
            assert np.abs(g["pose"] - w["pose"]).max() < 2e-3, (k, g, w)
        else:
            assert np.abs(g["pose"] - w["pose"]).max() <= 1e-6 * (1 + np.abs(w["pose"]).max()), (k, g["pose"], w["pose"])
            assert abs(g["error"] - w["error"]) <= 1e-5 * abs(w["error"]) + 1e-18, (k, g["error"], w["error"])
            assert abs(g["error_scale"] - w["error_scale"]) <= 1e-5 * abs(w["error_scale"]) + 1e-18, k
        assert g["success"] == w["success"], (k, g, w)


def test_trajectory_against_the_ground_truth():
    """The device's trajectory and the whole oracle chain's (extract -> Downsample -> Optimizer::Run against the window,
    on the CPU) both stay near the synthetic ground truth (5 cm and 0.5 degrees per scan).  The oracle chain's worst error
    on this sequence, measured: 0.0332 m and 0.00668 rad (z drifts most); the bound is about twice that."""
    rings, cols, n = 32, 1024, 12
    clouds, truth, got, res, view, edge, surface = _sequence_run(rings, cols, n, 8100)
    bound_t, bound_r = 0.06, 0.015
    dt, dr = trajectory_error([r["pose"] for r in res], truth)
    assert dt < bound_t and dr < bound_r, (dt, dr)
    ot, orr = trajectory_error(oracle_chain(clouds), truth)
    assert ot < bound_t and orr < bound_r, (ot, orr)


def test_batch_independence_entry_points_and_grids():
    """A scan's arithmetic does not depend on its neighbours: the sequence in batches of 4, scan by scan, through
    lfx_odometry_update on caller clouds and through lfx_odometry_update_host gives the same pose bits, iterations and
    codes; window maps without a grid (cell 0) give the same bits as the grids."""
    from lidar_feature_extraction_amd import make_sequence
    rings, cols, n = 32, 1024, 8
    clouds, _ = make_sequence(n, rings, cols, seed=8200)

    def by_batches(size, cell=1.0):
        fx = _fx(rings, cols, size)
        odo = fx.odometry(edge_cell=cell, surface_cell=cell)
        out = []
        for a in range(0, n, size):
            d, _ = _extract(fx, clouds[a:a + size])
            out += odo.update_batch(len(clouds[a:a + size]), _stream())
        odo.close()
        fx.close()
        return out

    four, one, no_grid = by_batches(4), by_batches(1), by_batches(4, cell=0.0)
    fx = _fx(rings, cols, n)
    d, got = _extract(fx, clouds)
    odo, odo_host = fx.odometry(), fx.odometry()
    caller, host = [], []
    for s in range(n):
        de, ds = _up(got[s].edge_points), _up(got[s].surface_points)
        caller.append(odo.update(de.data_ptr(), len(got[s].edge_points), ds.data_ptr(), len(got[s].surface_points), _stream()))
        host.append(odo_host.update_host(got[s].edge_points, got[s].surface_points, _stream()))
    for s in range(n):
        for name, other in (("batch 1", one), ("caller clouds", caller), ("host clouds", host), ("no grid", no_grid)):
            assert _same_bits(four[s], other[s]), (s, name, four[s], other[s])
    assert sum(r["aligned"] for r in four) == n - 1
    odo.close()
    odo_host.close()
    fx.close()


def test_capacity_drops_old_scans_and_refuses_what_cannot_fit():
    """A store too small for everything discards the scans older than the window (one move of the window to the front) and
    keeps the window intact: the same poses as an unbounded store, view reports the drops.  A scan larger than the store
    fails with pose and store unchanged."""
    from lidar_feature_extraction_amd import make_sequence
    from lidar_feature_extraction_amd.binding import LfxError
    rings, cols, n, w = 16, 900, 7, 2
    clouds, _ = make_sequence(n, rings, cols, seed=8400)
    fx = _fx(rings, cols, n)
    d, got = _extract(fx, clouds)
    big = fx.odometry(n_local_scans=w)
    ref = big.update_batch(n, _stream())
    big.close()
    ne, ns = max(len(g.edge_points) for g in got), max(len(g.surface_points) for g in got)
    odo = fx.odometry(n_local_scans=w, edge_capacity_points=3 * ne, surface_capacity_points=3 * ns)
    keep, es, ss = [], RecentScans(), RecentScans()
    for s in range(n):
        de, ds = _up(got[s].edge_points), _up(got[s].surface_points)
        keep += [de, ds]
        r = odo.update(de.data_ptr(), len(got[s].edge_points), ds.data_ptr(), len(got[s].surface_points), _stream())
        assert _same_bits(r, ref[s]), (s, r, ref[s])
        es.add(r["pose"], got[s].edge_points)
        ss.add(r["pose"], got[s].surface_points)
        view, edge, surface = _store(odo)
        m = view["n_scans"]
        assert view["n_added"] == s + 1 and m + view["dropped_scans"] == s + 1 and m >= min(w, s + 1)
        assert edge.tobytes() == np.concatenate(es.scans[s + 1 - m:]).tobytes()
        assert surface.tobytes() == np.concatenate(ss.scans[s + 1 - m:]).tobytes()
        assert _d2h(view["edge_window"], view["n_edge_window"]).tobytes() == es.get_recent(w).tobytes()
        assert _d2h(view["surface_window"], view["n_surface_window"]).tobytes() == ss.get_recent(w).tobytes()
    assert view["dropped_scans"] > 0 and view["compactions"] > 0
    # too large even beside the window alone
    pose_before, (v0, e0, s0) = odo.pose(), _store(odo)
    huge = _up(np.random.default_rng(9).normal(0, 5, (3 * ne + 1, 4)))
    with pytest.raises(LfxError, match="does not fit"):
        odo.update(huge.data_ptr(), 3 * ne + 1, huge.data_ptr(), 10, _stream())
    with pytest.raises(LfxError, match="does not fit"):
        odo.add(np.eye(4)[:3], huge.data_ptr(), 3 * ne + 1, huge.data_ptr(), 10, _stream())
    v1, e1, s1 = _store(odo)
    assert odo.pose().tobytes() == pose_before.tobytes()
    assert e1.tobytes() == e0.tobytes() and s1.tobytes() == s0.tobytes()
    for key in ("n_scans", "n_added", "dropped_scans", "compactions", "n_edge", "n_surface"):
        assert v1[key] == v0[key], key
    assert v1["edge_offsets"].tolist() == v0["edge_offsets"].tolist()
    odo.close()
    fx.close()


def test_no_side_effects_on_the_batch():
    """After update_batch, the batch's downloads, its device view and a following lfx_localize_batch give the same bits as
    before the odometry ran."""
    from lidar_feature_extraction_amd import make_sequence
    from oracle import binding as OB
    rings, cols, n = 32, 1024, 4
    clouds, _ = make_sequence(n, rings, cols, seed=8600)
    fx = _fx(rings, cols, n)
    d, _ = _extract(fx, clouds)
    maps = [OB.extract(c, canonical_ties=False) for c in make_sequence(2, rings, cols, seed=8690)[0]]
    import torch
    d_emap = torch.from_numpy(np.ascontiguousarray(np.concatenate([m["edge_points"] for m in maps]), np.float32)).to(_dev())
    d_smap = torch.from_numpy(np.ascontiguousarray(np.concatenate([m["surface_points"] for m in maps]), np.float32)).to(_dev())
    emap, smap = fx.make_map(d_emap.data_ptr(), d_emap.shape[0], 1.0, _stream()), fx.make_map(d_smap.data_ptr(), d_smap.shape[0], 1.0, _stream())
    poses = np.stack([np.eye(4)[:3]] * n)

    def snapshot():
        dl = [fx.download(s, _stream()) for s in range(n)]
        v = fx.device_view()
        total = sum(len(c) for c in clouds)
        dv = (_d2h(v.edge_points, total).tobytes(), _d2h(v.surface_points, total).tobytes(), _d2h(v.scan_info, n).tobytes())
        loc = fx.localize_batch(emap, smap, poses, K, MAX_ITER, 1.0, _stream())
        return dl, dv, loc
    before = snapshot()
    odo = fx.odometry()
    res = odo.update_batch(n, _stream())
    assert sum(r["aligned"] for r in res) == n - 1
    after = snapshot()
    for a, b in zip(before[0], after[0]):
        for f in ("labels", "curvature", "edge_index", "surface_index", "edge_points", "surface_points"):
            assert np.asarray(getattr(a, f)).tobytes() == np.asarray(getattr(b, f)).tobytes(), f
    assert before[1] == after[1]
    for a, b in zip(before[2], after[2]):
        assert a["pose"].tobytes() == b["pose"].tobytes() and (a["code"], a["iteration"], a["error"]) == (b["code"], b["iteration"], b["error"])
    odo.close()
    emap.close()
    smap.close()
    fx.close()


def test_validation_before_any_device_work():
    """n_scans other than the batch's size, n_neighbors outside [3, 16], n_local_scans 0, max_iter 0, an empty store and null
    arguments are refused, and the refused calls change nothing."""
    from lidar_feature_extraction_amd import make_sequence
    from lidar_feature_extraction_amd import binding as LB
    rings, cols = 16, 900
    fx = _fx(rings, cols, 2)
    odo = fx.odometry()
    with pytest.raises(LB.LfxError, match="no batch"):
        odo.update_batch(1, _stream())
    clouds, _ = make_sequence(2, rings, cols, seed=8700)
    d, _ = _extract(fx, clouds)
    with pytest.raises(LB.LfxError, match="n_scans"):
        odo.update_batch(1, _stream())
    with pytest.raises(LB.LfxError, match="n_scans"):
        odo.update_batch(3, _stream())
    for bad in (dict(n_neighbors=2), dict(n_neighbors=17), dict(n_local_scans=0), dict(max_iter=0), dict(edge_capacity_points=0),
                dict(surface_leaf=0.0), dict(edge_cell=-1.0)):
        with pytest.raises(LB.LfxError):
            fx.odometry(**bad)
    with pytest.raises(TypeError):
        fx.odometry(n_neighbours=15)
    L, ctx, null = fx._L, fx._ctx, C.c_void_p(0)
    res = (LB.OdometryResult * 2)()
    assert L.lfx_odometry_update_batch(ctx, odo.handle, 2, None, null) == -1
    assert L.lfx_odometry_update_batch(ctx, None, 2, res, null) == -1
    assert L.lfx_odometry_update(ctx, odo.handle, null, 5, null, 0, res, null) == -1       # a count without its cloud
    assert L.lfx_odometry_update(ctx, odo.handle, null, 0, null, 0, None, null) == -1
    assert L.lfx_odometry_update_host(ctx, odo.handle, null, 0, null, 7, res, null) == -1
    assert L.lfx_odometry_add(ctx, odo.handle, None, null, 0, null, 0, null) == -1
    assert L.lfx_odometry_create(ctx, None, C.byref(C.c_void_p())) == -1
    v = odo.view()
    assert (v["n_scans"], v["n_added"], v["n_edge"], v["n_surface"]) == (0, 0, 0, 0)
    assert np.array_equal(odo.pose(), np.eye(4)[:3])
    odo.close()
    fx.close()
