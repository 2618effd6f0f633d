"""lfx_mapper_* and the two savers (include/lfx.h): MapBuilder (map.hpp:95-153) with its map on the device, held to the
test-side restatement (tests/mapping_restatement.py, pinned by the reference's vectors in tests/test_mapping_reference.py)
bit for bit; the transform is odometry's (tests/odometry_restatement.transform).  Then the loop drive -> map -> file ->
localize end to end."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from lidar_feature_extraction_amd import Mapper, ScanMap, read_pcd
from lidar_feature_extraction_amd import binding as LB
from tests.mapping_restatement import ADDED, EMPTY, TOO_CLOSE, MapBuilder, pose, quaternion_matrix
from tests.odometry_restatement import transform

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = json.load(open(os.path.join(ROOT, "tests", "golden", "mapping_vectors.json")))
# The end-to-end test's bound on the localized position (m): 0.06, test_trajectory_against_the_ground_truth's.  First
# measured on an MI355X: 0.047 m, nearly all of it in z (xy within 0.023 m): the 16-ring, 15-degree sensor sees little of
# floor and ceiling.  A perturbation out of the ground plane as well leaves up to 0.09 m in z.
E2E_BOUND = 0.06


def _dev():
    import torch
    return torch.device("cuda", 0)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _up(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype).copy()).to(_dev())


def _fx(rings=16, cols=64, batch=1):
    from lidar_feature_extraction_amd import FeatureExtraction
    return FeatureExtraction(device=0, max_points_per_scan=rings * cols, max_batch=batch, max_points_per_ring=cols, max_rings=rings)


def _rotation(axis_angle):
    th = np.asarray(axis_angle, np.float64)
    k = np.linalg.norm(th)
    if k == 0:
        return np.eye(3)
    u = th / k
    Kx = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + np.sin(k) * Kx + (1 - np.cos(k)) * Kx @ Kx


def _records(points):
    p = np.asarray(points, np.float32).reshape(-1, 3)
    return np.hstack([p, np.ones((len(p), 1), np.float32)])


def _add_device(mapper, clouds, poses):
    """One lfx_mapper_add call over clouds packed back to back on the device (with a gap after each, so begins matter)."""
    begins, counts, parts, at = [], [], [], 0
    for c in clouds:
        c = np.asarray(c, np.float32).reshape(-1, 4)
        begins.append(at)
        counts.append(len(c))
        parts.append(c)
        parts.append(np.full((3, 4), 7.0, np.float32))
        at += len(c) + 3
    pts = _up(np.concatenate(parts))
    b, n = _up(np.array(begins, np.uint32), np.uint32), _up(np.array(counts, np.uint32), np.uint32)
    out = mapper.add(pts.data_ptr(), b.data_ptr(), n.data_ptr(), 1, len(clouds), at, np.stack(poses), _stream())
    import torch
    torch.cuda.current_stream().synchronize()
    return out


def _state(mapper):
    v = mapper.view()
    return v, mapper.points(_stream())


def test_reference_vectors_through_the_device(tmp_path):
    """test_map.cpp:67-110: TransformAdd of three points saved and read back as (0,1,0), (0,1,0), (3,1,0); IsEmpty before and
    after a point is added; an empty map writes no file."""
    fx = _fx()
    v = VECTORS["transform_add"]
    m = Mapper(fx)
    assert not m.save(str(tmp_path / "empty.pcd")) and not os.path.exists(tmp_path / "empty.pcd")
    outs = [m.add_host(_records(c["points"]), pose(quaternion_matrix(*c["quaternion_wxyz"]), c["translation"]), _stream())
            for c in v["clouds"]]
    assert outs == [ADDED, ADDED]
    assert m.save(str(tmp_path / "map.pcd"))
    loaded = read_pcd(str(tmp_path / "map.pcd"))
    assert loaded[:, :3].tolist() == v["loaded"]
    e = VECTORS["is_empty"]
    m2 = Mapper(fx)
    assert (m2.view()["n_points"] == 0) == e["before"] and not m2.view()["has_pose"]
    assert _add_device(m2, [_records(e["cloud"])], [np.eye(4)[:3]]).tolist() == [ADDED]
    assert (m2.view()["n_points"] == 0) == e["after"] and m2.view()["has_pose"]
    m.close(); m2.close(); fx.close()


def test_transform_bits():
    """Thresholds 0: every non-empty cloud is added; the map's bytes equal the restatement's transform of every cloud,
    concatenated in order (random poses with large angles and far translations, random 4th floats, sizes around 256)."""
    rng = np.random.default_rng(11)
    fx = _fx()
    m = Mapper(fx, translation_threshold=0.0, rotation_threshold=0.0, initial_capacity_points=1 << 16)
    sizes = [0, 1, 7, 255, 256, 257, 5000, 20011]
    want, clouds, poses = [], [], []
    for i in range(14):
        n = int(rng.choice(sizes))
        clouds.append(rng.normal(0, 40, (n, 4)).astype(np.float32))
        poses.append(pose(_rotation(rng.normal(0, 1.5, 3)), rng.normal(0, 60, 3)))
        if n:
            want.append(transform(poses[-1], clouds[-1]))
    out = _add_device(m, clouds, poses)
    assert out.tolist() == [EMPTY if len(c) == 0 else ADDED for c in clouds]
    v, got = _state(m)
    assert got.tobytes() == np.concatenate(want).tobytes()
    assert v["last_pose"].tobytes() == [p for p, c in zip(poses, clouds) if len(c)][-1].tobytes()
    m.close(); fx.close()


def _sequence(rng, n):
    """clouds (empty ones first, between keyframes and after) and poses of small and large steps"""
    clouds, poses, P = [], [], np.eye(4)[:3].copy()
    for i in range(n):
        big = rng.random() < 0.3
        R = _rotation(rng.normal(0, 0.15 if big else 0.02, 3)) @ P[:, :3]
        t = P[:, 3] + rng.normal(0, 0.8 if big else 0.15, 3)
        P = pose(R, t)
        k = 0 if (i < 2 or rng.random() < 0.2) else int(rng.integers(1, 600))
        clouds.append(rng.normal(0, 20, (k, 4)).astype(np.float32))
        poses.append(P)
    return clouds, poses


@pytest.mark.parametrize("thresholds", [(1.0, 0.1), (0.0, 0.0), (1e300, 1e300)])
def test_gate_as_a_sequence(thresholds):
    """The default thresholds, 0 (every non-empty cloud is added) and huge (only the first is): outcomes, counters, last
    pose and map equal the restatement of MapBuilder::Callback."""
    rng = np.random.default_rng(12)
    clouds, poses = _sequence(rng, 120)
    fx = _fx()
    tt, rt = thresholds
    m = Mapper(fx, translation_threshold=tt, rotation_threshold=rt)
    ref = MapBuilder(tt, rt)
    want = [ref.callback(c, p) for c, p in zip(clouds, poses)]
    got = _add_device(m, clouds, poses)
    assert got.tolist() == want
    v, pts = _state(m)
    assert pts.tobytes() == ref.map().tobytes()
    assert (v["n_added"], v["n_empty"], v["n_too_close"]) == (ref.counts["added"], ref.counts["empty"], ref.counts["too_close"])
    assert v["last_pose"].tobytes() == ref.prev.tobytes()
    if tt == 0.0:
        assert want.count(TOO_CLOSE) == 0
    if tt > 1.0:
        assert want.count(ADDED) == 1
    else:
        assert want.count(ADDED) > 5
    if tt == 1.0:
        assert want.count(TOO_CLOSE) > 5
    m.close(); fx.close()


def test_entry_points_agree():
    """One call of n clouds, n calls of one cloud, and the host form: the same outcomes, map bytes and view."""
    rng = np.random.default_rng(13)
    clouds, poses = _sequence(rng, 60)
    fx = _fx()
    a, b, h = Mapper(fx), Mapper(fx), Mapper(fx)
    oa = _add_device(a, clouds, poses).tolist()
    ob = [int(_add_device(b, [c], [p])[0]) for c, p in zip(clouds, poses)]
    oh = [h.add_host(c, p, _stream()) for c, p in zip(clouds, poses)]
    assert oa == ob == oh
    views = [_state(x) for x in (a, b, h)]
    for v, pts in views[1:]:
        assert pts.tobytes() == views[0][1].tobytes()
        for k in ("n_points", "n_added", "n_empty", "n_too_close", "has_pose"):
            assert v[k] == views[0][0][k], k
        assert v["last_pose"].tobytes() == views[0][0]["last_pose"].tobytes()
    for x in (a, b, h):
        x.close()
    fx.close()


def test_growth_and_max_points():
    """Initial capacity 1 000 and a few hundred adds: the map equals the restatement across several growths.  A call past
    max_points fails with everything unchanged; the next call that fits succeeds."""
    rng = np.random.default_rng(14)
    fx = _fx()
    m = Mapper(fx, translation_threshold=0.0, rotation_threshold=0.0, initial_capacity_points=1000, max_points=60000)
    ref = MapBuilder(0.0, 0.0)
    caps = set()
    for i in range(300):
        c = rng.normal(0, 10, (int(rng.integers(0, 300)), 4)).astype(np.float32)
        p = pose(_rotation(rng.normal(0, 1, 3)), rng.normal(0, 10, 3))
        want = ref.callback(c, p)
        if ref.n_points > 60000:
            break
        got = m.add_host(c, p, _stream()) if i % 2 else int(_add_device(m, [c], [p])[0])
        assert got == want
        caps.add(m.view()["capacity_points"])
    assert len(caps) >= 4
    v0, pts0 = _state(m)
    assert pts0.tobytes() == ref.map()[:v0["n_points"]].tobytes()
    # past max_points: all or nothing
    room = 60000 - v0["n_points"]
    too_many = [rng.normal(0, 1, (room, 4)).astype(np.float32), rng.normal(0, 1, (1, 4)).astype(np.float32)]
    ps = [pose(np.eye(3), [100.0 + k, 0, 0]) for k in range(2)]
    with pytest.raises(LB.LfxError) as e:
        _add_device(m, too_many, ps)
    assert e.value.code == LB.ERR_CAPACITY
    v1, pts1 = _state(m)
    assert pts1.tobytes() == pts0.tobytes()
    for k in ("n_points", "n_added", "n_empty", "n_too_close", "capacity_points"):
        assert v1[k] == v0[k]
    assert v1["last_pose"].tobytes() == v0["last_pose"].tobytes()
    assert _add_device(m, too_many[:1], ps[:1]).tolist() == [ADDED]
    assert m.view()["n_points"] == 60000 and m.view()["capacity_points"] == 60000
    m.close(); fx.close()


def test_argument_checks():
    fx = _fx()
    m = Mapper(fx)
    d = _up(np.zeros((4, 4), np.float32))
    u = _up(np.zeros(4, np.uint32), np.uint32)
    eye = np.eye(4)[:3]
    for args, what in (((d.data_ptr(), u.data_ptr(), u.data_ptr(), 0, 1, 4, [eye]), "stride 0"),
                       ((d.data_ptr(), u.data_ptr(), u.data_ptr(), 1, 0, 4, np.zeros((0, 3, 4))), "no clouds"),
                       ((d.data_ptr(), u.data_ptr(), u.data_ptr(), 1, 1, 4, [np.full((3, 4), np.nan)]), "nan pose")):
        with pytest.raises(LB.LfxError) as e:
            m.add(*args, stream=_stream())
        assert e.value.code == -1, what
    # a cloud past total_points
    n = _up(np.array([5], np.uint32), np.uint32)
    with pytest.raises(LB.LfxError) as e:
        m.add(d.data_ptr(), u.data_ptr(), n.data_ptr(), 1, 1, 4, [eye], _stream())
    assert e.value.code == -1 and "total_points" in str(e.value)
    assert m.view()["n_points"] == 0 and m.view()["n_added"] == 0
    with pytest.raises(TypeError):
        Mapper(fx, nonsense=1)
    with pytest.raises(LB.LfxError):
        Mapper(fx, initial_capacity_points=0)
    m.close(); fx.close()


def test_last_device_batch():
    """add_batch('edge' / 'surface', truth poses) over an extracted make_sequence batch equals the restatement on the
    downloaded clouds, and leaves the batch's results as they were."""
    import torch
    from lidar_feature_extraction_amd import concat, make_sequence
    rings, cols, n = 16, 900, 8
    clouds, truth = make_sequence(n, rings, cols, seed=9100, step=0.4, yaw_step_deg=3.0)
    fx = _fx(rings, cols, n)
    d = torch.from_numpy(concat(clouds).view(np.uint8).copy()).to(_dev())
    fx.extract_batch_device(d.data_ptr(), [len(c) for c in clouds], _stream())
    before = [fx.download(s, _stream()) for s in range(n)]
    for which in ("edge", "surface"):
        m = Mapper(fx)
        ref = MapBuilder()
        want = [ref.callback(getattr(before[s], which + "_points"), truth[s]) for s in range(n)]
        got = m.add_batch(which, truth, _stream())
        assert got.tolist() == want and want.count(ADDED) >= 2 and want.count(TOO_CLOSE) >= 2
        v, pts = _state(m)
        assert pts.tobytes() == ref.map().tobytes()
        m.close()
    after = [fx.download(s, _stream()) for s in range(n)]
    for a, b in zip(before, after):
        for k in ("edge_points", "surface_points", "edge_index", "surface_index", "labels"):
            assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    fx.close()


def test_odometry_save(tmp_path):
    """Odometry.save writes the store (GetAll): the files read back equal the store's x, y, z; an empty store writes
    nothing."""
    from lidar_feature_extraction_amd import make_sequence
    rings, cols = 16, 900
    clouds, _ = make_sequence(4, rings, cols, seed=9200)
    fx = _fx(rings, cols, 1)
    odo = fx.odometry()
    assert odo.save(str(tmp_path)) == (False, False)
    assert not os.path.exists(tmp_path / "edge.pcd") and not os.path.exists(tmp_path / "surface.pcd")
    for c in clouds:
        fx.ExtractFeatures(c)
        odo.update_batch(1)
    assert odo.save(str(tmp_path), _stream()) == (True, True)
    v = odo.view()
    from lidar_feature_extraction_amd.extraction import _download
    for name, ptr, n in (("edge", v["edge_points"], v["n_edge"]), ("surface", v["surface_points"], v["n_surface"])):
        store = _download(fx._L, ptr, n, _stream())
        got = read_pcd(str(tmp_path / (name + ".pcd")))
        assert len(got) == n > 0
        assert got[:, :3].tobytes() == store[:, :3].tobytes() and np.all(got[:, 3] == 1.0)
    odo.close(); fx.close()


def test_drive_map_file_localize(tmp_path):
    """The loop drive -> map -> file -> localize: a make_sequence drive of 16 x 900 scans with a step of 0.25 m (keyframes
    every few scans, well inside the 20 x 12 m room) into two mappers at the ground-truth poses, saved, loaded back with
    ScanMap.from_pcd, and every scan of the drive re-extracted and localized from its truth pose perturbed by 0.3 m in the
    ground plane and 2 degrees about the vertical (a ground vehicle's prior): the recovered position lies within E2E_BOUND
    of the truth."""
    import torch
    from lidar_feature_extraction_amd import concat, make_sequence
    rings, cols, n = 16, 900, 12
    clouds, truth = make_sequence(n, rings, cols, seed=9300, step=0.25, yaw_step_deg=1.0)
    fx = _fx(rings, cols, n)
    d = torch.from_numpy(concat(clouds).view(np.uint8).copy()).to(_dev())
    fx.extract_batch_device(d.data_ptr(), [len(c) for c in clouds], _stream())
    em, sm = Mapper(fx), Mapper(fx)
    oe = em.add_batch("edge", truth, _stream())
    os_ = sm.add_batch("surface", truth, _stream())
    assert oe.tolist() == os_.tolist() and 3 <= oe.tolist().count(ADDED) <= 6, oe
    assert em.save(str(tmp_path / "edge.pcd"), _stream()) and sm.save(str(tmp_path / "surface.pcd"), _stream())
    emap, smap = ScanMap.from_pcd(fx, str(tmp_path / "edge.pcd")), ScanMap.from_pcd(fx, str(tmp_path / "surface.pcd"))
    assert emap.info()["n_points"] == em.view()["n_points"] and smap.info()["n_points"] == sm.view()["n_points"]
    rng = np.random.default_rng(9301)
    initial = []
    for P in truth:
        d_t = rng.normal(size=3)
        d_t[2] = 0.0
        d_t = d_t / np.linalg.norm(d_t) * 0.3
        yaw = rng.choice([-1.0, 1.0]) * np.deg2rad(2.0)
        initial.append(pose(_rotation([0.0, 0.0, yaw]) @ P[:, :3], P[:, 3] + d_t))
    fx.extract_batch_device(d.data_ptr(), [len(c) for c in clouds], _stream())
    res = fx.localize_batch(emap, smap, np.stack(initial), max_iter=40)
    err = [float(np.linalg.norm(r["pose"][:, 3] - P[:, 3])) for r, P in zip(res, truth)]
    rot = [float(np.rad2deg(np.arccos(np.clip((np.trace(r["pose"][:, :3].T @ P[:, :3]) - 1) / 2, -1, 1)))) for r, P in zip(res, truth)]
    print("drive -> map -> file -> localize: max position error %.4f m, max rotation error %.3f deg" % (max(err), max(rot)))
    assert max(err) < E2E_BOUND, err
    emap.close(); smap.close(); em.close(); sm.close(); fx.close()


def test_calls_on_alternating_streams(tmp_path):
    """Successive calls on two streams, each call after a large one growing the map: the growth copy is ordered behind the
    previous call's append on the other stream, and so is a save; map and file equal the restatement."""
    import torch
    rng = np.random.default_rng(15)
    fx = _fx()
    m = Mapper(fx, translation_threshold=0.0, rotation_threshold=0.0, initial_capacity_points=1000)
    ref = MapBuilder(0.0, 0.0)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    inputs = []
    for i in range(8):
        c = rng.normal(0, 10, ((150000 + 1000 * i) if i % 2 == 0 else 3, 4)).astype(np.float32)
        p = pose(_rotation(rng.normal(0, 1, 3)), rng.normal(0, 10, 3))
        assert ref.callback(c, p) == ADDED
        inputs.append((_up(c), _up(np.array([0], np.uint32), np.uint32), _up(np.array([len(c)], np.uint32), np.uint32), p, len(c)))
    torch.cuda.synchronize()                   # (the inputs are on the device before any call)
    caps = []
    for i, (d, b, n, p, k) in enumerate(inputs):
        out = m.add(d.data_ptr(), b.data_ptr(), n.data_ptr(), 1, 1, k, [p], streams[i % 2].cuda_stream)
        assert out.tolist() == [ADDED]
        caps.append(m.view()["capacity_points"])
    assert len(set(caps)) >= 3
    assert m.save(str(tmp_path / "map.pcd"), streams[0].cuda_stream)
    torch.cuda.synchronize()
    want = ref.map()
    assert m.points().tobytes() == want.tobytes()
    assert read_pcd(str(tmp_path / "map.pcd"))[:, :3].tobytes() == np.ascontiguousarray(want[:, :3]).tobytes()
    m.close(); fx.close()
