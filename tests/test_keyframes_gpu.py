"""The keyframe store on the device (lfx_keyframes, include/lfx.h) against its restatement (tests/keyframes_restatement.py):
every device result is compared byte for byte -- nothing here has a tolerance.

The transform kernel gives each workgroup lfx::kKfRun = 1024 consecutive source records (kKfThreads 256 lanes x kKfPerLane 4,
csrc/lfx_kernels_keyframes.hpp; KR.RUN) counted from the first record of the range it was launched for, and each wave 64
consecutive records per step (KR.WAVE).  The `build` case puts a keyframe boundary at -1, 0 and +1 of every multiple of 64 up
to 4096, has runs of 300 one-record and 40 empty keyframes, keyframes longer than a run, and ranges that start and end inside a
run (tests/test_keyframes_expect.py holds those conditions)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import deskew_cases as K
from tests import keyframes_restatement as KR
from tests import pose_graph_cases as PG
from tests import segment_cases as S

pytestmark = pytest.mark.gpu
GUARD = 64                                   # guard records behind a build's n_out


def _up(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype).copy()).to(K.dev())


def _bytes(ptr, nbytes):
    """nbytes from a device address, after a synchronise"""
    out = np.zeros(int(nbytes), np.uint8)
    if nbytes:
        K.sync()
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(out.ctypes.data, int(ptr), out.nbytes, 2) == 0
    return out


def _pack(clouds, gap=3, stride=1):
    """clouds back to back on the device with a gap after each (so begins matter) and counts `stride` words apart (the words
    between them hold garbage): what Keyframes.clouds() takes, and the tensors to keep alive"""
    begins, parts, at = [], [], 0
    for c in clouds:
        begins.append(at)
        parts += [np.asarray(c, np.float32).reshape(-1, 4), np.full((gap, 4), 7.0, np.float32)]
        at += len(c) + gap
    counts = np.full((len(clouds) - 1) * stride + 1, 0xDEADBEEF, np.uint32)
    counts[::stride] = [len(c) for c in clouds]
    keep = (_up(np.concatenate(parts)), _up(np.array(begins, np.uint32), np.uint32), _up(counts, np.uint32))
    return keep, (keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), stride, at)


def _device_store(fx, store, strides=(1, 1)):
    """a device store of the restatement's capacities holding its keyframes, added in one call"""
    from lidar_feature_extraction_amd import Keyframes
    kf = fx.keyframes(store.max_keyframes, store.max_points)
    if len(store):
        ke, e = _pack(store.clouds[KR.EDGE], 3, strides[0])
        ks, s = _pack(store.clouds[KR.SURFACE], 1, strides[1])
        assert kf.add(Keyframes.clouds(*e), Keyframes.clouds(*s), store.poses(), K.stream()) == 0
        K.sync()
    return kf


def _state(kf):
    """view() and every byte the store holds on the device: records to max_points, begins to max_keyframes + 1, every pose"""
    v = kf.view(K.stream())
    i = kf.info()
    blobs = [_bytes(v["points"][q], 16 * i["max_points"][q]).tobytes() for q in (0, 1)]
    blobs += [_bytes(v["begin"][q], 8 * (i["max_keyframes"] + 1)).tobytes() for q in (0, 1)]
    blobs.append(_bytes(v["poses"], 96 * i["max_keyframes"]).tobytes())
    return v, blobs


def _build_guarded(kf, kind, first, count, want, stream=None):
    """a build into a buffer with GUARD records behind the cloud: the cloud's bytes are `want`'s, the guards untouched"""
    import torch
    n = len(want)
    out = torch.full((n + GUARD, 4), -123.25, dtype=torch.float32, device=K.dev())
    got = kf.build(kind, first, count, d_out=out.data_ptr(), capacity_points=n, stream=K.stream() if stream is None else stream)
    K.sync()
    host = out.cpu().numpy()
    assert got == n, (kind, first, count, got, n)
    assert host[:n].tobytes() == want.tobytes(), (kind, first, count, int((host[:n].view(np.uint32) != want.view(np.uint32)).any(axis=1).sum()))
    assert (host[n:] == -123.25).all(), (kind, first, count)


@pytest.fixture(scope="module")
def fx():
    f = K.fx_for(16, 64, 3)
    yield f
    f.close()


@pytest.fixture(scope="module")
def bits(fx):
    store = KR.bits_case()[0]
    kf = _device_store(fx, store)
    yield store, kf
    kf.close()


def test_build_bits(bits):
    store, kf = bits
    for kind in (KR.EDGE, KR.SURFACE):
        for first, count in KR.bits_ranges(store.begin(kind)):
            _build_guarded(kf, kind, first, count, store.build(kind, first, count))
    # the store holds what went in, -0.0 and all, and the prefix of the counts
    v = kf.view(K.stream())
    assert v["n_keyframes"] == len(store)
    for kind in (KR.EDGE, KR.SURFACE):
        n = int(store.begin(kind)[-1])
        assert v["n_points"][kind] == n
        assert _bytes(v["points"][kind], 16 * n).tobytes() == store.records(kind).tobytes()
        assert _bytes(v["begin"][kind], 8 * (len(store) + 1)).tobytes() == store.begin(kind).tobytes()
    assert _bytes(v["poses"], 96 * len(store)).tobytes() == store.poses().tobytes()
    # build() without a target makes its own tensor; more records than the capacity is refused
    assert kf.build("edge").cpu().numpy().tobytes() == store.build(KR.EDGE).tobytes()
    from lidar_feature_extraction_amd import binding as B
    with pytest.raises(B.LfxError) as e:
        kf.build("edge", 0, len(store), d_out=1, capacity_points=int(store.begin(KR.EDGE)[-1]) - 1, stream=K.stream())
    assert e.value.code == B.ERR_CAPACITY


def test_build_equals_a_fresh_mapper_fed_the_same_clouds(bits, fx):
    """The cross-check with the code that was there before: one Mapper.add (thresholds 0) of the same clouds and poses."""
    store, kf = bits
    for kind in (KR.EDGE, KR.SURFACE):
        n = int(store.begin(kind)[-1])
        m = fx.mapper(translation_threshold=0.0, rotation_threshold=0.0, initial_capacity_points=n)
        keep, (pts, begin, count, stride, total) = _pack(store.clouds[kind])
        m.add(pts, begin, count, stride, len(store), total, store.poses(), K.stream())
        want = m.points(K.stream())
        assert len(want) == n
        assert kf.build(kind).cpu().numpy().tobytes() == want.tobytes()
        m.close()


def test_add_from_a_batch_with_strides_and_from_the_host(fx):
    from lidar_feature_extraction_amd import Keyframes, make_scan
    from lidar_feature_extraction_amd import binding as B
    rng = np.random.default_rng(77)
    clouds = [make_scan(16, 64, seed=500 + k) for k in range(3)]
    d, got = K.extract(fx, clouds)
    poses = KR.bits_poses(3, 8)
    want = KR.Store(12, (8192, 8192))
    assert want.add([g.edge_points for g in got], [g.surface_points for g in got], poses) == 0
    assert int(want.begin(KR.EDGE)[-1]) + int(want.begin(KR.SURFACE)[-1]) > 0
    kf = fx.keyframes(12, 8192)
    assert kf.add_batch(poses, K.stream()) == 0                      # the last device batch, as it lies in the context
    # counts 5 (edge) and 2 (surface) words apart, gaps between the clouds; among the records -0.0
    e2 = [rng.normal(0, 9, (k, 4)).astype(np.float32) for k in (5, 0, 257, 1)]
    s2 = [rng.normal(0, 9, (k, 4)).astype(np.float32) for k in (0, 0, 64, 300)]
    e2[0][1] = [-0.0, 0.0, -0.0, -0.0]
    p2 = KR.bits_poses(4, 9)
    assert want.add(e2, s2, p2) == 3
    ke, e = _pack(e2, 3, 5)
    ks, s = _pack(s2, 2, 2)
    assert kf.add(Keyframes.clouds(*e), Keyframes.clouds(*s), p2, K.stream()) == 3
    # from the host: both clouds, one empty, both empty
    for e3, s3, p3 in ((e2[2], s2[3], p2[0]), (np.zeros((0, 4), np.float32), s2[2], p2[1]), (np.zeros((0, 4), np.float32),) * 2 + (p2[2],)):
        kid = len(want)
        assert want.add([e3], [s3], [p3]) == kid
        assert kf.add_host(e3, s3, p3, K.stream()) == kid

    def same():
        v = kf.view(K.stream())
        assert v["n_keyframes"] == len(want) == 10
        for kind in (KR.EDGE, KR.SURFACE):
            assert v["n_points"][kind] == int(want.begin(kind)[-1])
            assert _bytes(v["points"][kind], 16 * v["n_points"][kind]).tobytes() == want.records(kind).tobytes()
            assert _bytes(v["begin"][kind], 8 * (len(want) + 1)).tobytes() == want.begin(kind).tobytes()
            assert kf.build(kind).cpu().numpy().tobytes() == want.build(kind).tobytes()
        assert kf.poses(stream=K.stream()).tobytes() == want.poses().tobytes()

    same()
    # the refusals: the store, on the host and on the device, is as it was
    v0, before = _state(kf)
    few = [np.zeros((1, 4), np.float32)] * 3
    big = [np.zeros((1, 4), np.float32), rng.normal(0, 1, (8192, 4)).astype(np.float32)]
    ok_pose = KR.bits_poses(3, 10)
    bad_pose = ok_pose.copy()
    bad_pose[1, 2, 3] = np.nan
    cases = [(few, few, ok_pose, None, B.ERR_CAPACITY),                              # 10 + 3 keyframes > 12
             (big, big[::-1], ok_pose[:2], None, B.ERR_CAPACITY),                    # more records than max_points
             (few[:2], few[:2], bad_pose[:2], None, B.ERR_INVALID_ARGUMENT),         # a pose that is not finite
             (few[:2], few[:2], ok_pose[:2], 4, B.ERR_INVALID_ARGUMENT)]             # a cloud past total_points
    for ec, sc, pc, total, code in cases:
        ke, e = _pack(ec)
        ks, s = _pack(sc)
        if total is not None:
            e = e[:4] + (total,)
        with pytest.raises(B.LfxError) as err:
            kf.add(Keyframes.clouds(*e), Keyframes.clouds(*s), pc, K.stream())
        assert err.value.code == code, (err.value, code)
    with pytest.raises(B.LfxError) as err:
        kf.add_host(big[1], big[1][:1], ok_pose[0], K.stream())
    assert err.value.code == B.ERR_CAPACITY
    with pytest.raises(B.LfxError) as err:
        kf.add_host(few[0], few[0], bad_pose[1], K.stream())
    assert err.value.code == B.ERR_INVALID_ARGUMENT
    v1, after = _state(kf)
    assert v0 == v1 and before == after
    same()
    kf.close()
    del d


def test_follow_a_pose_graph_and_set_poses(fx):
    g = PG.circles()[0]
    n = len(g["poses"])
    rng = np.random.default_rng(31)
    edge = [rng.normal(0, 20, (int(k), 4)).astype(np.float32) for k in rng.integers(0, 40, n)]
    surface = [rng.normal(0, 20, (int(k), 4)).astype(np.float32) for k in rng.integers(0, 90, n)]
    want = KR.Store(n, (sum(map(len, edge)), sum(map(len, surface))))
    assert want.add(edge, surface, g["poses"]) == 0
    kf = _device_store(fx, want)
    pg = fx.pose_graph(n, len(g["edges"]))
    pg.add_nodes(g["poses"], K.stream())
    pg.add_edges(g["edges"], K.stream())
    before = [kf.build(kind).cpu().numpy() for kind in (0, 1)]
    assert all(b.tobytes() == want.build(kind).tobytes() for kind, b in enumerate(before))
    pg.optimize(K.stream())
    kf.follow(pg, stream=K.stream())
    moved = pg.poses(stream=K.stream())
    assert kf.poses(stream=K.stream()).tobytes() == moved.tobytes() and moved.tobytes() != g["poses"].tobytes()
    want.set_poses(moved)
    for kind in (0, 1):
        got = kf.build(kind).cpu().numpy()
        assert got.tobytes() == want.build(kind).tobytes() and got.tobytes() != before[kind].tobytes()
    # a range from a device array: only that range moves (d_poses[k] goes to keyframe k)
    other = KR.bits_poses(n, 12)
    d_other = _up(other, np.float64)
    kf.follow(d_other.data_ptr(), 100, 17, K.stream())
    want.set_poses(other[100:117], 100)
    assert kf.poses(stream=K.stream()).tobytes() == want.poses().tobytes()
    # set_poses of a sub-range moves only that range
    kf.set_poses(g["poses"][40:45], 40, K.stream())
    want.set_poses(g["poses"][40:45], 40)
    assert kf.poses(stream=K.stream()).tobytes() == want.poses().tobytes()
    assert want.poses()[39].tobytes() == moved[39].tobytes() and want.poses()[40].tobytes() == g["poses"][40].tobytes()
    for kind in (0, 1):
        assert kf.build(kind, 30, 100).cpu().numpy().tobytes() == want.build(kind, 30, 100).tobytes()
    pg.close()
    kf.close()


def _submap_guarded(kf, store, kind, center, radius, first, count, capacity, room=None):
    import torch
    want, wres = store.submap(kind, center, radius, first, count, capacity)
    room = capacity if room is None else room
    out = torch.full((room + GUARD, 4), -123.25, dtype=torch.float32, device=K.dev())
    _, res = kf.submap(kind, center, radius, first, len(store) - first if count is None else count, d_out=out.data_ptr(), capacity_points=capacity,
                       stream=K.stream())
    K.sync()
    host = out.cpu().numpy()
    assert res == wres, (res, wres)
    assert host[:len(want)].tobytes() == want.tobytes() and (host[len(want):] == -123.25).all()
    return res


def test_submap_by_hand(fx):
    store, c, _, _, _ = KR.sphere_case()
    kf = _device_store(fx, store)
    for kind in (KR.EDGE, KR.SURFACE):
        for radius, flags in KR.SPHERE_WANT.items():
            res = _submap_guarded(kf, store, kind, c, radius, 0, None, 64)
            assert res["n_selected"] == sum(flags) and not res["truncated"]
    # stops exactly at the capacity; one record short of keyframe 4; the first does not fit; a smaller one behind is not written
    assert _submap_guarded(kf, store, KR.EDGE, c, 7.0, 0, None, 14) == dict(n_selected=6, n_written_keyframes=5, n_points=14, first_id=0, last_id=4, truncated=True)
    assert _submap_guarded(kf, store, KR.EDGE, c, 7.0, 0, None, 13) == dict(n_selected=6, n_written_keyframes=4, n_points=9, first_id=0, last_id=3, truncated=True)
    assert _submap_guarded(kf, store, KR.EDGE, c, 7.0, 0, None, 4)["last_id"] == 0
    # a window that leaves the near keyframes out
    res = _submap_guarded(kf, store, KR.EDGE, c, 7.0, 4, 3, 64)
    assert (res["first_id"], res["last_id"], res["n_points"]) == (4, 5, 11)
    # nothing selected, nothing that fits, only an empty keyframe selected, an empty window: n_points 0, the guards untouched
    for radius, first, count, capacity in ((0.5, 0, None, 64), (7.0, 0, None, 2), (2.0, 3, 1, 64), (7.0, 2, 0, 64)):
        res = _submap_guarded(kf, store, KR.EDGE, c, radius, first, count, capacity)
        assert res["n_points"] == 0
    # its own tensor
    cloud, res = kf.submap("surface", c, 5.0, stream=K.stream())
    K.sync()
    assert cloud.cpu().numpy().tobytes() == store.submap(KR.SURFACE, c, 5.0)[0].tobytes()
    kf.close()


def test_submap_selection_on_1000_random_poses(fx):
    rng = np.random.default_rng(41)
    n = 1000
    poses = np.array([KR.pose(rng.normal(0, 1.5, 3), rng.normal(0, 30, 3)) for _ in range(n)])
    edge = [rng.normal(0, 5, (int(k), 4)).astype(np.float32) for k in rng.choice([0, 1, 2, 3, 70], n)]
    store = KR.Store(n, (sum(map(len, edge)), 1))
    assert store.add(edge, [np.zeros((0, 4), np.float32)] * n, poses) == 0
    kf = _device_store(fx, store)
    total = int(store.begin(KR.EDGE)[-1])
    for center, radius, first, count, capacity in (([3.0, -4.0, 5.0], 40.0, 0, None, total), ([0.0, 0.0, 0.0], 25.0, 300, 650, total),
                                                   ([10.0, 10.0, 0.0], 60.0, 0, None, total // 3), ([0.0, 0.0, 0.0], 1e-3, 0, None, total)):
        res = _submap_guarded(kf, store, KR.EDGE, center, radius, first, count, capacity)
        print("submap of 1000: radius %g window (%d, %s) capacity %d -> %s" % (radius, first, count, capacity, res))
    assert _submap_guarded(kf, store, KR.EDGE, [3.0, -4.0, 5.0], 40.0, 0, None, total)["n_selected"] > 300
    assert _submap_guarded(kf, store, KR.SURFACE, [3.0, -4.0, 5.0], 40.0, 0, None, 1, room=1)["n_points"] == 0
    kf.close()


@pytest.fixture(scope="module")
def hold():
    h = S.Hold()
    print("a hold: %d units, %.3f ms per %d measured" % (h.amount, h.ms_per_unit, h.unit))
    yield h
    for what, ms in h.issue_ms:
        print("held %.0f ms; issued %.3f ms after the hold was queued: %s" % (S.HOLD_MS, ms, what))


def test_calls_on_three_streams_are_ordered_one_behind_the_other(fx, hold):
    """Three held cases (tests/segment_cases.py Hold, as tests/test_newer_streams_gpu.py uses it): the producer's stream is
    kept busy, the dependent calls are issued on other streams while an event behind the producer says it has not run, and
    the cloud is the one the producer leaves.  (1) add on A (from the host: the add that does not wait), build on B.
    (2) follow on B, build on A.  (3) add on A, follow on B, build on a third stream.  Every stream has run the busy kernel
    and a build before the part that counts."""
    import torch
    store, c, edge, surface, poses = KR.sphere_case()
    want = KR.Store(len(store) + 2, (64, 64))
    assert want.add(edge, surface, poses) == 0
    kf = _device_store(fx, want)
    a, b = S.two_streams()
    third = torch.cuda.Stream()
    others = [KR.bits_poses(len(store) + 2, seed) for seed in (13, 14)]
    d_others = [_up(o, np.float64) for o in others]
    new = [(np.arange(20, dtype=np.float32).reshape(5, 4), np.arange(12, dtype=np.float32).reshape(3, 4)),
           (np.arange(8, dtype=np.float32).reshape(2, 4) - 3.0, np.arange(16, dtype=np.float32).reshape(4, 4) + 0.5)]
    outs = [torch.full((64 + GUARD, 4), -123.25, dtype=torch.float32, device=K.dev()) for _ in range(4)]
    for st in (a, b, third):
        hold._run(1, st)
        kf.build("edge", d_out=outs[3].data_ptr(), capacity_points=64, stream=st.cuda_stream)
    K.sync()

    def check(out, n, stream):
        stream.synchronize()
        host = out.cpu().numpy()
        cloud = want.build(KR.EDGE)
        assert n == len(cloud) and host[:n].tobytes() == cloud.tobytes() and (host[n:] == -123.25).all()

    # (1)
    hold(a)
    assert kf.add_host(new[0][0], new[0][1], poses[0], a.cuda_stream) == len(store)
    e = S.event_behind(a)
    n = kf.build("edge", d_out=outs[0].data_ptr(), capacity_points=64, stream=b.cuda_stream)
    hold.still_held(e, "keyframes: add on A, build on B")
    assert want.add([new[0][0]], [new[0][1]], [poses[0]]) == len(store)
    check(outs[0], n, b)
    # (2)
    K.sync()
    hold(b)
    kf.follow(d_others[0].data_ptr(), 0, len(want), b.cuda_stream)
    e = S.event_behind(b)
    n = kf.build("edge", d_out=outs[1].data_ptr(), capacity_points=64, stream=a.cuda_stream)
    hold.still_held(e, "keyframes: follow on B, build on A")
    want.set_poses(others[0][:len(want)])
    check(outs[1], n, a)
    # (3)
    K.sync()
    hold(a)
    assert kf.add_host(new[1][0], new[1][1], poses[1], a.cuda_stream) == len(store) + 1
    e = S.event_behind(a)
    kf.follow(d_others[1].data_ptr(), 0, len(store) + 2, b.cuda_stream)
    n = kf.build("edge", d_out=outs[2].data_ptr(), capacity_points=64, stream=third.cuda_stream)
    hold.still_held(e, "keyframes: add on A, follow on B, build on a third stream")
    assert want.add([new[1][0]], [new[1][1]], [poses[1]]) == len(store) + 1
    want.set_poses(others[1])
    check(outs[2], n, third)
    K.sync()
    assert kf.build("surface").cpu().numpy().tobytes() == want.build(KR.SURFACE).tobytes()
    assert kf.poses(stream=K.stream()).tobytes() == want.poses().tobytes()
    kf.close()


def test_save_writes_the_builds(fx, tmp_path):
    from lidar_feature_extraction_amd import read_pcd
    store, c, edge, surface, poses = KR.sphere_case()
    kf = _device_store(fx, store)
    os.makedirs(tmp_path / "both")
    assert kf.save(str(tmp_path / "both"), K.stream()) == (True, True)
    for kind, name in ((KR.EDGE, "edge.pcd"), (KR.SURFACE, "surface.pcd")):
        got = read_pcd(str(tmp_path / "both" / name))
        assert got[:, :3].tobytes() == store.build(kind)[:, :3].tobytes() == kf.build(kind).cpu().numpy()[:, :3].tobytes()
    kf.close()
    # an empty kind writes no file; a store of more records than the save's chunk (2^20) goes down in pieces, the second of
    # which begins inside the last keyframe
    rng = np.random.default_rng(51)
    sizes = (600000, 0, 500000)
    assert sum(sizes) > 1 << 20 > sizes[0]
    only = KR.Store(3, (sum(sizes), 1))
    e = [rng.normal(0, 30, (k, 4)).astype(np.float32) for k in sizes]
    assert only.add(e, [np.zeros((0, 4), np.float32)] * 3, poses[:3]) == 0
    kf = _device_store(fx, only)
    os.makedirs(tmp_path / "edge_only")
    assert kf.save(str(tmp_path / "edge_only"), K.stream()) == (True, False)
    assert not os.path.exists(tmp_path / "edge_only" / "surface.pcd")
    assert read_pcd(str(tmp_path / "edge_only" / "edge.pcd"))[:, :3].tobytes() == only.build(KR.EDGE)[:, :3].tobytes()
    kf.close()
