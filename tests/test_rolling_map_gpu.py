"""lfx_rolling_map_* (include/lfx.h) on the device held to tests/rolling_map_restatement.py bit for bit: the insert rule under
contention, the window's moves, the order and the capacity rule of an extraction, the counters, the round trip through PCD
files -- tiny windows, a few seconds in all.  Then lfx_rolling_map_update_batch over a moving 32 x 1024 sensor: its plumbing
bit for bit, its steps against the oracle's optimizer, its trajectory against the ground truth."""
import ctypes as C

import numpy as np
import pytest

from lidar_feature_extraction_amd import RollingMap, read_pcd
from lidar_feature_extraction_amd import binding as LB
from tests.mapping_restatement import pose
from tests.rolling_map_restatement import Store

pytestmark = pytest.mark.gpu

I = np.eye(4)[:3]
BLOCK = 1024                                  # cells a workgroup of the extraction looks at (kRollCells)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _up(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype).copy()).to(_dev())


@pytest.fixture(scope="module")
def fx():
    from lidar_feature_extraction_amd import FeatureExtraction
    f = FeatureExtraction(device=0, max_points_per_scan=1024, max_batch=1, max_points_per_ring=64, max_rings=16)
    yield f
    f.close()


def _rotation(axis_angle):
    th = np.asarray(axis_angle, np.float64)
    k = np.linalg.norm(th)
    if k == 0:
        return np.eye(3)
    u = th / k
    Kx = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + np.sin(k) * Kx + (1 - np.cos(k)) * Kx @ Kx


def _insert(rm, kind, clouds, poses, placed=None, stride=1, gap=3):
    """One lfx_rolling_map_insert call.  placed: the order the clouds lie in memory (default: their own), a gap of `gap`
    records of 7.0 behind each; the counts `stride` words apart."""
    n = len(clouds)
    placed = list(range(n)) if placed is None else list(placed)
    begins, parts, at = [0] * n, [], 0
    for k in placed:
        c = np.asarray(clouds[k], np.float32).reshape(-1, 4)
        begins[k] = at
        parts += [c, np.full((gap, 4), 7.0, np.float32)]
        at += len(c) + gap
    counts = np.full(n * stride, 0xFFFFFFFF, np.uint32)
    counts[::stride] = [len(c) for c in clouds]
    pts = _up(np.concatenate(parts) if at else np.zeros((1, 4), np.float32))
    b, cn = _up(np.array(begins, np.uint32), np.uint32), _up(counts, np.uint32)
    rm.insert(kind, pts.data_ptr(), b.data_ptr(), cn.data_ptr(), stride, n, max(at, 1), np.stack(poses), _stream())
    import torch
    torch.cuda.current_stream().synchronize()


def _same(rm, kind, ref):
    """the device's store equals the restatement: the whole window's records in order, the counters, the live count"""
    lo, hi = ref.window()
    got = rm.extract(kind, lo, hi, _stream())
    want = ref.extract_all()
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
    v = rm.view(_stream())["edge" if kind in (0, "edge") else "surface"]
    assert {k: v[k] for k in ref.counts} == ref.counts
    assert v["live"] == len(want) and v["origin"] == ref.o and v["dims"] == ref.n


def _cloud(rng, n, spread):
    """n records around the origin, a few of them non-finite or far away, random 4th floats"""
    c = np.empty((n, 4), np.float32)
    c[:, :3] = rng.normal(0, 1, (n, 3)) * spread
    c[:, 3] = rng.normal(0, 1, n)
    for value in (np.nan, np.inf, -np.inf, 1e30, 6e5):
        rows = rng.random(n) < 0.01
        c[rows, rng.integers(0, 3)] = value
    return c


@pytest.mark.parametrize("dims", [(4, 4, 2), (8, 8, 4), (5, 3, 2)])
def test_insert_calls_of_every_size(fx, dims):
    """Calls of 0, 1, 255, 256, 257 records and of several clouds into one map, random poses with large angles: after every
    call the window, the four counters and the live count equal the restatement's.  Later calls fall into live voxels: the
    stored bits stay and merged counts them.  The surface store takes the same calls with another leaf."""
    rng = np.random.default_rng(8200 + dims[0])
    rm = RollingMap(fx, edge_leaf=0.5, surface_leaf=0.25, edge_dims=dims, surface_dims=dims)
    ref = dict(edge=Store(0.5, dims), surface=Store(0.25, dims))
    for n in (0, 1, 255, 256, 257, 600):
        for kind in ("edge", "surface"):
            c = _cloud(rng, n, 0.8 * float(ref[kind].leaf) * max(dims) / 2)
            p = pose(_rotation(rng.normal(0, 1.5, 3)), rng.normal(0, 0.3, 3))
            _insert(rm, kind, [c], [p])
            ref[kind].insert([c], [p])
            _same(rm, kind, ref[kind])
    assert ref["edge"].counts["merged"] > 100 and ref["edge"].counts["outside"] > 50 and ref["edge"].counts["nonfinite"] > 10
    rm.close()


def test_the_lowest_rank_wins_under_contention(fx):
    """70 001 records of three clouds into the 256 voxels of an (8, 8, 4) window in one call: every voxel is fought over by
    many workgroups and holds the record of the lowest (cloud, index).  Then the same records in reversed order into a fresh
    map: the ranks follow the new order."""
    rng = np.random.default_rng(8201)
    pts = np.empty((70001, 4), np.float32)
    pts[:, :2] = rng.uniform(-2, 2, (70001, 2))
    pts[:, 2] = rng.uniform(-1, 1, 70001)
    pts[:, 3] = np.arange(70001)
    for records in (pts, pts[::-1].copy()):
        clouds = [records[:30000], records[30000:30001], records[30001:]]
        rm = RollingMap(fx, edge_leaf=0.5, edge_dims=(8, 8, 4), surface_dims=(1, 1, 1))
        ref = Store(0.5, (8, 8, 4))
        _insert(rm, "edge", clouds, [I, I, I], placed=[2, 0, 1])
        ref.insert(clouds, [I, I, I])
        assert ref.counts == dict(inserted=256, merged=70001 - 256, outside=0, nonfinite=0)
        _same(rm, "edge", ref)
        rm.close()


def test_cloud_addressing(fx):
    """Gaps between the clouds, counts 4 words apart, begins in descending order, empty clouds first, in the middle and last:
    the ranks are (cloud index, index in the cloud), not addresses."""
    rng = np.random.default_rng(8202)
    dims = (8, 8, 4)
    sizes = [0, 300, 0, 0, 257, 1, 0, 700, 0]
    clouds = [_cloud(rng, n, 1.2) for n in sizes]
    poses = [pose(_rotation(rng.normal(0, 1.5, 3)), rng.normal(0, 0.3, 3)) for _ in sizes]
    want = Store(0.5, dims)
    want.insert(clouds, poses)
    for placed, stride, gap in ((None, 1, 0), (range(len(sizes))[::-1], 4, 5), (rng.permutation(len(sizes)), 2, 1)):
        rm = RollingMap(fx, edge_leaf=0.5, edge_dims=dims, surface_dims=(1, 1, 1))
        _insert(rm, "edge", clouds, poses, placed=placed, stride=stride, gap=gap)
        _same(rm, "edge", want)
        rm.close()
    # the host form: one cloud a call, the same state as one call of one cloud each
    rm = RollingMap(fx, edge_leaf=0.5, edge_dims=dims, surface_dims=(1, 1, 1))
    for c, p in zip(clouds, poses):
        rm.insert_host("edge", c, p, _stream())
    _same(rm, "edge", want)
    rm.close()


def _centre(c):
    return [c * 0.5 + 0.25, 0.25, 0.25]


def _rec(x, y=0.1, z=0.1, w=1.0):
    return [x, y, z, w]


def test_window_moves(fx):
    """The recentring cases of tests/test_rolling_map_expect.py on the device, with inserts between them: by 1, N - 1, N, past
    N, back (every voxel reappears), a stale slot overwritten, back again (the voxel whose slot was taken does not)."""
    rm = RollingMap(fx, edge_leaf=0.5, surface_leaf=0.5, edge_dims=(4, 1, 1), surface_dims=(5, 3, 2))
    ref = Store(0.5, (4, 1, 1))
    other = Store(0.5, (5, 3, 2))
    pts = np.array([_rec(0.5 * v + 0.1, w=float(v)) for v in (-2, -1, 0, 1)], np.float32)
    rng = np.random.default_rng(8203)
    _insert(rm, "edge", [pts], [I])
    ref.insert([pts], [I])
    _same(rm, "edge", ref)
    live = []
    for c in (1, 3, 4, 9, 0):
        rm.recenter(_centre(c))
        ref.recenter(_centre(c))
        other.recenter(_centre(c))
        _same(rm, "edge", ref)
        live.append(len(ref.extract_all()))
        # the (5, 3, 2) store follows the same centres with inserts of its own between the moves: negative origins, stale slots
        c5 = _cloud(rng, 200, 1.0) + np.array(_centre(c) + [0.0], np.float32)
        _insert(rm, "surface", [c5], [I])
        other.insert([c5], [I])
        _same(rm, "surface", other)
    assert live == [3, 1, 0, 0, 4]
    rm.recenter(_centre(4))
    ref.recenter(_centre(4))
    taker = np.array([_rec(0.5 * 2 + 0.1, w=20.0)], np.float32)
    _insert(rm, "edge", [taker], [I])
    ref.insert([taker], [I])
    _same(rm, "edge", ref)
    rm.recenter(_centre(0))
    ref.recenter(_centre(0))
    _same(rm, "edge", ref)
    assert ref.extract_all()[:, 3].tolist() == [-1.0, 0.0, 1.0]
    _insert(rm, "edge", [pts], [I])
    ref.insert([pts], [I])
    _same(rm, "edge", ref)
    assert ref.counts == dict(inserted=6, merged=3, outside=0, nonfinite=0)
    assert other.counts["outside"] > 0 and other.counts["merged"] > 0
    rm.close()


def _extract_with_canary(rm, kind, lo, hi, capacity):
    import torch
    out = torch.full((capacity + 4, 4), -77.0, dtype=torch.float32, device=_dev())
    n = rm.extract_device(kind, lo, hi, out.data_ptr(), capacity, _stream())
    torch.cuda.current_stream().synchronize()
    return n, out.cpu().numpy()


def test_extract_boxes_and_capacities(fx):
    """The whole window, a box partly outside, an empty box, a one-voxel box, hi < lo, a box far outside; every capacity
    around the need: the count is the full need and nothing at or past the capacity is written."""
    rng = np.random.default_rng(8204)
    dims = (8, 8, 4)
    rm = RollingMap(fx, edge_leaf=0.5, edge_dims=dims, surface_dims=(1, 1, 1))
    ref = Store(0.5, dims)
    c = _cloud(rng, 150, 1.0)
    _insert(rm, "edge", [c], [I])
    ref.insert([c], [I])
    one = ref.extract_all()[5, :3]
    v = np.floor(one * 2) / 2
    boxes = [ref.window(), ([-0.7, -0.2, -9.0], [9.0, 0.9, 0.3]), ([-100.0] * 3, [100.0] * 3), ([-1e300] * 3, [1e300] * 3),
             (list(v), list(v + 0.49)), ([0.9, 0.9, 0.4], [-0.9, 1.5, 0.45]), ([50.0] * 3, [60.0] * 3),
             ([-0.5, -0.5, 0.0], [-0.5, -0.5, 0.0])]
    sizes = []
    for lo, hi in boxes:
        want = ref.extract(lo, hi)
        got = rm.extract("edge", lo, hi, _stream())
        assert got.tobytes() == want.tobytes()
        sizes.append(len(want))
    assert sizes[0] == sizes[2] == sizes[3] > 40 and 0 < sizes[1] < sizes[0] and sizes[4] == 1 and sizes[5] == sizes[6] == 0
    lo, hi = boxes[1]
    want = ref.extract(lo, hi)
    need = len(want)
    for capacity in (0, 1, need - 1, need, need + 1):
        n, out = _extract_with_canary(rm, "edge", lo, hi, capacity)
        assert n == need
        k = min(capacity, need)
        assert out[:k].tobytes() == want[:k].tobytes()
        assert (out[k:] == -77.0).all()
    rm.close()


def test_extract_compaction_across_blocks(fx):
    """A (64, 64, 16) window about half full, so the compaction crosses its scan's block boundaries (64 workgroups of 1 024
    cells), and live counts of 0, 1 and a block's cells - 1, + 0, + 1 in a window of several blocks."""
    rng = np.random.default_rng(8205)
    dims = (64, 64, 16)
    rm = RollingMap(fx, edge_leaf=0.5, surface_leaf=0.5, edge_dims=dims, surface_dims=(32, 16, 8))
    ref = Store(0.5, dims)
    cells = rng.permutation(64 * 64 * 16)[:64 * 64 * 8]
    v = np.stack([cells % 64 - 32, (cells // 64) % 64 - 32, cells // 4096 - 8], axis=1)
    c = np.hstack([(v + rng.uniform(0.1, 0.9, v.shape)) * 0.5, rng.normal(0, 1, (len(v), 1))]).astype(np.float32)
    _insert(rm, "edge", [c], [I])
    ref.insert([c], [I])
    assert ref.counts["inserted"] == 64 * 64 * 8
    _same(rm, "edge", ref)
    lo, hi = [-7.3, -15.9, -2.2], [11.1, 3.3, 3.9]       # a box whose rows are no multiple of anything
    assert rm.extract("edge", lo, hi, _stream()).tobytes() == ref.extract(lo, hi).tobytes()
    small = Store(0.5, (32, 16, 8))           # 4 096 cells: 4 workgroups
    _same(rm, "surface", small)               # 0 live
    at = 0
    for live in (1, BLOCK - 1, BLOCK, BLOCK + 1):
        cells = np.arange(at, live) * 3 % 4096            # (3 is a unit modulo 4 096: distinct cells, spread over the blocks)
        v = np.stack([cells % 32 - 16, (cells // 32) % 16 - 8, cells // 512 - 4], axis=1)
        c = np.hstack([(v + 0.5) * 0.5, np.arange(at, live)[:, None]]).astype(np.float32)
        _insert(rm, "surface", [c], [I])
        small.insert([c], [I])
        assert small.counts["inserted"] == live
        _same(rm, "surface", small)
        at = live
    rm.close()


def test_save_and_seed_from_files(fx, tmp_path):
    """Save -> read_pcd -> insert_host at the identity into a fresh map of the same leaves reproduces both windows: a stored
    point is its own voxel's representative.  (A PCD file holds x, y, z: the 4th float is 1 on both sides.)  An empty store
    writes no file."""
    rng = np.random.default_rng(8206)
    cfg = dict(edge_leaf=0.2, surface_leaf=0.4, edge_dims=(16, 12, 6), surface_dims=(9, 7, 5))
    rm = RollingMap(fx, **cfg)
    assert rm.save(str(tmp_path), _stream()) == (False, False) and not (tmp_path / "edge.pcd").exists()
    clouds = {}
    for kind, spread in (("edge", 1.2), ("surface", 1.4)):
        c = _cloud(rng, 900, spread)
        c[:, 3] = 1.0
        p = pose(_rotation(rng.normal(0, 1.5, 3)), rng.normal(0, 0.2, 3))
        _insert(rm, kind, [c], [p])
        clouds[kind] = (c, p)
    assert rm.save(str(tmp_path), _stream()) == (True, True)
    seeded = RollingMap(fx, **cfg)
    for kind in ("edge", "surface"):
        ref = Store(cfg[kind + "_leaf"], cfg[kind + "_dims"])
        ref.insert([clouds[kind][0]], [clouds[kind][1]])
        want = ref.extract_all()
        assert len(want) > 100
        file = read_pcd(str(tmp_path / (kind + ".pcd")))
        assert file.tobytes() == want.tobytes()
        seeded.insert_host(kind, file, None, _stream())
        lo, hi = ref.window()
        assert seeded.extract(kind, lo, hi, _stream()).tobytes() == want.tobytes()
        assert seeded.view(_stream())[kind]["inserted"] == len(want)
    rm.close(); seeded.close()


def test_validation_before_any_device_work(fx):
    L, ctx = fx._L, fx._ctx
    bad = LB.ERR_INVALID_ARGUMENT
    for config in (dict(edge_leaf=0.0), dict(surface_leaf=-1.0), dict(edge_leaf=float("nan")), dict(surface_leaf=float("inf")),
                   dict(edge_dims=(0, 4, 4)), dict(surface_dims=(4, 4, 0)), dict(edge_dims=(2048, 2048, 513)),
                   dict(edge_dims=(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF))):
        with pytest.raises(LB.LfxError) as e:
            RollingMap(fx, **config)
        assert e.value.code == bad
    rm = RollingMap(fx, edge_leaf=0.5, edge_dims=(4, 4, 2), surface_dims=(4, 4, 2))
    before = rm.view(_stream())
    pts = _up(np.zeros((16, 4), np.float32))
    b, n = _up(np.array([4], np.uint32), np.uint32), _up(np.array([5], np.uint32), np.uint32)
    nan_pose = I.copy()
    nan_pose[1, 2] = np.nan
    pd = C.POINTER(C.c_double)

    def insert(kind=0, points=pts.data_ptr(), begin=b.data_ptr(), count=n.data_ptr(), stride=1, clouds=1, total=8, p=I):
        pm = np.ascontiguousarray(p, np.float64)
        return L.lfx_rolling_map_insert(ctx, rm.handle, kind, C.c_void_p(points), C.c_void_p(begin), C.c_void_p(count), stride, clouds,
                                        total, pm.ctypes.data_as(pd), C.c_void_p(_stream()))

    assert insert(kind=2) == bad and insert(kind=-1) == bad
    assert insert(points=0) == bad and insert(begin=0) == bad and insert(count=0) == bad
    assert insert(stride=0) == bad and insert(clouds=0) == bad
    assert insert(p=nan_pose) == bad
    assert insert() == bad and b"past total_points" in L.lfx_last_error(ctx)       # records 4 + 5 > 8
    assert insert(total=9) == 0
    host = np.zeros((2, 4), np.float32)
    assert L.lfx_rolling_map_insert_host(ctx, rm.handle, 3, C.c_void_p(host.ctypes.data), 2, I.ctypes.data_as(pd), None) == bad
    assert L.lfx_rolling_map_insert_host(ctx, rm.handle, 0, None, 2, I.ctypes.data_as(pd), None) == bad
    assert L.lfx_rolling_map_insert_host(ctx, rm.handle, 0, C.c_void_p(host.ctypes.data), 2, nan_pose.ctypes.data_as(pd), None) == bad
    lo, hi, cnt = np.zeros(3), np.ones(3), C.c_uint64(99)
    bad_lo = np.array([0.0, np.nan, 0.0])

    def extract(kind=0, lo_=lo, out=None, capacity=0, count=C.byref(cnt)):
        return L.lfx_rolling_map_extract(ctx, rm.handle, kind, lo_.ctypes.data_as(pd), hi.ctypes.data_as(pd), out, capacity, count, None)

    assert extract(kind=5) == bad and extract(lo_=bad_lo) == bad and extract(capacity=3) == bad and extract(count=None) == bad
    assert extract() == 0 and cnt.value == 1
    for centre in ([np.nan, 0, 0], [0, np.inf, 0], [0, 0, 1e9]):
        with pytest.raises(LB.LfxError):
            rm.recenter(centre)
    after = rm.view(_stream())
    assert after["edge"]["origin"] == before["edge"]["origin"] == (-2, -2, -1)
    assert after["edge"]["inserted"] == 1 and after["edge"]["merged"] == 4 and after["surface"] == before["surface"]
    rm.close()


# ---------------------------------------------------------------------------- lfx_rolling_map_update_batch
K, MAX_ITER = 15, 20
RINGS, COLS, SEED = 32, 1024, 8100
# test_loop_against_the_ground_truth: twice what the CPU voxel chain (the restatement over the oracle's extraction and
# Optimizer::Run) measures on the 24 scans, 0.03798 m and 0.009358 rad
BOUND_T, BOUND_R = 0.076, 0.0187


def _big_fx(batch):
    from lidar_feature_extraction_amd import FeatureExtraction
    return FeatureExtraction(device=0, max_points_per_scan=RINGS * COLS, max_batch=batch, max_points_per_ring=COLS, max_rings=RINGS)


def _extract(fx, clouds):
    from lidar_feature_extraction_amd import concat
    import torch
    d = torch.from_numpy(concat(clouds).view(np.uint8).copy()).to(_dev())
    fx.extract_batch_device(d.data_ptr(), [len(c) for c in clouds], _stream())
    return d, [fx.download(s, _stream()) for s in range(len(clouds))]


def _whole(rm, kind):
    v = rm.view(_stream())[kind]
    leaf = float(v["leaf"])
    lo = [(v["origin"][a] + 0.5) * leaf for a in range(3)]
    hi = [(v["origin"][a] + v["dims"][a] - 0.5) * leaf for a in range(3)]
    return rm.extract(kind, lo, hi, _stream())


@pytest.fixture(scope="module")
def run24():
    """24 scans of the moving 32 x 1024 sensor through one update_batch at the default config, no odometry: the device's
    results, its two stores extracted whole, the scans as the device extracted them."""
    from lidar_feature_extraction_amd import make_sequence
    clouds, truth = make_sequence(24, RINGS, COLS, seed=SEED)
    fx = _big_fx(24)
    d, got = _extract(fx, clouds)
    rm = fx.rolling_map()
    res = rm.update_batch(None, 24, _stream())
    out = dict(clouds=clouds, truth=truth, got=got, res=res, edge=_whole(rm, "edge"), surface=_whole(rm, "surface"),
               view=rm.view(_stream()), pose=rm.pose())
    rm.close()
    fx.close()
    return out


def _bits(r):
    return (r["pose"].tobytes(), r["initial_pose"].tobytes(), r["error"], r["error_scale"], r["iteration"], r["code"], r["aligned"],
            r["inserted"], r["recentered"], r["n_edge_map"], r["n_surface_map"])


def _replay(result):
    return lambda edge_box, surface_box, scan, initial: dict(pose=result["pose"], code=result["code"], success=result["success"])


def test_loop_plumbing_bit_for_bit(run24):
    """The restatement's loop fed the device's own results: at every scan the same decision (aligned, inserted, recentred),
    the same initial pose bits and box sizes.  For the aligned ones of the first 12 scans the alignment of lfx_localize_host
    (the Downsample and lfx_scan_to_map_align's optimizer) on maps made from the restatement's two boxes, from the reported
    initial pose, gives the same pose bits, error, scale, iteration and code: both searches are exact and break ties by
    index, so the grids cannot matter.  After the batch the two stores extracted whole equal the restatement's."""
    from tests.rolling_map_restatement import RollingMap as Restated
    got, res = run24["got"], run24["res"]
    ref = Restated()
    fx = _big_fx(1)
    aligned = 0
    for k in range(24):
        scan = (got[k].edge_points, got[k].surface_points)
        r = ref.update(scan, _replay(res[k]))
        g = res[k]
        assert (r["aligned"], r["inserted"], r["recentered"]) == (g["aligned"], g["inserted"], g["recentered"]), (k, g)
        assert (r["n_edge_map"], r["n_surface_map"]) == (g["n_edge_map"], g["n_surface_map"]), (k, g)
        assert r["initial_pose"].tobytes() == g["initial_pose"].tobytes()
        if not g["aligned"]:
            assert (g["code"], g["iteration"]) == (6, 0) and g["pose"].tobytes() == g["initial_pose"].tobytes()
        elif k < 12:
            emap, smap = fx.make_map_from_host(r["edge_box"], 1.0, _stream()), fx.make_map_from_host(r["surface_box"], 1.0, _stream())
            a = fx.localize_host(emap, smap, scan[0], scan[1], g["initial_pose"], K, MAX_ITER, 1.0, _stream())
            assert a["pose"].tobytes() == g["pose"].tobytes(), (k, a, g)
            assert (a["error"], a["error_scale"], a["iteration"], a["code"]) == (g["error"], g["error_scale"], g["iteration"], g["code"]), (k, a, g)
            emap.close(); smap.close()
            aligned += 1
    fx.close()
    assert aligned == 11 and not res[0]["aligned"] and all(r["inserted"] for r in res)
    assert run24["edge"].tobytes() == ref.stores["edge"].extract_all().tobytes()
    assert run24["surface"].tobytes() == ref.stores["surface"].extract_all().tobytes()
    for kind in ("edge", "surface"):
        assert {c: run24["view"][kind][c] for c in ref.stores[kind].counts} == ref.stores[kind].counts
    assert run24["pose"].tobytes() == res[-1]["pose"].tobytes() == run24["view"]["pose"].tobytes()
    assert run24["view"]["correction"].tobytes() == np.eye(4)[:3].tobytes()


def test_loop_step_parity_against_the_oracle(run24):
    """As tests/test_odometry_gpu.py::test_step_parity_against_the_oracle, with its tolerances: at every aligned step of the
    first 12 scans the oracle's Optimizer::Run on the two boxes the scan met, its edge cloud, its downsampled surface cloud
    and the reported initial pose agrees with the device's alignment."""
    from oracle import binding as OB
    from tests.odometry_restatement import downsample, optimize_scan
    from tests.rolling_map_restatement import RollingMap as Restated
    got, res = run24["got"], run24["res"]
    want = [OB.extract(c, canonical_ties=False) for c in run24["clouds"][:12]]
    ref = Restated()
    for k in range(12):
        assert np.array_equal(got[k].edge_points[:, :3], want[k]["edge_points"][:, :3])
        assert np.array_equal(got[k].surface_points[:, :3], want[k]["surface_points"][:, :3])
        r = ref.update((got[k].edge_points, got[k].surface_points), _replay(res[k]))
        if not res[k]["aligned"]:
            continue
        g = res[k]
        w = optimize_scan(r["edge_box"], r["surface_box"], K, want[k]["edge_points"], downsample(want[k]["surface_points"], 1.0),
                          g["initial_pose"], MAX_ITER)
        if (g["code"], g["iteration"]) != (w["code"], w["iteration"]):
            assert abs(g["iteration"] - w["iteration"]) <= 1, (k, g, w)
            assert np.abs(g["pose"] - w["pose"]).max() < 2e-3, (k, g, w)
        else:
            assert np.abs(g["pose"] - w["pose"]).max() <= 1e-6 * (1 + np.abs(w["pose"]).max()), (k, g["pose"], w["pose"])
            assert abs(g["error"] - w["error"]) <= 1e-5 * abs(w["error"]) + 1e-18, (k, g["error"], w["error"])
            assert abs(g["error_scale"] - w["error_scale"]) <= 1e-5 * abs(w["error_scale"]) + 1e-18, k
        assert g["success"] == w["success"], (k, g, w)


def test_loop_against_the_ground_truth(run24):
    """24 scans.  The CPU voxel chain (the restatement's loop over the oracle's extraction, Downsample and Optimizer::Run)
    measures a worst error of 0.03798 m and 0.009358 rad against the synthetic ground truth; the device's trajectory and that
    chain both stay under twice that (0.076 m, 0.0187 rad: test_trajectory_against_the_ground_truth's rule).  The feature's
    claim: the CPU voxel chain is no worse than the 7-scan window's chain (oracle_chain: 0.06053 m, 0.01065 rad) on the same
    scans."""
    from oracle import binding as OB
    from tests.odometry_restatement import oracle_chain, trajectory_error
    from tests.rolling_map_restatement import RollingMap as Restated, oracle_align
    truth = run24["truth"]
    dt, dr = trajectory_error([r["pose"] for r in run24["res"]], truth)
    print("device: %.5f m %.6f rad" % (dt, dr))
    ref, align = Restated(), oracle_align(K, MAX_ITER, 1.0)
    chain = []
    for c in run24["clouds"]:
        s = OB.extract(c, canonical_ties=False)
        chain.append(ref.update((s["edge_points"], s["surface_points"]), align)["pose"])
    ct, cr = trajectory_error(chain, truth)
    ot, orr = trajectory_error(oracle_chain(run24["clouds"]), truth)
    print("CPU voxel chain: %.5f m %.6f rad; 7-scan window: %.5f m %.6f rad" % (ct, cr, ot, orr))
    assert dt < BOUND_T and dr < BOUND_R, (dt, dr)
    assert ct < BOUND_T and cr < BOUND_R, (ct, cr)
    assert ct <= ot and cr <= orr, (ct, cr, ot, orr)


def test_loop_batch_splitting_chaining_and_a_forced_failure(run24):
    """The same bits come out of one batch, batches of 4 and batches of 1 (8 scans), without odometry poses and with the poses
    of a real Odometry run over the same scans; with them the correction is pose x odom^-1 of the last scan, in the
    restatement's arithmetic.  A forced failure -- max_iter 1 from a start 3 m off, which ends in LFX_ALIGN_MAX_ITERATION on
    the CPU chain too -- inserts nothing and carries the initial pose."""
    from tests.rolling_map_restatement import compose, inverse
    n = 8
    clouds = run24["clouds"][:n]

    def by_batches(size, chained, **config):
        fx = _big_fx(size)
        rm, odo = fx.rolling_map(**config), fx.odometry()
        out, odom = [], []
        for a in range(0, n, size):
            d, _ = _extract(fx, clouds[a:a + size])
            poses = None
            if chained:
                poses = np.stack([r["pose"] for r in odo.update_batch(len(clouds[a:a + size]), _stream())])
                odom += list(poses)
            out += rm.update_batch(poses, len(clouds[a:a + size]), _stream())
        state = (_whole(rm, "edge").tobytes(), _whole(rm, "surface").tobytes(), rm.view(_stream())["correction"])
        rm.close(); odo.close(); fx.close()
        return out, odom, state

    for chained in (False, True):
        whole, odom, state = by_batches(n, chained)
        if not chained:
            assert [_bits(r) for r in whole] == [_bits(r) for r in run24["res"][:n]]
        else:
            assert whole[0]["initial_pose"].tobytes() == odom[0].tobytes()
            assert state[2].tobytes() == compose(whole[-1]["pose"], inverse(odom[-1])).tobytes()
            assert whole[3]["initial_pose"].tobytes() == compose(compose(whole[2]["pose"], inverse(odom[2])), odom[3]).tobytes()
        assert sum(r["aligned"] for r in whole) == n - 1 and all(r["inserted"] for r in whole)
        for size in (4, 1):
            other, _, other_state = by_batches(size, chained)
            assert [_bits(r) for r in other] == [_bits(r) for r in whole], (chained, size)
            assert other_state[:2] == state[:2] and other_state[2].tobytes() == state[2].tobytes()
    # the forced failure
    fx = _big_fx(1)
    rm = fx.rolling_map(max_iter=1)
    d, _ = _extract(fx, clouds[:1])
    first = rm.update_batch(None, 1, _stream())[0]
    assert not first["aligned"] and first["inserted"]
    before = rm.view(_stream())
    off = np.eye(4)[:3].copy()
    off[0, 3] = 3.0
    d, _ = _extract(fx, clouds[1:2])
    r = rm.update_batch(off[None], 1, _stream())[0]
    assert (r["aligned"], r["code"], r["success"], r["inserted"]) == (True, 3, False, False), r
    after = rm.view(_stream())
    assert r["initial_pose"].tobytes() == off.tobytes() and rm.pose().tobytes() == off.tobytes()
    assert after["correction"].tobytes() == np.eye(4)[:3].tobytes()
    assert after["edge"] == before["edge"] and after["surface"] == before["surface"]
    rm.close(); fx.close()


def test_loop_leaves_the_batch_alone_and_validates():
    """After update_batch the batch's downloads and its device view hold the same bits as before (as
    test_no_side_effects_on_the_batch checks for the odometry).  n_scans other than the batch's, null results, non-finite
    odometry poses and bad settings are refused before any device work."""
    from lidar_feature_extraction_amd import make_sequence
    n = 3
    clouds, _ = make_sequence(n, RINGS, COLS, seed=8600)
    fx = _big_fx(n)
    rm = fx.rolling_map()
    with pytest.raises(LB.LfxError, match="no batch"):
        rm.update_batch(None, 1, _stream())
    d, _ = _extract(fx, clouds)

    def snapshot():
        import torch
        dl = [fx.download(s, _stream()) for s in range(n)]
        v = fx.device_view()
        total = sum(len(c) for c in clouds)
        torch.cuda.synchronize()
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        out = [np.zeros((total, 4), np.float32), np.zeros((total, 4), np.float32), np.zeros(4 * n, np.uint32)]
        for a, p in zip(out, (v.edge_points, v.surface_points, v.scan_info)):
            assert hip.hipMemcpy(a.ctypes.data, int(p), a.nbytes, 2) == 0
        return dl, [a.tobytes() for a in out]
    before = snapshot()
    for bad in (1, 4):
        with pytest.raises(LB.LfxError, match="n_scans"):
            rm.update_batch(None, bad, _stream())
    poses = np.stack([np.eye(4)[:3]] * n)
    poses[1, 0, 0] = np.nan
    with pytest.raises(LB.LfxError, match="finite"):
        rm.update_batch(poses, n, _stream())
    assert fx._L.lfx_rolling_map_update_batch(fx._ctx, rm.handle, n, None, None, None) == LB.ERR_INVALID_ARGUMENT
    assert rm.view(_stream())["edge"]["inserted"] == 0
    res = rm.update_batch(None, n, _stream())
    assert sum(r["aligned"] for r in res) == n - 1
    after = snapshot()
    for a, b in zip(before[0], after[0]):
        for f in ("labels", "curvature", "edge_index", "surface_index", "edge_points", "surface_points"):
            assert np.asarray(getattr(a, f)).tobytes() == np.asarray(getattr(b, f)).tobytes(), f
    assert before[1] == after[1]
    for bad in (dict(n_neighbors=2), dict(n_neighbors=17), dict(max_iter=0), dict(scan_surface_leaf=0.0), dict(edge_cell=-1.0),
                dict(match_half_extent=(1.0, -1.0, 1.0)), dict(initial_pose=np.full((3, 4), np.nan))):
        with pytest.raises(LB.LfxError):
            fx.rolling_map(**bad)
    with pytest.raises(TypeError):
        fx.rolling_map(n_neighbours=15)
    rm.close(); fx.close()
