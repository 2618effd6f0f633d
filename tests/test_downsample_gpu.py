"""lfx_voxel_downsample / lfx_downsample_surface (Downsample = pcl::VoxelGrid, downsample.hpp:37-51, applied
to scan_surface at localization/.../surface.hpp:111) against the oracle's restatement of the PCL algorithm, bit for bit
(both sum the points of a cell in input order).  Parity with PCL itself is unpinned: see oracle/lfx_oracle.h."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _oracle(cloud, leaf):
    from oracle import binding as OB
    L = OB.lib()
    cloud = np.ascontiguousarray(cloud, np.float32)
    out = np.zeros_like(cloud)
    n = C.c_int(0)
    rc = L.orc_voxel_downsample(OB.ptr(cloud, C.POINTER(C.c_float)), len(cloud), leaf, OB.ptr(out, C.POINTER(C.c_float)), C.byref(n))
    return rc, out[:n.value].copy()


def test_voxel_downsample_random_clouds():
    import torch
    from lidar_feature_extraction_amd import FeatureExtraction
    rng = np.random.default_rng(11)
    sizes = [1, 2, 0, 777, 5000, 40000, 3, 1025, 130000]
    clouds = []
    for k, n in enumerate(sizes):
        c = np.ones((n, 4), np.float32)
        scale = [3.0, 30.0, 120.0][k % 3]
        c[:, :3] = (rng.standard_normal((n, 3)) * scale).astype(np.float32)
        c[:, 2] *= 0.1
        clouds.append(c)
    clouds.append(np.array([[0, 0, 0, 1], [4000, 4000, 4000, 1]], np.float32))       # leaf too small for this one
    begin = np.zeros(len(clouds), np.uint32)
    begin[1:] = np.cumsum([len(c) for c in clouds])[:-1]
    count = np.array([len(c) for c in clouds], np.uint32)
    total = int(count.sum())
    dev = torch.device("cuda", 0)
    d_pts = torch.from_numpy(np.concatenate(clouds)).to(dev)
    d_begin = torch.from_numpy(begin.astype(np.int32)).to(dev)
    d_count = torch.from_numpy(count.astype(np.int32)).to(dev)
    d_out = torch.zeros((total, 4), dtype=torch.float32, device=dev)
    d_n = torch.zeros(len(clouds), dtype=torch.int32, device=dev)
    d_st = torch.zeros(len(clouds), dtype=torch.int32, device=dev)
    fx = FeatureExtraction(device=0, max_points_per_scan=1024, max_batch=1)
    stream = torch.cuda.current_stream().cuda_stream
    for leaf in (1.0, 0.25, 0.01):
        fx.voxel_downsample(d_pts.data_ptr(), d_begin.data_ptr(), d_count.data_ptr(), 1, len(clouds), total, leaf, d_out.data_ptr(),
                            d_n.data_ptr(), d_st.data_ptr(), stream)
        torch.cuda.synchronize()
        out, n_out, st = d_out.cpu().numpy(), d_n.cpu().numpy(), d_st.cpu().numpy()
        for k, c in enumerate(clouds):
            rc, want = _oracle(c, leaf)
            assert st[k] == rc, (leaf, k)
            if rc == 0:
                assert n_out[k] == len(want), (leaf, k, n_out[k], len(want))
                assert out[begin[k]:begin[k] + len(want)].tobytes() == want.tobytes(), (leaf, k)
    fx.close()


def test_downsample_of_the_surface_clouds_of_a_batch():
    """The localizer's use: Downsample(scan_surface, 1.0) (surface.hpp:111), chained on the device behind the extraction."""
    import torch
    from lidar_feature_extraction_amd import FeatureExtraction, make_scan, concat
    from oracle import binding as OB
    rings, cols = 32, 1024
    clouds = [make_scan(rings, cols, seed=6100 + k, drop_fraction=(0.1 if k == 2 else 0.0)) for k in range(4)]
    dev = torch.device("cuda", 0)
    fx = FeatureExtraction(device=0, max_points_per_scan=rings * cols, max_batch=4, max_points_per_ring=cols, max_rings=rings)
    d = torch.from_numpy(concat(clouds).view(np.uint8).copy()).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    fx.extract_batch_device(d.data_ptr(), [len(c) for c in clouds], stream)
    total = sum(len(c) for c in clouds)
    d_out = torch.zeros((total, 4), dtype=torch.float32, device=dev)
    d_n = torch.zeros(4, dtype=torch.int32, device=dev)
    d_st = torch.zeros(4, dtype=torch.int32, device=dev)
    fx.downsample_surface(1.0, d_out.data_ptr(), d_n.data_ptr(), d_st.data_ptr(), stream)
    torch.cuda.synchronize()
    out, n_out = d_out.cpu().numpy(), d_n.cpu().numpy()
    at = 0
    for k, c in enumerate(clouds):
        w = OB.extract(c, canonical_ties=False)
        surf = w["surface_points"].copy()
        rc, want = _oracle(surf, 1.0)
        assert rc == 0 and n_out[k] == len(want) and 0 < len(want) < len(surf)
        assert out[at:at + len(want)].tobytes() == want.tobytes(), k
        at += len(c)
    fx.close()


# ------------------------------------------------------------------------------------ edges (tests/downsample_cases.py)
SENTINEL = 0x7FA5A5A5                        # a NaN no centroid has: whatever the kernel does not write keeps it


@pytest.fixture(scope="module")
def fx():
    from lidar_feature_extraction_amd import FeatureExtraction
    f = FeatureExtraction(device=0, max_points_per_scan=1024, max_batch=1)
    yield f
    f.close()


def _run(fx, clouds, leaf, count_stride=1, total=None):
    """One lfx_voxel_downsample call over the clouds, back to back; d_out prefilled with SENTINEL.  -> out (records),
    out_count, status, begin."""
    import torch
    lens = np.array([len(c) for c in clouds], np.int64)
    begin = np.zeros(len(clouds), np.uint32)
    begin[1:] = np.cumsum(lens)[:-1]
    total = int(total if total is not None else max(1, lens.sum()))
    pts = np.zeros((total, 4), np.float32)
    for c, b in zip(clouds, begin):
        pts[b:b + len(c)] = c
    count = np.full(len(clouds) * count_stride, 0x00FFFFFF, np.uint32)      # the slots between counts are not counts
    count[::count_stride] = lens
    dev = torch.device("cuda", 0)
    d_pts = torch.from_numpy(pts).to(dev)
    d_begin = torch.from_numpy(begin.view(np.int32)).to(dev)
    d_count = torch.from_numpy(count.view(np.int32)).to(dev)
    d_out = torch.from_numpy(np.full((total, 4), SENTINEL, np.uint32).view(np.int32)).to(dev)
    d_n = torch.full((len(clouds),), -1, dtype=torch.int32, device=dev)
    d_st = torch.full((len(clouds),), -1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    fx.voxel_downsample(d_pts.data_ptr(), d_begin.data_ptr(), d_count.data_ptr(), count_stride, len(clouds), total, leaf,
                        d_out.data_ptr(), d_n.data_ptr(), d_st.data_ptr(), stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.float32), d_n.cpu().numpy(), d_st.cpu().numpy(), begin


def _check_against_oracle(names, clouds, leaf, out, n_out, st, begin):
    from tests import downsample_cases as D
    for name, c, n, s, b in zip(names, clouds, n_out, st, begin):
        rc, want = D.oracle(c, leaf)
        assert (s, n) == (rc, len(want)), (name, leaf, s, n, rc, len(want))
        region = out[b:b + len(c)]
        assert region[:len(want)].tobytes() == want.tobytes(), (name, leaf)
        assert (region[len(want):].view(np.uint32) == SENTINEL).all(), ("written past the centroids", name, leaf)


def test_voxel_downsample_edge_clouds(fx):
    """Every edge cloud (limits of "leaf too small", cell boundaries, far coordinates, n around 1 024 and 12 288, 2 046 to
    2 049 cells, largest keys at the radix byte boundaries, non-finite points) against the oracle: status, count and
    centroid bytes, and nothing written past the centroids (a status-1 cloud's records untouched).  One launch per leaf."""
    from tests import downsample_cases as D
    by_leaf = {}
    for name, c, leaf in D.all_cases():
        by_leaf.setdefault(leaf, []).append((name, c))
    assert len(by_leaf) > 5
    for leaf, cases in by_leaf.items():
        names, clouds = [n for n, _ in cases], [c for _, c in cases]
        _check_against_oracle(names, clouds, leaf, *_run(fx, clouds, leaf))


def test_voxel_downsample_skips_non_finite_points(fx):
    """Non-finite points inserted anywhere leave the kernel's output byte for byte as it was without them, in both forms."""
    from tests import downsample_cases as D
    rng = np.random.default_rng(31)
    clean = [D.cloud(rng.normal(0, 4, (n, 3))) for n in (1, 64, 1500, 12000, 12288, 20000)]
    dirty = [D.insert_nonfinite(rng, c, k) for c, k in zip(clean, (3, 1, 40, 288, 1, 500))]
    assert len(dirty[3]) == 12288 and len(dirty[4]) == 12289     # the dirty clouds straddle the form switch
    out0, n0, st0, b0 = _run(fx, clean, 0.5)
    out1, n1, st1, b1 = _run(fx, dirty, 0.5)
    assert (st0 == 0).all() and (st1 == 0).all() and (n0 == n1).all()
    for k in range(len(clean)):
        assert out0[b0[k]:b0[k] + n0[k]].tobytes() == out1[b1[k]:b1[k] + n1[k]].tobytes(), k
    _check_against_oracle(range(len(dirty)), dirty, 0.5, out1, n1, st1, b1)


def test_voxel_downsample_batch_interplay():
    """One batch mixing status 0 and 1, empty clouds and both forms, counts at count_stride 4; then calls with a larger
    total_points (the sort scratch grows) and a smaller one again, on one context."""
    from lidar_feature_extraction_amd import FeatureExtraction
    from tests import downsample_cases as D
    rng = np.random.default_rng(37)
    far = D.cloud([[0, 0, 0], [4000, 4000, 4000]])
    mixed = [D.cloud(rng.normal(0, 5, (700, 3))), far, np.zeros((0, 4), np.float32), D.cloud(rng.normal(0, 20, (15000, 3))),
             far, D.cloud(rng.normal(0, 5, (12288, 3))), np.zeros((0, 4), np.float32), D.cloud([[1, 2, 3]]),
             D.cloud(np.full((5, 3), np.nan))]
    f = FeatureExtraction(device=0, max_points_per_scan=1024, max_batch=1)
    try:
        for clouds, stride, leaf in ((mixed[:2], 4, 0.001), (mixed, 4, 0.001), (mixed + mixed, 1, 0.5), (mixed[:3], 4, 0.5),
                                     (mixed[5:6], 1, 0.25)):
            out, n_out, st, begin = _run(f, clouds, leaf, count_stride=stride)
            _check_against_oracle(range(len(clouds)), clouds, leaf, out, n_out, st, begin)
        # total_points larger than the clouds need
        out, n_out, st, begin = _run(f, mixed, 1.0, total=200000)
        _check_against_oracle(range(len(mixed)), mixed, 1.0, out, n_out, st, begin)
    finally:
        f.close()


def test_voxel_downsample_against_float64(fx):
    """Independent of the oracle: one centroid per distinct float32 cell, in ascending cell index, each within a
    count-scaled rounding bound of the float64 mean of its members; both forms, heads in LDS and in memory."""
    from tests import downsample_cases as D
    rng = np.random.default_rng(41)
    cases = [(D.cloud(rng.normal(0, 8, (4000, 3))), 0.3), (D.cloud(rng.uniform(-50, 50, (13000, 3))), 2.0),
             (D.cloud(rng.uniform(2.0, 2.9, (12288, 3))), 1.0), (D.cloud(1.0e5 + rng.normal(0, 0.5, (2000, 3))), 0.01),
             (D.cloud(rng.uniform(-30, 30, (12000, 3))), 1.0)]
    for cloud, leaf in cases:
        out, n_out, st, begin = _run(fx, [cloud], leaf)
        assert st[0] == 0
        D.check_against_float64(cloud, leaf, out[:n_out[0]])


def test_voxel_downsample_random_draws(fx):
    """A slice of tools/stress_downsample.py: random draws over the generators, against the oracle."""
    from tests import downsample_cases as D
    rng = np.random.default_rng(43)
    for _ in range(6):
        leaf = float(np.float32(10.0 ** rng.uniform(-2, 0.5)))
        clouds = [D.draw(rng)[0] for _ in range(8)]
        _check_against_oracle(range(len(clouds)), clouds, leaf, *_run(fx, clouds, leaf))
