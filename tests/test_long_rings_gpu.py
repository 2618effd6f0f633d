"""Rings longer than LFX_MAX_RING_POINTS (4 608): contexts created with a larger max_points_per_ring hand such rings to the
long-ring kernel (workspace in HBM).  Every output against the CPU oracle: bit-exact labels, curvature bits, index sets and
clouds (tests/parity.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from lidar_feature_extraction_amd import FeatureExtraction, HyperParameters, make_scan, POINT_DTYPE  # noqa: E402
from lidar_feature_extraction_amd import binding as LB, synth  # noqa: E402
from oracle import binding as OB  # noqa: E402
from tests.parity import assert_scan_equal, assert_filtered_equal  # noqa: E402

PARAM_SETS = {"defaults": HyperParameters(), "launch_yaml": HyperParameters.launch_yaml()}


def oracle_params(hp):
    return OB.Params(hp.padding, hp.neighbor_degree_threshold, hp.distance_diff_threshold,
                     hp.parallel_beam_min_range_ratio, hp.edge_threshold, hp.surface_threshold,
                     hp.min_range, hp.max_range, hp.n_blocks)


def want_of(c, hp=None):
    return OB.extract(c, params=None if hp is None else oracle_params(hp), canonical_ties=True)


def ring_lengths(rings_cols, seed, **kw):
    """One scan whose ring r has rings_cols[r] points (ids 0 .. len - 1), each ring a make_scan ring of its own length."""
    parts = []
    for r, cols in enumerate(rings_cols):
        p = make_scan(1, cols, seed=seed + r, **kw)
        p["ring"] = r
        parts.append(p)
    return synth.concat(parts)


def test_create_accepts_long_ring_capacity():
    f = FeatureExtraction(device=0, max_points_per_scan=4 * 20000, max_batch=1, max_points_per_ring=20000, max_rings=4)
    f.close()
    assert LB.MAX_RING_POINTS == 4608 and LB.MAX_LONG_RING_POINTS == 262144
    with pytest.raises(LB.LfxError):
        FeatureExtraction(device=0, max_points_per_scan=1 << 20, max_batch=1, max_points_per_ring=LB.MAX_LONG_RING_POINTS + 1,
                          max_rings=4)


def test_four_rings_of_6000():
    c = make_scan(4, 6000, seed=601)
    f = FeatureExtraction(device=0, max_points_per_scan=len(c), max_batch=1, max_points_per_ring=6000, max_rings=4)
    got = f.ExtractFeatures(c)
    assert got.ring_status.tolist() == [0, 0, 0, 0]
    assert_scan_equal(got, want_of(c), "4 x 6000")
    assert len(got.edge_index) > 0 and len(got.surface_index) > 0
    f.close()


@pytest.mark.parametrize("rings,cols,kw", [
    (4, 5000, {"shuffle": True}),               # line-based sensor: no order within a line, every ring sorted
    (6, 8000, {}),
    (6, 8000, {"start_col": 3001}),
    (4, 9000, {"reverse": True}),
    (2, 32768, {"shuffle": True}),
    (1, 70000, {}),                             # positions beyond 65 535
    (1, 70000, {"shuffle": True}),
], ids=lambda v: str(v))
def test_shapes(rings, cols, kw):
    c = make_scan(rings, cols, seed=700 + rings + cols, **kw)
    f = FeatureExtraction(device=0, max_points_per_scan=len(c), max_batch=1, max_points_per_ring=cols, max_rings=rings)
    got = f.ExtractFeatures(c)
    assert not got.ring_status.any()
    assert_scan_equal(got, want_of(c), "%d x %d %s" % (rings, cols, kw))
    f.close()


@pytest.mark.parametrize("name", sorted(PARAM_SETS))
@pytest.mark.parametrize("shuffle", [False, True])
def test_parameter_sets(name, shuffle):
    hp = PARAM_SETS[name]
    c = make_scan(3, 7000, seed=810, shuffle=shuffle)
    f = FeatureExtraction(params=hp, device=0, max_points_per_scan=len(c), max_batch=1, max_points_per_ring=7000, max_rings=3)
    assert_scan_equal(f.ExtractFeatures(c), want_of(c, hp), "%s shuffle=%s" % (name, shuffle))
    f.close()


@pytest.mark.parametrize("padding,n_blocks", [(20, 6), (5, 1), (5, 64), (2, 64), (20, 1)])
def test_padding_and_blocks(padding, n_blocks):
    """Padding 20: label_pass_wide (reach kept as two run lengths); one block of the whole ring; 64 short blocks (which
    the unit kernels would take for a ring of 4 608 points or fewer)."""
    hp = HyperParameters(padding=padding, n_blocks=n_blocks)
    c = make_scan(2, 12000, seed=900 + padding + n_blocks, shuffle=True)
    f = FeatureExtraction(params=hp, device=0, max_points_per_scan=len(c), max_batch=1, max_points_per_ring=12000, max_rings=2)
    assert_scan_equal(f.ExtractFeatures(c), want_of(c, hp), "P%d B%d" % (padding, n_blocks))
    f.close()


@pytest.mark.parametrize("max_rings", [8, 0])
def test_mixed_short_and_long_rings(max_rings):
    """One batch: short rings through the unit kernels (and the LDS-resident kernels for the shuffled one), long rings through
    the long-ring kernel, on a context with the sensor's ring count and one without."""
    scans = [ring_lengths([900, 6000, 2000, 4608, 4609, 10000, 300, 7000], seed=1000),
             ring_lengths([5000, 100, 4000, 12000], seed=1100, shuffle=True),
             make_scan(8, 1800, seed=1200)]
    f = FeatureExtraction(device=0, max_points_per_scan=max(len(c) for c in scans), max_batch=3, max_points_per_ring=12000,
                          max_rings=max_rings)
    got = f.extract_batch(scans)
    for i, c in enumerate(scans):
        assert_scan_equal(got[i], want_of(c), "mixed scan %d (max_rings %d)" % (i, max_rings))
    f.close()


def test_organised_grid_of_long_rings_falls_back():
    """A 16 x 6 000 grid in column-major order on a context with the sensor's ring count: the organised route takes the
    scan first, cannot take rings that long, and the scan is redone through bucketing and the long-ring kernel."""
    c = make_scan(16, 6000, seed=1300)
    f = FeatureExtraction(device=0, max_points_per_scan=len(c), max_batch=1, max_points_per_ring=6000, max_rings=16)
    for rep in range(3):                            # (the route choice follows what earlier batches reported)
        assert_scan_equal(f.ExtractFeatures(c), want_of(c), "16 x 6000 grid rep %d" % rep)
    f.close()


def _zeroed(c, frac, seed):
    z = c.copy()
    rng = np.random.default_rng(seed)
    pick = rng.uniform(0, 1, len(z)) < frac
    z["x"][pick] = 0.0
    z["y"][pick] = 0.0
    z["z"][pick] = 0.0
    return z, (z["x"] == 0) & (z["y"] == 0) & (z["z"] == 0)


@pytest.mark.parametrize("max_rings", [4, 0])
def test_zero_records_filtered(max_rings):
    """(0, 0, 0) records with drop_zero_points: a long-ring context declines the holes form; the grid is bucketed."""
    scans = [_zeroed(make_scan(4, 6000, seed=1400 + i), 0.05, 1500 + i) for i in range(2)]
    f = FeatureExtraction(device=0, max_points_per_scan=4 * 6000, max_batch=2, max_points_per_ring=6000, max_rings=max_rings,
                          drop_zero_points=True)
    for rep in range(3):
        got = f.extract_batch([z for z, _ in scans])
        for i, (z, mask) in enumerate(scans):
            keep = np.nonzero(~mask)[0]
            want = OB.extract(np.ascontiguousarray(z[keep]), canonical_ties=True)
            assert_filtered_equal(got[i], want, keep, mask, "zeros scan %d rep %d" % (i, rep))
    f.close()


def test_skip_statuses_next_to_valid_long_rings():
    """A zero-norm adjacent pair (status 5) on a long ring, and a ring above the context's capacity (status 7), each beside
    long rings that are labelled."""
    a = ring_lengths([6000, 6000, 6000], seed=1600)
    r1 = np.nonzero(a["ring"] == 1)[0]
    for k in r1[100:102]:
        a["x"][k] = 0.0
        a["y"][k] = 0.0                              # z stays: x = y = 0 is a zero-norm point the zero filter keeps
    b = ring_lengths([6000, 9000, 5000], seed=1700, shuffle=True)
    f = FeatureExtraction(device=0, max_points_per_scan=len(b), max_batch=2, max_points_per_ring=8000, max_rings=3)
    got = f.extract_batch([a, b])
    wa = want_of(a)
    assert got[0].ring_status.tolist() == [0, 5, 0]
    assert_scan_equal(got[0], wa, "zero pair [ties]")   # (the two zero-norm points tie in angle; canonical order)
    assert got[1].ring_status.tolist() == [0, 7, 0]
    # the oracle takes the ring of 9 000; the library skips it: compare the other two rings against the oracle on the scan
    # without it
    keep = np.nonzero(b["ring"] != 1)[0]
    wb = OB.extract(np.ascontiguousarray(b[keep]), canonical_ties=True)
    assert np.array_equal(got[1].labels[keep], wb["labels"]) and not got[1].labels[b["ring"] == 1].any()
    assert got[1].curvature[keep].tobytes() == wb["curvature"].tobytes()
    assert np.array_equal(got[1].edge_index, keep[wb["edge_index"]].astype(np.uint32))
    assert np.array_equal(got[1].surface_index, keep[wb["surface_index"]].astype(np.uint32))
    assert got[1].edge_points.tobytes() == wb["edge_points"].tobytes()
    assert got[1].surface_points.tobytes() == wb["surface_points"].tobytes()
    f.close()


def test_one_context_over_batches_of_changing_size():
    """Consecutive batches of different sizes and orders on one context: both sets of accumulators, the long list emptied
    between batches."""
    f = FeatureExtraction(device=0, max_points_per_scan=4 * 9000, max_batch=5, max_points_per_ring=9000, max_rings=4)
    batches = [
        [make_scan(4, 9000, seed=1800, shuffle=True)],
        [make_scan(4, 5000, seed=1810 + i, start_col=77 * i) for i in range(5)],
        [make_scan(4, 1200, seed=1820), make_scan(2, 9000, seed=1821)],
        [make_scan(4, 7000, seed=1830 + i, shuffle=i % 2 == 1) for i in range(3)],
        [make_scan(4, 9000, seed=1800, shuffle=True)],
    ]
    for b, scans in enumerate(batches):
        got = f.extract_batch(scans)
        for i, c in enumerate(scans):
            assert_scan_equal(got[i], want_of(c), "batch %d scan %d" % (b, i))
    f.close()


def test_host_entry_points():
    """lfx_extract, submit / wait (two in flight), and the device path with download, pack_xyz / pack_xyz12 / pack_colored."""
    import torch
    clouds = [make_scan(4, 6000, seed=1900, shuffle=True), make_scan(3, 8000, seed=1901), make_scan(4, 5000, seed=1902, reverse=True)]
    wants = [want_of(c) for c in clouds]
    f = FeatureExtraction(device=0, max_points_per_scan=max(len(c) for c in clouds), max_batch=3, max_points_per_ring=8000,
                          max_rings=4)
    for i, c in enumerate(clouds):
        assert_scan_equal(f.ExtractFeatures(c), wants[i], "host %d" % i)
    t0 = f.submit(clouds[0])
    t1 = f.submit(clouds[1])
    assert_scan_equal(f.wait(t0), wants[0], "submit 0")
    t2 = f.submit(clouds[2])
    assert_scan_equal(f.wait(t1), wants[1], "submit 1")
    assert_scan_equal(f.wait(t2), wants[2], "submit 2")
    stream = torch.cuda.current_stream().cuda_stream
    dev = torch.from_numpy(synth.concat(clouds).view(np.uint8).copy()).to("cuda:0")
    f.extract_batch_device(dev.data_ptr(), [len(c) for c in clouds], stream)
    for i in range(3):
        assert_scan_equal(f.download(i, stream), wants[i], "device %d" % i)
    cap = sum(len(c) for c in clouds)
    nb = len(clouds)
    e = torch.zeros((cap, 4), dtype=torch.float32, device="cuda:0")
    s = torch.zeros((cap, 4), dtype=torch.float32, device="cuda:0")
    offs = torch.zeros(2 * (nb + 1), dtype=torch.int32, device="cuda:0")
    e12 = torch.zeros((cap, 3), dtype=torch.float32, device="cuda:0")
    s12 = torch.zeros((cap, 3), dtype=torch.float32, device="cuda:0")
    offs12 = torch.zeros(2 * (nb + 1), dtype=torch.int32, device="cuda:0")
    col = torch.zeros((cap, 8), dtype=torch.float32, device="cuda:0")
    coffs = torch.zeros(nb + 1, dtype=torch.int32, device="cuda:0")
    f.pack_xyz(e.data_ptr(), s.data_ptr(), offs.data_ptr(), cap, stream)
    f.pack_xyz12(e12.data_ptr(), s12.data_ptr(), offs12.data_ptr(), cap, stream)
    f.pack_colored(col.data_ptr(), coffs.data_ptr(), cap, stream)
    torch.cuda.synchronize()
    e, s, offs, col, coffs = e.cpu().numpy(), s.cpu().numpy(), offs.cpu().numpy(), col.cpu().numpy(), coffs.cpu().numpy()
    assert np.array_equal(offs12.cpu().numpy(), offs)
    assert np.array_equal(e12.cpu().numpy()[:offs[nb]], e[:offs[nb], :3])
    assert np.array_equal(s12.cpu().numpy()[:offs[2 * nb + 1]], s[:offs[2 * nb + 1], :3])
    for i, c in enumerate(clouds):
        w = wants[i]
        for arr, o0, o1, idx in ((e, offs[i], offs[i + 1], w["edge_index"]), (s, offs[nb + 1 + i], offs[nb + 2 + i], w["surface_index"])):
            assert o1 - o0 == len(idx)
            assert np.array_equal(arr[o0:o1, 0], c["x"][idx]) and np.array_equal(arr[o0:o1, 1], c["y"][idx])
            assert np.array_equal(arr[o0:o1, 2], c["z"][idx]) and np.all(arr[o0:o1, 3] == 1.0)
        order = w["sorted_index"]
        assert coffs[i + 1] - coffs[i] == len(c)
        g = col[coffs[i]:coffs[i + 1]]
        assert np.array_equal(g[:, 0], c["x"][order]) and np.array_equal(g[:, 1], c["y"][order])
        assert np.array_equal(g[:, 2], c["z"][order])
    f.close()
