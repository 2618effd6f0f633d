"""lfx_scan_context_batch on the device (include/lfx.h, the place recognition section) against the numpy restatement
(tests/scan_context_restatement.py), bit for bit: every route a scan can take, a record layout the general loader reads,
the smallest and the largest grid, hand-placed records on every edge of the arithmetic, scans that give nothing, an
output buffer used twice, and what the call refuses."""
import ctypes as C

import numpy as np
import pytest

from tests import deskew_cases as K
from tests import scan_context_restatement as R

pytestmark = pytest.mark.gpu

RINGS, COLS = R.RINGS, R.COLS
ROUTES = ["organised", "shuffled", "dropped", "zeros"]
CONFIGS = [dict(), dict(n_rings=1, n_sectors=4), dict(n_rings=40, n_sectors=120)]

_SCANS = {}


def _scans():
    """Five 16 x 900 scans from different places of the room, made once."""
    from lidar_feature_extraction_amd import make_scan
    if not _SCANS:
        _SCANS["base"] = [make_scan(RINGS, COLS, seed=700 + s, sensor_pose=(1.5 * s - 3.0, 0.4 * s, 0.3 * s)) for s in range(5)]
    return _SCANS["base"]


def _routed(clouds, route, rng):
    out = []
    for c in clouds:
        c = c.copy()
        if route == "shuffled":
            c = c[rng.permutation(len(c))]
        elif route == "dropped":
            c = c[rng.uniform(0, 1, len(c)) >= 0.05]
        elif route == "zeros":
            z = rng.uniform(0, 1, len(c)) < 0.05
            c["x"][z], c["y"][z], c["z"][z] = 0.0, 0.0, 0.0
        out.append(np.ascontiguousarray(c))
    return out


def _device_batch(fx, records, counts):
    """records (bytes of the scans back to back) through the device path; the device buffer, which the caller keeps alive."""
    d = K.upload_bytes(records) if len(records) else K.upload_bytes(np.zeros(32, np.uint8))
    fx.extract_batch_device(d.data_ptr(), counts, K.stream())
    return d


def _got(fx, cfg):
    out = fx.scan_context(cfg, None, K.stream())
    K.sync()
    return out.cpu().numpy()


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError((what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.mark.parametrize("route", ROUTES)
def test_descriptors_on_every_route(route):
    """Batches of 1, 3 and 5 scans on one route -- read in place, shuffled (bucketed), with 5 % of the records dropped, with
    5 % written as (0, 0, 0) and the zero filter on -- for the default grid, the smallest (1 x 4) and the largest (40 x 120):
    every float equals the restatement's on the same records."""
    from lidar_feature_extraction_amd import binding as B, concat
    rng = np.random.default_rng(40 + ROUTES.index(route))
    kw = dict(drop_zero_points=True, stream_hint=B.STREAM_GRID_WITH_HOLES) if route == "zeros" else {}
    fx = K.fx_for(RINGS, COLS, 5, **kw)
    clouds = _routed(_scans(), route, rng)
    want = {i: [R.descriptor_of_cloud(R.config(**f), c) for c in clouds] for i, f in enumerate(CONFIGS)}
    for n in (1, 3, 5):
        batch = clouds[5 - n:]
        d = _device_batch(fx, concat(batch), [len(c) for c in batch])
        fx.batch_status(K.stream())
        for i, f in enumerate(CONFIGS):
            got = _got(fx, R.config(**f))
            _same(got, np.stack(want[i][5 - n:]), (route, n, f))
            # (not an empty comparison: the room reaches 12 m of the grid's 80, at most 15 % of its cells)
            assert (got > 0).mean() > (0.5 if i == 1 else 0.02), (route, n, f)
        del d
    fx.close()


@pytest.mark.parametrize("be", [False, True], ids=["le", "be"])
def test_descriptors_from_unaligned_records(be):
    """29-byte records x1 y5 z9 (tests/layout_cases.py), in both byte orders: the general loader's three 4-byte loads from
    addresses aligned to nothing."""
    from lidar_feature_extraction_amd import FeatureExtraction, binding as B
    from tests import layout_cases as LC
    lay = LC.timed29(B.FLOAT32, be)
    clouds = _scans()[:3]
    fx = FeatureExtraction(device=0, max_points_per_scan=RINGS * COLS, max_batch=3, max_points_per_ring=COLS, max_rings=RINGS,
                           layout=lay.library_layout())
    records = np.concatenate([lay.fill(c).view(np.uint8) for c in clouds])
    d = _device_batch(fx, records, [len(c) for c in clouds])
    fx.batch_status(K.stream())
    for f in CONFIGS:
        cfg = R.config(**f)
        _same(_got(fx, cfg), np.stack([R.descriptor_of_cloud(cfg, c) for c in clouds]), (be, f))
    del d
    fx.close()


def _hand_cloud():
    """Records on every edge of the header's arithmetic, for 3 rings x 8 sectors out to 12 m (ring_r2 = 0, 16, 64, 144) and
    min_radius 0.5 (or 0)."""
    from lidar_feature_extraction_amd import POINT_DTYPE
    f = np.float32
    below, above = (lambda v: np.nextafter(f(v), f(0))), (lambda v: np.nextafter(f(v), f(np.inf)))
    nan, inf = f(np.nan), f(np.inf)
    rec = [
        (5, 0, 0.1), (-5, 0, 0.2), (0, 5, 0.3), (0, -5, 0.4),                                  # every axis
        (9, 0.0, 0.5), (9, -0.0, 0.6), (-9, 0.0, 0.7), (-9, -0.0, 0.8),                        # y = +0.0 and -0.0 on both sides of x
        (0, 4, 1.0), (0, below(4), 1.1), (0, above(4), 1.2),                                   # r2 at, below, above ring_r2[1]
        (0, -8, 1.3), (0, -below(8), 1.4), (0, -above(8), 1.5),                                # ... ring_r2[2]
        (12, 0, 9.0), (below(12), 0, 1.6), (above(12), 0, 9.0),                                # ... ring_r2[R]
        (-0.5, 0, 1.7), (-below(0.5), 0, 9.0), (-above(0.5), 0, 1.8),                          # ... min_radius^2
        (7, 7, -5.0), (-7, -6, -0.0),                                                          # z below -sensor_height; z = -0.0
        (nan, 2, 9.0), (2, nan, 9.0), (2, 2, nan), (inf, 2, 9.0), (2, inf, 9.0), (2, -2, inf),
        (-inf, 2, 9.0), (2, -inf, 9.0), (2, -2, -inf),
        (0, 0, 0), (0.0, -0.0, 0), (-0.0, 0.0, 0),                                             # (0, 0, 0)
        (3, 4, 2.0), (3, 4, 2.5), (3, 4, -1.0),                                                # one cell, three heights
    ]
    c = np.zeros(len(rec), POINT_DTYPE)
    a = np.array(rec, np.float32)
    c["x"], c["y"], c["z"], c["pad"] = a[:, 0], a[:, 1], a[:, 2], 1.0
    c["ring"] = np.arange(len(rec)) % RINGS
    return c


def test_hand_placed_records_and_scans_that_give_nothing():
    """One batch: the hand-placed cloud, an empty scan, a scan entirely out of range, an ordinary scan.  Bit for bit against
    the restatement for min_radius 0.5 and 0 and for the default grid; a few cells by hand; the empty scan and the one out of
    range are all zeros."""
    from lidar_feature_extraction_amd import POINT_DTYPE, concat
    hand = _hand_cloud()
    far = np.zeros(48, POINT_DTYPE)
    far["x"], far["y"], far["z"], far["pad"] = 20.0 + np.arange(48), 20.0, 1.0, 1.0
    far["ring"] = np.arange(48) % RINGS
    far["x"][7] = 200.0                          # (beyond the default grid's 80 m as well; the others lie inside it)
    empty = np.zeros(0, POINT_DTYPE)
    clouds = [hand, empty, far, _scans()[0]]
    fx = K.fx_for(RINGS, COLS, 4)
    d = _device_batch(fx, concat(clouds), [len(c) for c in clouds])
    for min_radius in (0.5, 0.0):
        cfg = R.config(n_rings=3, n_sectors=8, max_radius=12.0, min_radius=min_radius, sensor_height=1.5)
        got = _got(fx, cfg)
        _same(got, np.stack([R.descriptor_of_cloud(cfg, c) for c in clouds]), min_radius)
        assert not got[1].any() and not got[2].any() and got[3].any()
        g = got[0]
        # sectors of 45 degrees from -pi: +x is sector 4, +y 6; -x with y = +-0.0 is the upper half's last, 7; -y is the
        # first direction of sector 2, and whether the table's cos(-pi / 2) lets it count decides between 1 and 2
        h = np.float32(1.5)
        assert g[1][4] == np.float32(0.1) + h and g[1][6] == np.float32(1.2) + h
        assert max(g[1][1], g[1][2]) == np.float32(1.4) + h and min(g[1][1], g[1][2]) == 0.0
        assert max(g[2][1], g[2][2]) == np.float32(1.5) + h and min(g[2][1], g[2][2]) == 0.0
        assert g[2][4] == np.float32(1.6) + np.float32(1.5)                                # 9 and just under 12 on +x; 12 itself is out
        assert g[2][7] == np.float32(0.8) + h and g[1][7] == np.float32(0.2) + h
        assert g[0][6] == np.float32(1.1) + h
        assert g[2][5] == 0.0 and g[2][0] == 1.5                                               # below the ground; z = -0.0
        assert g[1][5] == 4.0                                                                  # (3, 4): the largest of three
        assert g[0][4] == 0.0 and g[0][3] == 0.0 and g[0][5] == 0.0                            # nothing of the non-finite records
        # ring 0 on -x: 0.5 and just above it, and with min_radius 0 the (0, 0, 0) records too (y >= 0: all of the upper
        # half's directions count) -- the lower z of 0 does not show; just under 0.5 m (z = 9) only without a min_radius
        assert g[0][7] == (np.float32(9.0) + np.float32(1.5) if min_radius == 0.0 else np.float32(1.8) + np.float32(1.5))
    zeros_only = np.zeros(5, POINT_DTYPE)
    zeros_only["ring"] = np.arange(5)
    d2 = _device_batch(fx, concat([zeros_only]), [5])
    for min_radius, want in ((0.0, 1.5), (0.1, 0.0)):
        cfg = R.config(n_rings=3, n_sectors=8, max_radius=12.0, min_radius=min_radius, sensor_height=1.5)
        got = _got(fx, cfg)
        assert got[0][0][7] == want and np.count_nonzero(got) == (1 if want else 0), (min_radius, got)
    d3 = _device_batch(fx, concat(clouds), [len(c) for c in clouds])
    cfg = R.config()
    _same(_got(fx, cfg), np.stack([R.descriptor_of_cloud(cfg, c) for c in clouds]), "defaults")
    del d, d2, d3
    fx.close()


def test_an_output_buffer_used_twice_holds_nothing_stale():
    """Two calls into one buffer after different batches: the second result equals a call into a fresh buffer (every cell is
    written on every call), with more calls than the context has table slots in between."""
    import torch
    from lidar_feature_extraction_amd import concat
    fx = K.fx_for(RINGS, COLS, 3)
    cfg = R.config()
    clouds = _scans()
    out = torch.full((3, 20, 60), float("nan"), dtype=torch.float32, device=K.dev())
    d = _device_batch(fx, concat(clouds[:3]), [len(c) for c in clouds[:3]])
    assert fx.scan_context(cfg, out.data_ptr(), K.stream()) is None
    K.sync()
    first = out.cpu().numpy().copy()
    _same(first, np.stack([R.descriptor_of_cloud(cfg, c) for c in clouds[:3]]), "first")
    # a sparser batch: the last scan cut to its first ring columns, so that cells the first batch filled stay empty
    cut = [clouds[3], clouds[4], np.ascontiguousarray(clouds[0][:RINGS * 40])]
    d2 = _device_batch(fx, concat(cut), [len(c) for c in cut])
    for _ in range(6):
        fx.scan_context(cfg, out.data_ptr(), K.stream())
    K.sync()
    second = out.cpu().numpy().copy()
    fresh = _got(fx, cfg)
    _same(second, fresh, "second")
    _same(second, np.stack([R.descriptor_of_cloud(cfg, c) for c in cut]), "second against the restatement")
    # (the cut scan sees 16 of 360 degrees: most of what the first batch's third scan filled must now be empty)
    assert ((first[2] > 0) & (second[2] == 0)).sum() >= 50
    del d, d2
    fx.close()


def test_refusals():
    """LFX_ERR_INVALID_ARGUMENT, with the output untouched: no batch yet, NULL arguments, R or S out of range, S odd, radii
    that are not finite or not in order, n_scans that is not the last batch's."""
    import torch
    from lidar_feature_extraction_amd import binding as B, concat
    L = B.load()
    fx = K.fx_for(RINGS, COLS, 2)
    out = torch.full((2, 40, 120), 7.0, dtype=torch.float32, device=K.dev())
    cfg = R.config()

    def refused(cfg, n=2, ptr=None, ctx=None):
        c = C.byref(cfg) if cfg is not None else None
        rc = L.lfx_scan_context_batch(fx._ctx if ctx is None else ctx, c, n, C.c_void_p(out.data_ptr() if ptr is None else ptr), C.c_void_p(K.stream()))
        assert rc == B.ERR_INVALID_ARGUMENT, rc

    refused(cfg)                                  # no batch yet
    clouds = _scans()[:2]
    d = _device_batch(fx, concat(clouds), [len(c) for c in clouds])
    refused(None)
    refused(cfg, ptr=0)
    refused(cfg, ctx=C.c_void_p(0))
    for n in (0, 1, 3):
        refused(cfg, n=n)
    for fields in (dict(n_rings=0), dict(n_rings=41), dict(n_sectors=2), dict(n_sectors=59), dict(n_sectors=122), dict(max_radius=float("nan")),
                   dict(max_radius=float("inf")), dict(min_radius=-1.0), dict(min_radius=80.0), dict(min_radius=float("nan")),
                   dict(sensor_height=float("nan"))):
        refused(R.config(**fields))
    K.sync()
    assert (out.cpu().numpy() == 7.0).all()
    _same(_got(fx, cfg), np.stack([R.descriptor_of_cloud(cfg, c) for c in clouds]), "after the refusals")
    del d
    fx.close()
