"""lfx_segment_batch on the device (include/lfx.h, the segmentation section) against the numpy restatement
(tests/segment_restatement.py), byte for byte -- class, id and counts: every route a scan can take, hand-made images that are
hard on a parallel labelling (a serpentine, a spiral, a ring round the circle, the seam), the smallest and the largest image
and a batch that crosses the workspace's chunk, degenerate inputs, a record layout the general loader reads, outputs and
workspace used twice, and what the call refuses."""
import ctypes as C

import numpy as np
import pytest

from tests import deskew_cases as K
from tests import segment_restatement as R

pytestmark = pytest.mark.gpu

RINGS, COLS = 16, 900
ROUTES = ["organised", "shuffled", "dropped", "zeros"]

_SCANS = {}


def _scans():
    """Five 16 x 900 scans from different places of the room, made once (the scan-context tests' scans)."""
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


def _numpy(got):
    K.sync()
    cls, ids, counts = got
    return cls.cpu().numpy(), ids.cpu().numpy().view(np.uint32), counts.cpu().numpy().view(np.uint32)


def _same(got, want, what):
    for name, g, w in zip(("class", "id", "counts"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            raise AssertionError((what, name, len(bad), bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def _check(fx, clouds, cfg, what, want=None, **kw):
    from lidar_feature_extraction_amd import concat
    d = _device_batch(fx, concat(clouds), [len(c) for c in clouds])
    got = _numpy(fx.segment(cfg, stream=K.stream()))
    _same(got, R.segment_batch(cfg, clouds, **kw) if want is None else want, what)
    del d
    return got


def _join(parts):
    return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.stack([p[2] for p in parts]))


@pytest.mark.parametrize("route", ROUTES)
def test_every_route(route):
    """Batches of 1, 3 and 5 scans on one route -- read in place, shuffled (bucketed), with 5 % of the records dropped, with
    5 % written as (0, 0, 0) and the zero filter on."""
    from lidar_feature_extraction_amd import binding as B
    rng = np.random.default_rng(40 + ROUTES.index(route))
    kw = dict(drop_zero_points=True, stream_hint=B.STREAM_GRID_WITH_HOLES) if route == "zeros" else {}
    fx = K.fx_for(RINGS, COLS, 5, **kw)
    clouds = _routed(_scans(), route, rng)
    cfg = R.config(n_rows=RINGS, n_columns=COLS)
    want = [R.segment_cloud(cfg, c) for c in clouds]
    for n in (1, 3, 5):
        got = _check(fx, clouds[5 - n:], cfg, (route, n), want=_join(want[5 - n:]))
        fx.batch_status(K.stream())
        # (not an empty comparison: every class is there, and the floor is mostly ground)
        assert (got[2].sum(axis=0) > 0).all() and got[2][:, R.GROUND].min() > 500, got[2]
    fx.close()


# --- hand-made images ----------------------------------------------------------------------------------------------------
def _serpentine(H, W):
    """Even rows full from column 0 to W - 2, odd rows one cell, alternately at the right and at the left end: one component
    that runs through every row, the longest chain an H x W image holds."""
    cells = []
    for r in range(H):
        if r % 2 == 0:
            cells += [(r, c) for c in range(W - 1)]
        else:
            cells.append((r, W - 2 if (r // 2) % 2 == 0 else 0))
    return cells


def _spiral(H, W):
    """A path that winds inwards with an empty lane between its turns."""
    cells, top, bottom, left, right = [], 0, H - 1, 0, W - 2
    while top <= bottom and left <= right:
        cells += [(top, k) for k in range(left, right + 1)]
        cells += [(k, right) for k in range(top + 1, bottom + 1)]
        if bottom - top < 2 or right - left < 2:
            break
        cells += [(bottom, k) for k in range(right - 1, left - 1, -1)]
        cells += [(k, left) for k in range(bottom - 1, top + 1, -1)]
        cells.append((top + 2, left + 1))
        top, bottom, left, right = top + 2, bottom - 2, left + 2, right - 2
    return sorted(set(cells))


def _hand_images(H, W):
    """[(name, cells)] for an H x W image (H >= 8, W >= 64)."""
    ring = [(3, c) for c in range(W)]
    seam = [(2, W - 2), (2, W - 1), (2, 0), (2, 1), (1, 1), (0, 1)]               # least index (0, 1): not a seam cell
    diagonal = [(0, 5), (1, 6), (4, 9), (5, 8)]
    run = lambda row, c0, n: [(row, c) for c in range(c0, c0 + n)]
    thresholds = run(0, 0, 29) + run(2, 0, 30) + [(4, 5), (5, 5), (6, 5), (6, 6)] + [(4, 15), (5, 15), (6, 15), (6, 16), (6, 17)] + \
        [(4, 25), (4, 26), (4, 27), (5, 25), (5, 26)] + [(4, 35), (4, 36), (5, 36), (6, 36), (6, 37)]
    return [("serpentine", _serpentine(H, W)), ("spiral", _spiral(H, W)), ("ring", ring), ("seam", seam), ("diagonal", diagonal),
            ("thresholds", thresholds)]


@pytest.mark.parametrize("shape", [(8, 64), (16, 900)], ids=["8x64", "16x900"])
def test_hand_made_images(shape):
    """One batch of images (ground test off, every record at 10 m: occupied neighbours join), each against the restatement
    and against what the drawing says.  16 x 900: the serpentine and the spiral cross many workgroups."""
    H, W = shape
    cfg = R.config(n_rows=H, n_columns=W, ground_first_row=0, ground_last_row=0)
    images = _hand_images(H, W)
    rng = np.random.default_rng(H)
    clouds = []
    for _, cells in images:
        c = R.image_cloud(cfg, cells)
        clouds.append(np.ascontiguousarray(c[rng.permutation(len(c))]))            # (the records in no particular order)
    fx = K.fx_for(RINGS, max(W, 64), len(clouds))
    cls, ids, counts = _check(fx, clouds, cfg, shape)
    fx.close()
    begin = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    part = {name: (cls[begin[k]:begin[k + 1]], ids[begin[k]:begin[k + 1]], clouds[k]) for k, (name, _) in enumerate(images)}
    for name in ("serpentine", "spiral"):
        c, i, _ = part[name]
        assert set(c.tolist()) == {R.SEGMENT} and set(i.tolist()) == {0}, name
    c, i, _ = part["ring"]
    assert set(c.tolist()) == {R.SEGMENT} and set(i.tolist()) == {3 * W} and len(c) == W
    c, i, _ = part["seam"]
    assert set(c.tolist()) == {R.SEGMENT} and set(i.tolist()) == {1}
    c, i, cloud = part["diagonal"]
    assert set(c.tolist()) == {R.CLUTTER} and sorted(set(i.tolist())) == [5, W + 6, 4 * W + 9, 5 * W + 8]
    c, i, _ = part["thresholds"]
    by_id = {int(k): (int(c[i == k][0]), int((i == k).sum())) for k in np.unique(i)}
    assert by_id == {0: (R.CLUTTER, 29), 2 * W: (R.SEGMENT, 30), 4 * W + 5: (R.CLUTTER, 4), 4 * W + 15: (R.SEGMENT, 5),
                     4 * W + 25: (R.CLUTTER, 5), 4 * W + 35: (R.SEGMENT, 5)}, by_id


def test_the_smallest_image():
    """1 x 4: four cells, columns 90 degrees apart (equal ranges do not join); rows above 0 are not in the image."""
    cfg = R.config(n_rows=1, n_columns=4, ground_first_row=0, ground_last_row=0, small_min_points=1, small_min_rows=1)
    recs = [R.centre_record(cfg, 0, c, 10.0) for c in range(4)] + [R.centre_record(cfg, 1, 2, 10.0), R.centre_record(cfg, 0, 2, 5.0),
                                                                     R.centre_record(cfg, 0, 1, 0.5)]
    fx = K.fx_for(RINGS, 64, 1)
    cls, ids, counts = _check(fx, [R.cloud_of(recs)], cfg, "1x4")
    fx.close()
    assert cls.tolist() == [2, 2, 2, 2, 0, 2, 0] and ids.tolist() == [0, 1, 2, 3, R.NO_ID, 2, R.NO_ID]


def _sparse_large(cfg, seed):
    """A few hundred records of a 128 x 4096 image: a blob of neighbouring cells, the last column through every row (odd
    seeds: one cell per row anywhere), the four corners."""
    rng = np.random.default_rng(seed)
    H, W = int(cfg.n_rows), int(cfg.n_columns)
    r0, c0 = int(rng.integers(0, H - 12)), int(rng.integers(0, W - 12))
    blob = {(r0 + int(a), c0 + int(b)) for a, b in rng.integers(0, 12, (150, 2))}
    column = {(r, int(rng.integers(0, W))) for r in range(H)} if seed % 2 else {(r, 4095) for r in range(H)}
    cells = sorted(blob | column | {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)})
    return R.cloud_of([R.centre_record(cfg, r, c, 10.0 + 0.05 * int(rng.integers(0, 4))) for r, c in cells])


def test_the_largest_image_and_a_batch_over_the_chunk():
    """128 x 4096 with a few hundred records, alone and then in a batch one scan over what the workspace takes at a time."""
    from lidar_feature_extraction_amd import binding as B
    cfg = R.config(n_rows=128, n_columns=4096, ground_first_row=0, ground_last_row=0)
    per_chunk = B.SEGMENT_BUDGET_CELLS // (128 * 4096)
    assert 24 <= per_chunk <= 64
    clouds = [_sparse_large(cfg, s) for s in range(per_chunk + 1)]
    want = [R.segment_cloud(cfg, c) for c in clouds]
    fx = K.fx_for(128, 64, per_chunk + 1)
    _check(fx, clouds[:1], cfg, "one", want=_join(want[:1]))
    got = _check(fx, clouds, cfg, "over the chunk", want=_join(want))
    fx.close()
    assert got[2][::2, R.SEGMENT].min() >= 128              # (even seeds: the column through every row, one component)


# --- degenerate inputs -----------------------------------------------------------------------------------------------------
def test_empty_and_nan_scans_rows_above_the_image():
    from lidar_feature_extraction_amd import POINT_DTYPE
    empty = np.zeros(0, POINT_DTYPE)
    nans = _scans()[1][:500].copy()
    nans["x"], nans["y"][::2], nans["z"][::3] = np.nan, np.inf, -np.inf
    clouds = [_scans()[0], empty, nans, _scans()[2], empty]
    fx = K.fx_for(RINGS, COLS, 5)
    for H in (16, 8, 1):                                    # (8, 1: rows the image does not have)
        cfg = R.config(n_rows=H, n_columns=COLS, ground_last_row=min(7, H - 1))
        cls, ids, counts = _check(fx, clouds, cfg, H)
        assert counts[1].tolist() == [0, 0, 0, 0] and counts[2].tolist() == [500, 0, 0, 0] and counts[4].tolist() == [0, 0, 0, 0]
        if H < 16:
            assert counts[0][0] >= (16 - H) * COLS
    fx.close()


def test_ring_ids_make_the_row_a_rank():
    from lidar_feature_extraction_amd import FeatureExtraction
    ring_ids = [3 * k + 1 for k in range(RINGS)]
    clouds = []
    for c in _scans()[:2]:
        c = c.copy()
        c["ring"] = 3 * c["ring"] + 1
        clouds.append(c)
    clouds[1]["ring"][::97] = 2                              # an id the context does not know
    fx = FeatureExtraction(device=0, max_points_per_scan=RINGS * COLS, max_batch=2, max_points_per_ring=COLS, max_rings=RINGS, ring_ids=ring_ids)
    cfg = R.config(n_rows=RINGS, n_columns=COLS)
    cls, ids, counts = _check(fx, clouds, cfg, "ring ids", ring_ids=ring_ids)
    fx.close()
    assert counts[0][R.GROUND] > 500 and (cls[len(clouds[0]):][::97] == R.NONE).all()


@pytest.mark.parametrize("be", [False, True], ids=["le", "be"])
def test_unaligned_records(be):
    """29-byte records x1 y5 z9 (tests/layout_cases.py), in both byte orders: the general loader."""
    from lidar_feature_extraction_amd import FeatureExtraction, binding as B
    from tests import layout_cases as LC
    lay = LC.timed29(B.FLOAT32, be)
    clouds = _scans()[:3]
    fx = FeatureExtraction(device=0, max_points_per_scan=RINGS * COLS, max_batch=3, max_points_per_ring=COLS, max_rings=RINGS,
                           layout=lay.library_layout())
    records = np.concatenate([lay.fill(c).view(np.uint8) for c in clouds])
    d = _device_batch(fx, records, [len(c) for c in clouds])
    cfg = R.config(n_rows=RINGS, n_columns=COLS)
    _same(_numpy(fx.segment(cfg, stream=K.stream())), R.segment_batch(cfg, clouds), be)
    del d
    fx.close()


# --- stale state -----------------------------------------------------------------------------------------------------------
def test_outputs_and_workspace_used_twice_and_two_configs_in_turn():
    import torch
    from lidar_feature_extraction_amd import concat
    fx = K.fx_for(RINGS, COLS, 3)
    clouds = _scans()
    cfg = R.config(n_rows=RINGS, n_columns=COLS)
    coarse = R.config(n_rows=RINGS, n_columns=360, segment_min_points=10, ground_tan=0.3)
    total = sum(len(c) for c in clouds[:3])
    cls = torch.full((total,), 77, dtype=torch.uint8, device=K.dev())
    ids = torch.full((total,), 77, dtype=torch.int32, device=K.dev())
    counts = torch.full((3, 4), 77, dtype=torch.int32, device=K.dev())
    d = _device_batch(fx, concat(clouds[:3]), [len(c) for c in clouds[:3]])
    # two configs in turn on one batch, into the same outputs
    for c in (cfg, coarse, cfg, coarse):
        fx.segment(c, cls, ids, counts, K.stream())
        _same(_numpy((cls, ids, counts)), R.segment_batch(c, clouds[:3]), "in turn")
    # a smaller, sparser batch after the larger one: the same outputs and workspace
    cut = [np.ascontiguousarray(clouds[3][:RINGS * 40]), np.ascontiguousarray(clouds[4][::7])]
    d2 = _device_batch(fx, concat(cut), [len(c) for c in cut])
    n = sum(len(c) for c in cut)
    fx.segment(cfg, cls, ids, counts, K.stream())
    got = _numpy((cls, ids, counts))
    want = R.segment_batch(cfg, cut)
    _same((got[0][:n], got[1][:n], got[2][:2]), want, "smaller")
    fresh = _numpy(fx.segment(cfg, stream=K.stream()))
    _same((got[0][:n], got[1][:n], got[2][:2]), fresh, "smaller against fresh outputs")
    # (nothing past the batch's records and scans is touched)
    before = R.segment_batch(coarse, clouds[:3])
    assert got[0][n:].tobytes() == before[0][n:].tobytes() and got[2][2].tolist() == before[2][2].tolist()
    del d, d2
    fx.close()


def test_outputs_are_sized_by_the_batch_the_library_ran_last():
    """segment() sizes what it allocates by lfx_batch_points, the library's own record: after submit() / wait() alone, after a
    small scan followed by a submitted large one, and after an extract_batch of empty clouds, which runs nothing and leaves
    the batch before in place.  Tensors shorter than the batch are refused; ids and counts can be left out."""
    import torch
    from lidar_feature_extraction_amd import POINT_DTYPE, binding as B
    fx = K.fx_for(RINGS, COLS, 1)
    cfg = R.config(n_rows=RINGS, n_columns=COLS)
    small, big = np.ascontiguousarray(_scans()[0][:RINGS * 40]), _scans()[1]
    want_small, want_big = R.segment_batch(cfg, [small]), R.segment_batch(cfg, [big])
    assert fx.batch_points() == 0
    fx.wait(fx.submit(big))
    assert fx.batch_points() == len(big)
    _same(_numpy(fx.segment(cfg, stream=K.stream())), want_big, "submit / wait alone")
    fx.ExtractFeatures(small)
    assert fx.batch_points() == len(small)
    _same(_numpy(fx.segment(cfg, stream=K.stream())), want_small, "small")
    fx.wait(fx.submit(big))
    assert fx.batch_points() == len(big)
    got = fx.segment(cfg, stream=K.stream())
    assert got[0].numel() == len(big) and got[1].numel() == len(big)
    _same(_numpy(got), want_big, "a large scan submitted after a small one")
    fx.ExtractFeatures(small)
    res = fx.extract_batch([np.zeros(0, POINT_DTYPE)])
    assert len(res) == 1 and len(res[0].labels) == 0
    assert fx.batch_points() == len(small) and int(fx.device_view().batch) == 1
    _same(_numpy(fx.segment(cfg, stream=K.stream())), want_small, "after an empty extract_batch")
    n = len(small)
    mark = lambda count, dtype: torch.full((count,), 77, dtype=dtype, device=K.dev())
    for kw in (dict(classes=mark(n - 1, torch.uint8)), dict(ids=mark(n - 1, torch.int32)), dict(counts=mark(3, torch.int32)),
               dict(classes=mark(n, torch.int32)), dict(ids=mark(n, torch.uint8))):
        with pytest.raises(B.LfxError):
            fx.segment(cfg, stream=K.stream(), **kw)
        K.sync()
        assert (list(kw.values())[0].cpu().numpy() == 77).all()
    with pytest.raises(B.LfxError):
        fx.pack_features_segmented(mark(n - 1, torch.uint8), stream=K.stream())
    cls, ids, counts = fx.segment(cfg, ids=False, counts=False, stream=K.stream())
    K.sync()
    assert ids is None and counts is None and cls.cpu().numpy().tobytes() == want_small[0].tobytes()
    fx.close()


# --- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    """LFX_ERR_INVALID_ARGUMENT with the outputs untouched: no batch yet, NULL arguments, every field out of its range, n_rows
    above the context's max_rings, n_scans that is not the last batch's."""
    import torch
    from lidar_feature_extraction_amd import binding as B, concat
    L = B.load()
    fx = K.fx_for(RINGS, COLS, 2)
    clouds = _scans()[:2]
    total = sum(len(c) for c in clouds)
    cls = torch.full((total,), 77, dtype=torch.uint8, device=K.dev())
    ids = torch.full((total,), 77, dtype=torch.int32, device=K.dev())
    counts = torch.full((2, 4), 77, dtype=torch.int32, device=K.dev())
    cfg = R.config(n_rows=RINGS, n_columns=COLS)

    def refused(cfg, n=2, ptr=None, ctx=None):
        c = C.byref(cfg) if cfg is not None else None
        rc = L.lfx_segment_batch(fx._ctx if ctx is None else ctx, c, n, C.c_void_p(cls.data_ptr() if ptr is None else ptr),
                                 C.c_void_p(ids.data_ptr()), C.c_void_p(counts.data_ptr()), C.c_void_p(K.stream()))
        assert rc == B.ERR_INVALID_ARGUMENT, rc

    refused(cfg)                                  # no batch yet
    d = _device_batch(fx, concat(clouds), [len(c) for c in clouds])
    refused(None)
    refused(cfg, ptr=0)
    refused(cfg, ctx=C.c_void_p(0))
    for n in (0, 1, 3):
        refused(cfg, n=n)
    nan, inf = float("nan"), float("inf")
    for fields in (dict(n_rows=0), dict(n_rows=17), dict(n_rows=129), dict(n_columns=2), dict(n_columns=901), dict(n_columns=4098),
                   dict(row_step=0.0), dict(row_step=nan), dict(min_range=0.0), dict(min_range=100.0), dict(max_range=inf), dict(max_range=nan),
                   dict(ground_first_row=8), dict(ground_last_row=16), dict(ground_tan=-1.0), dict(ground_tan=nan), dict(segment_tan=0.0),
                   dict(segment_tan=inf), dict(segment_min_points=0), dict(small_min_points=0), dict(small_min_rows=0)):
        refused(R.config(**dict(dict(n_rows=RINGS, n_columns=COLS), **fields)))
    K.sync()
    assert (cls.cpu().numpy() == 77).all() and (ids.cpu().numpy() == 77).all() and (counts.cpu().numpy() == 77).all()
    _same(_numpy(fx.segment(cfg, cls, ids, counts, K.stream())), R.segment_batch(cfg, clouds), "after the refusals")
    del d
    fx.close()
