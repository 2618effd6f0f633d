"""lfx_distance_* on the device (include/lfx.h, the distance section) against the restatement (tests/distance_restatement.py):
classes, d2, i2, the stats, metres and the costmap are compared byte for byte -- nothing here has a tolerance.
tests/test_distance_expect.py holds the restatement to its own brute force, to scipy and to the hand values.

What the shapes are built around is named in tests/distance_cases.py (SEG_ROWS, TILE, SITES, SEARCH_MAX): the column pass's
y-segments of 64 rows and tiles of 256 columns, the two row kernels on either side of a cap of 64 cells, and the envelope
kernel's workgroups of 64, 256 and 1024 threads for rows of up to 1024, up to 4096 and wider ones."""
import ctypes as C

import numpy as np
import pytest

from tests import deskew_cases as K
from tests import distance_cases as DC
from tests import distance_restatement as D
from tests import occupancy_cases as OC
from tests import occupancy_restatement as O
from tests import segment_cases as S

pytestmark = pytest.mark.gpu
RES = 0.25
COST = dict(inscribed_radius=0.75, inflation_radius=1.25, cost_scaling_factor=3.0)          # Rc = 5 at RES


@pytest.fixture(scope="module")
def fx():
    f = K.fx_for(16, 64, 2)
    yield f
    f.close()


@pytest.fixture(scope="module")
def hold():
    return S.Hold()


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(K.dev())


def _lut(cost, res):
    """the library's own table: the bytes the device is handed (tests/test_distance_expect.py holds them to the restatement)"""
    from lidar_feature_extraction_amd import distance_cost_table
    return distance_cost_table(cost, res)


def _outputs(df, want, cap, what, res=RES, costs=(COST,)):
    """metres and the costmaps of the field the object holds, against the restatement's of `want`"""
    cl, d2, i2, _ = want
    m = df.metres(res, stream=K.stream())
    K.sync()
    DC.same_bytes(m.cpu().numpy(), D.metres(cl, d2, i2, res), (what, "metres"))
    for cost in costs:
        for track in (1, 0):
            cfg = D.cost_config(**dict(cost, track_unknown=track))
            if cap and cap < D.cost_cells(cfg, res):
                continue
            c = df.costmap(res, cfg, stream=K.stream())
            K.sync()
            DC.same_bytes(c.cpu().numpy(), D.costmap(cl, d2, _lut(cfg, res), cfg), (what, "costmap", cost, track))


def _holds(df, want, what):
    """the object's fields and stats are the restatement's"""
    cl, d2, i2, stats = want
    got = df.fields(K.stream())
    DC.same_bytes(got[0], cl, (what, "classes"))
    DC.same_bytes(got[1], d2, (what, "d2"))
    assert (got[2] is None) == (i2 is None), what
    if i2 is not None:
        DC.same_bytes(got[2], i2, (what, "i2"))
    assert df.stats(K.stream()) == stats, (what, df.stats(K.stream()), stats)
    info = df.info()
    assert info["transformed"] == 1 and info["inside"] == int(i2 is not None), (what, info)


def _case(fx, name, G, fields, insides=(False, True), outputs=True, df=None):
    from lidar_feature_extraction_amd import DistanceField
    h, w = G.shape
    own = df is None
    df = DistanceField(fx, w, h) if own else df
    d_grid = _up(G)
    for inside in insides:
        want = DC.expected(name, G, fields, inside)
        df.from_grid(d_grid, stream=K.stream(), **dict(fields, inside=int(inside)))
        _holds(df, want, (name, inside))
        assert df.info()["max_cells"] == fields.get("max_cells", 0)
        if outputs:
            _outputs(df, want, fields.get("max_cells", 0), (name, inside))
    if own:
        df.close()


# --- the grids of tests/distance_cases.py ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DC.smallest(), ids=lambda c: c[0])
def test_smallest_grids(fx, case):
    name, G, fields = case
    _case(fx, name, G, fields)
    cl, d2, i2, stats = DC.expected(name, G, fields, True)
    if name == "no_obstacle" or name == "all_unknown" or name == "1x1_free" or name == "1x1_unknown":
        assert (d2 == D.FAR).all() and stats["max_d2"] == 0 and stats["n_far"] == G.size and (i2 == 0).all()
    if name in ("all_obstacles", "all_unknown_as_obstacles", "1x1_obstacle"):
        assert (i2 == D.FAR).all() and (d2 == 0).all() and stats["n_obstacle"] == G.size
    if name.startswith("percent"):
        assert stats["n_obstacle"] == {"percent_at_the_value": 2, "percent_one_above": 1, "percent_two_above": 0}[name]


@pytest.mark.parametrize("case", DC.capped(), ids=lambda c: c[0])
def test_the_cap(fx, case):
    name, G, fields = case
    _case(fx, name, G, fields)
    d2 = DC.expected(name, G, fields)[1]
    if fields["max_cells"] == 5:
        assert d2[4, 3] == 25 and d2[0, 5] == 25 and d2[1, 5] == D.FAR
    if fields["max_cells"] == 1:
        assert (d2 != D.FAR).sum() == 3
    if fields["max_cells"] in (0, 32767, DC.SEARCH_MAX, DC.SEARCH_MAX + 1):
        assert d2[8, 8] == 128 and (d2 != D.FAR).all()


@pytest.mark.parametrize("case", DC.breakers(), ids=lambda c: c[0])
def test_envelope_breakers(fx, case):
    name, G, fields = case
    _case(fx, name, G, fields)
    if not fields:                  # ... and through the other row kernel, under a cap no distance reaches
        _case(fx, name + "_cap64", G, dict(max_cells=DC.SEARCH_MAX), outputs=False)


@pytest.mark.parametrize("shape", DC.shapes(), ids=lambda s: "%dx%d" % s)
def test_launch_shape_edges(fx, shape):
    w, h = shape
    G = DC.shape_grid(w, h)
    name = "shape_%dx%d" % (w, h)
    _case(fx, name, G, {}, outputs=w * h < 20000)
    _case(fx, name + "_cap9", G, dict(max_cells=9), insides=(False,), outputs=False)


@pytest.mark.parametrize("case", DC.largest(), ids=lambda c: c[0])
def test_largest_sides(fx, case):
    """one obstacle at one end of the longest row and of the longest column: d2 reaches 16383^2 and 16383^2 + 1 -- the 32-bit
    headroom -- and a full-length row finishes; metres takes the square root of the largest values there are"""
    name, G, fields = case
    _case(fx, name, G, fields, insides=(False,), outputs=False)
    cl, d2, _, stats = want = DC.expected(name, G, fields)
    if fields["max_cells"] == 0:
        assert stats["max_d2"] == 16383 ** 2 + 1 and d2[-1, -1] == 16383 ** 2 + 1 and (d2 == 16383 ** 2).sum() == 1 and stats["n_far"] == 0
    else:
        assert stats["max_d2"] == 10000 and stats["n_far"] == G.size - 101 - 100
    from lidar_feature_extraction_amd import DistanceField
    df = DistanceField(fx, G.shape[1], G.shape[0])
    df.from_grid(_up(G), stream=K.stream(), **fields)
    _outputs(df, want, fields["max_cells"], name, res=0.05, costs=({},))
    df.close()


def test_metres_square_roots(fx):
    """every d2 of a 300 x 2 row with one obstacle is a different integer: 0 .. 299^2 and their successors, square roots that
    are exact, just under and just over a float's midpoint among them"""
    G = DC.with_obstacles(2, 300, [(0, 0)])
    from lidar_feature_extraction_amd import DistanceField
    df = DistanceField(fx, 300, 2)
    want = DC.expected("roots", G, {}, True)
    df.from_grid(_up(G), stream=K.stream(), inside=1)
    for res in (0.05, 0.1, 1.0, 0.3333333):
        _outputs(df, want, 0, ("roots", res), res=res, costs=())
    df.close()


# --- one object, many transforms ----------------------------------------------------------------------------------------------------
def test_reuse_of_one_object(fx):
    """dense, then empty, then capped, then `inside` off: nothing of an earlier transform survives"""
    from lidar_feature_extraction_amd import DistanceField
    h, w = 67, 129
    df = DistanceField(fx, w, h)
    assert df.info() == dict(width=w, height=h, transformed=0, max_cells=0, inside=0, device_bytes=df.info()["device_bytes"])
    assert df.info()["device_bytes"] >= w * h * (1 + 2 + 4 + 4) + 1024 * 1024 + 1
    dense, empty = DC.random_grid(h, w, 0.4, seed=3), DC.random_grid(h, w, 0.0, seed=4)
    sparse = DC.random_grid(h, w, 0.002, seed=5)
    _case(fx, "reuse_dense", dense, {}, insides=(True,), df=df)
    _case(fx, "reuse_empty", empty, {}, insides=(True,), df=df)
    assert df.stats(K.stream()) == dict(n_obstacle=0, n_unknown=int((empty < 0).sum()), n_far=w * h, max_d2=0)
    _case(fx, "reuse_capped", sparse, dict(max_cells=6), insides=(True,), df=df)
    assert df.view(K.stream())["i2"] != 0
    _case(fx, "reuse_capped", sparse, dict(max_cells=6), insides=(False,), df=df)
    assert df.view(K.stream())["i2"] == 0 and df.info()["inside"] == 0
    _case(fx, "reuse_dense", dense, dict(unknown_is_obstacle=0), insides=(False,), df=df)
    df.close()


# --- from_occupancy ---------------------------------------------------------------------------------------------------------------
EMITS = ({}, dict(min_observations=3, w_hit=60, w_miss=25, l_min=-100, l_max=200))


def _occupancy(fx, cfg):
    from lidar_feature_extraction_amd import OccupancyGrid
    return OccupancyGrid(fx, cfg.width, cfg.height, cfg.resolution, (cfg.origin_x, cfg.origin_y), cfg.max_scans, config=cfg)


def _same_as_from_grid(fx, g, df, other, what, fields):
    """from_occupancy of the grid's counts is from_grid of the grid's own emit, for both emit configs"""
    for emit in EMITS:
        out = g.emit(stream=K.stream(), **emit)
        other.from_grid(out, stream=K.stream(), **fields)
        df.from_occupancy(g, emit, stream=K.stream(), **fields)
        a, b = df.fields(K.stream()), other.fields(K.stream())
        for name, x, y in zip(("classes", "d2", "i2"), a, b):
            assert (x is None) == (y is None)
            if x is not None:
                DC.same_bytes(x, y, (what, emit, name))
        assert df.stats(K.stream()) == other.stats(K.stream()), (what, emit)
        yield out.cpu().numpy(), a


def test_from_occupancy_on_the_hand_grids():
    from lidar_feature_extraction_amd import DistanceField
    fx = K.fx_for(16, 64, 2)
    for grid in OC.HAND_GRIDS:
        cfg = OC.hand_config(8, *grid)
        df, other = DistanceField(fx, *grid), DistanceField(fx, *grid)
        for name in sorted(OC.HAND):
            clouds, poses = OC.hand_scans(name)
            g = _occupancy(fx, cfg)
            d = S.device_batch(fx, clouds)
            g.add_batch(poses, stream=K.stream())
            g.render(stream=K.stream())
            for G, got in _same_as_from_grid(fx, g, df, other, (name, grid), dict(occupied_percent=60, inside=1)):
                want = DC.expected("hand_%s_%dx%d_%d" % ((name,) + grid + (int((G < 0).sum()),)), G, dict(occupied_percent=60), True)
                DC.same_bytes(got[1], want[1], (name, "d2"))
                DC.same_bytes(got[2], want[2], (name, "i2"))
            g.close()
            del d
        df.close()
        other.close()
    fx.close()


def _grid33(fx):
    cfg = O.config(n_beams=64, max_scans=S.N_SCANS, width=512, height=512, resolution=0.4, origin_x=-102.4, origin_y=-102.4, chunk_scans=8)
    g = _occupancy(fx, cfg)
    d = S.device_batch(fx, S.scans33())
    g.add_batch(OC.tilted_poses(S.N_SCANS, seed=33), stream=K.stream())
    return g, d


def test_from_occupancy_on_33_scans():
    from lidar_feature_extraction_amd import DistanceField
    fx = S.fx33()
    g, d = _grid33(fx)
    g.render(stream=K.stream())
    df, other = DistanceField(fx, 512, 512), DistanceField(fx, 512, 512)
    for k, (G, got) in enumerate(_same_as_from_grid(fx, g, df, other, "33 scans", dict(max_cells=0, inside=1))):
        st = df.stats(K.stream())
        assert st["n_obstacle"] > 20 and st["n_unknown"] > 10000 and st["n_far"] == 0 and st["max_d2"] > 100 * 100, st
        if k == 0:
            want = DC.expected("33_scans", G, {}, False)
            DC.same_bytes(got[1], want[1], "33 scans against the restatement")
    list(_same_as_from_grid(fx, g, df, other, "33 scans capped", dict(max_cells=12)))
    # a grid of another size is refused, and the field stays
    small = DistanceField(fx, 512, 511)
    before = df.fields(K.stream())
    with pytest.raises(Exception):
        small.from_occupancy(g, stream=K.stream())
    with pytest.raises(Exception):
        df.from_occupancy(g, dict(w_hit=0), stream=K.stream())
    for x, y in zip(before, df.fields(K.stream())):
        assert (x is None and y is None) or x.tobytes() == y.tobytes()
    for o in (small, other, df, g):
        o.close()
    fx.close()
    del d


def test_from_occupancy_behind_a_render_on_the_other_stream(hold):
    """A render queued on a held stream A, then at once a from_occupancy on B and a clear on A: the transform sees the
    rendered counts, and the clear, issued after it, does not reach its read."""
    from lidar_feature_extraction_amd import DistanceField
    fx = S.fx33()
    g, d = _grid33(fx)
    df, other = DistanceField(fx, 512, 512), DistanceField(fx, 512, 512)
    K.sync()
    a, b = S.two_streams()
    hold(a)
    g.render(stream=a.cuda_stream)
    e = S.event_behind(a)
    hold.still_held(e, "distance: render on A, from_occupancy on B")
    df.from_occupancy(g, stream=b.cuda_stream, inside=1)
    g.clear(stream=a.cuda_stream)
    got = df.fields(b.cuda_stream)
    K.sync()
    hits, misses = g.counts(K.stream())
    assert not hits.any() and not misses.any()
    g.render(stream=K.stream())
    other.from_grid(g.emit(stream=K.stream()), stream=K.stream(), inside=1)
    want = other.fields(K.stream())
    assert want[1].min() == 0 and (want[0] == D.OBSTACLE).sum() > 100
    for name, x, y in zip(("classes", "d2", "i2"), got, want):
        DC.same_bytes(x, y, ("two streams", name))
    for o in (other, df, g):
        o.close()
    fx.close()
    del d


def test_a_clear_on_the_other_stream_waits_for_a_held_from_occupancy(hold):
    """The reader's half of the two-object call: a from_occupancy queued on a held stream B records the grid's event too, so
    a clear of the grid issued on A while B is still held does not reach the counts before the transform has read them."""
    from lidar_feature_extraction_amd import DistanceField
    fx = S.fx33()
    g, d = _grid33(fx)
    g.render(stream=K.stream())
    df, other = DistanceField(fx, 512, 512), DistanceField(fx, 512, 512)
    other.from_grid(g.emit(stream=K.stream()), stream=K.stream(), inside=1)
    want = other.fields(K.stream())
    assert want[1].min() == 0 and (want[0] == D.OBSTACLE).sum() > 100
    K.sync()
    a, b = S.two_streams()
    hold(b)
    df.from_occupancy(g, stream=b.cuda_stream, inside=1)
    e = S.event_behind(b)
    hold.still_held(e, "distance: from_occupancy on B, clear of its grid on A")
    g.clear(stream=a.cuda_stream)
    got = df.fields(b.cuda_stream)
    K.sync()
    for name, x, y in zip(("classes", "d2", "i2"), got, want):
        DC.same_bytes(x, y, ("a held reader", name))
    hits, misses = g.counts(K.stream())
    assert not hits.any() and not misses.any()               # (and the clear did run)
    for o in (other, df, g):
        o.close()
    fx.close()
    del d


# --- the outputs --------------------------------------------------------------------------------------------------------------------
def test_outputs_to_device_pinned_and_unaligned_memory(fx):
    """metres and costmap into device memory, into a pinned block and into a device pointer that is not 4-byte aligned (the
    bytes around it untouched); a second cost config, then the first again; a costmap the cap does not cover is refused"""
    import torch
    from lidar_feature_extraction_amd import DistanceField
    h, w = 37, 71                                                # (an odd number of cells: the last thread's four reach past the end)
    G = DC.random_grid(h, w, 0.01, seed=9)
    df = DistanceField(fx, w, h)
    want = DC.expected("outputs", G, dict(max_cells=7), True)
    cl, d2, i2, _ = want
    df.from_grid(_up(G), stream=K.stream(), max_cells=7, inside=1)
    first, second = D.cost_config(**COST), D.cost_config(inscribed_radius=0.3, inflation_radius=1.7, cost_scaling_factor=1.0, track_unknown=0)
    costs = {k: D.costmap(cl, d2, _lut(c, RES), c) for k, c in (("first", first), ("second", second))}
    assert costs["first"].tobytes() != costs["second"].tobytes() and len(np.unique(costs["second"])) > 5
    metres = D.metres(cl, d2, i2, RES)
    for which in ("first", "second", "first"):
        c = df.costmap(RES, first if which == "first" else second, stream=K.stream())
        K.sync()
        DC.same_bytes(c.cpu().numpy(), costs[which], ("device", which))
    # a pinned block
    pm, pc = torch.zeros((h, w), dtype=torch.float32).pin_memory(), torch.zeros((h, w), dtype=torch.uint8).pin_memory()
    df.metres(RES, out=pm.data_ptr(), stream=K.stream())
    df.costmap(RES, second, out=pc.data_ptr(), stream=K.stream())
    K.sync()
    DC.same_bytes(pm.numpy(), metres, "pinned metres")
    DC.same_bytes(pc.numpy(), costs["second"], "pinned costmap")
    # device pointers 1, 2 and 3 bytes off a word
    for off in (1, 2, 3):
        bm = torch.full((h * w * 4 + 16,), 0xA5, dtype=torch.uint8, device=K.dev())
        bc = torch.full((h * w + 16,), 0xA5, dtype=torch.uint8, device=K.dev())
        df.metres(RES, out=bm.data_ptr() + off, stream=K.stream())
        df.costmap(RES, first, out=bc.data_ptr() + off, stream=K.stream())
        K.sync()
        hm, hc = bm.cpu().numpy(), bc.cpu().numpy()
        assert hm[off:off + h * w * 4].tobytes() == metres.tobytes() and hc[off:off + h * w].tobytes() == costs["first"].tobytes(), off
        assert (hm[:off] == 0xA5).all() and (hm[off + h * w * 4:] == 0xA5).all() and (hc[:off] == 0xA5).all() and (hc[off + h * w:] == 0xA5).all()
    # Rc = 8 at 0.25 m: the cap of 7 does not cover it
    before = df.fields(K.stream())
    with pytest.raises(Exception):
        df.costmap(RES, dict(inflation_radius=2.0), stream=K.stream())
    df.costmap(RES, dict(inflation_radius=1.75), stream=K.stream())          # (Rc = 7: covered)
    _holds(df, want, "after the refused costmap")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, df.fields(K.stream())))
    df.close()


# --- refusals -----------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_field_as_it_was(fx):
    import torch
    from lidar_feature_extraction_amd import DistanceField
    from lidar_feature_extraction_amd import binding as B
    L = fx._L
    for w, h in ((0, 4), (4, 0), (16385, 4), (4, 16385)):
        with pytest.raises(B.LfxError):
            DistanceField(fx, w, h)
    h, w = 20, 33
    df = DistanceField(fx, w, h)
    G = DC.random_grid(h, w, 0.02, seed=12)
    d_grid = _up(G)
    out = torch.zeros(h * w * 4, dtype=torch.uint8, device=K.dev())
    null, st = C.c_void_p(0), C.c_void_p(K.stream())
    # before any transform
    for call in (lambda: df.metres(RES, out=out.data_ptr()), lambda: df.costmap(RES, out=out.data_ptr()), lambda: df.stats()):
        with pytest.raises(B.LfxError):
            call()
    assert df.info()["transformed"] == 0
    want = DC.expected("errors", G, dict(max_cells=20), True)
    df.from_grid(d_grid, stream=K.stream(), max_cells=20, inside=1)
    _holds(df, want, "errors: the transform")
    bad_configs = [dict(occupied_percent=0), dict(occupied_percent=101), dict(unknown_is_obstacle=2), dict(max_cells=32768), dict(inside=2), dict(reserved=1)]
    for fields in bad_configs:
        with pytest.raises(B.LfxError):
            df.from_grid(d_grid, stream=K.stream(), **fields)
    for res in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(B.LfxError):
            df.metres(res, out=out.data_ptr(), stream=K.stream())
        with pytest.raises(B.LfxError):
            df.costmap(res, out=out.data_ptr(), stream=K.stream())
    for cost in (dict(inscribed_radius=-0.1), dict(inflation_radius=0.1), dict(cost_scaling_factor=float("nan")), dict(track_unknown=2),
                 dict(inflation_radius=300.0)):
        with pytest.raises(B.LfxError):
            df.costmap(RES, cost, out=out.data_ptr(), stream=K.stream())
    cfg, cost = B.DistanceConfig(), B.DistanceCostConfig()
    L.lfx_distance_default_config(C.byref(cfg))
    L.lfx_distance_cost_default_config(C.byref(cost))
    ctx, hd, po = fx._ctx, df.handle, C.c_void_p(out.data_ptr())
    assert L.lfx_distance_from_grid(ctx, hd, null, C.byref(cfg), st) == -1 and L.lfx_distance_from_grid(ctx, hd, C.c_void_p(d_grid.data_ptr()), None, st) == -1
    assert L.lfx_distance_from_grid(null, hd, C.c_void_p(d_grid.data_ptr()), C.byref(cfg), st) == -1
    assert L.lfx_distance_from_grid(ctx, null, C.c_void_p(d_grid.data_ptr()), C.byref(cfg), st) == -1
    assert L.lfx_distance_metres(ctx, hd, C.c_float(RES), null, st) == -1 and L.lfx_distance_metres(ctx, null, C.c_float(RES), po, st) == -1
    assert L.lfx_distance_costmap(ctx, hd, None, C.c_float(RES), po, st) == -1 and L.lfx_distance_costmap(ctx, hd, C.byref(cost), C.c_float(RES), null, st) == -1
    assert L.lfx_distance_stats(ctx, hd, None, st) == -1 and L.lfx_distance_view(ctx, hd, None, st) == -1 and L.lfx_distance_info(hd, None) == -1
    assert L.lfx_distance_from_occupancy(ctx, hd, null, None, C.byref(cfg), st) == -1
    assert L.lfx_distance_create(ctx, 4, 4, None) == -1
    L.lfx_distance_destroy(null)
    K.sync()
    assert not out.any()
    _holds(df, want, "errors: after the refusals")
    _outputs(df, want, 20, "errors: after the refusals")
    df.close()
