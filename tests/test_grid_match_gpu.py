"""lfx_grid_match_* on the device (include/lfx.h, the grid-match section) against the restatement
(tests/grid_match_restatement.py): the score field, the scans' points, scores, the search's best, slice_best and volume are
compared bit for bit -- nothing here has a tolerance.  tests/test_grid_match_expect.py holds the restatement to a brute force
and to hand values.  What the shapes are built around is named in tests/grid_match_cases.py."""
import ctypes as C

import numpy as np
import pytest

from tests import deskew_cases as K
from tests import grid_match_cases as GC
from tests import grid_match_restatement as G
from tests import occupancy_cases as OC
from tests import segment_cases as S

pytestmark = pytest.mark.gpu
RES, ORIGIN = 0.25, (-30.5, -20.25)
WORLD = (300, 257)                                           # width, height


@pytest.fixture(scope="module")
def fx():
    f = K.fx_for(16, 64, 4)
    yield f
    f.close()


@pytest.fixture(scope="module")
def hold():
    return S.Hold()


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(K.dev())


def _geom(w, h, res=RES, origin=ORIGIN):
    return G.geometry(w, h, res, *origin)


def _matcher(fx, geom, **fields):
    from lidar_feature_extraction_amd import GridMatcher
    return GridMatcher(fx, geom["width"], geom["height"], geom["resolution"], (geom["origin_x"], geom["origin_y"]), **fields)


def _distance(fx, grid, **fields):
    """a DistanceField holding the transform of an int8 grid, and its d2 on the host"""
    from lidar_feature_extraction_amd import DistanceField
    df = DistanceField(fx, grid.shape[1], grid.shape[0])
    df.from_grid(_up(grid), stream=K.stream(), **fields)
    return df, df.fields(K.stream())[1]


def _random_lut(rs, seed, peak=1000):
    return np.random.default_rng(seed).integers(0, peak + 1, rs * rs + 1).astype(np.uint16)


@pytest.fixture(scope="module")
def world(fx):
    """a matcher over 300 x 257 cells whose field takes a random table of Rs = 64 through the distances to a few hundred
    obstacles: every cell its own value; (matcher, S on the host, geometry), the field checked where it is made"""
    w, h = WORLD
    geom = _geom(w, h)
    df, d2 = _distance(fx, GC.random_grid(h, w, 0.003, seed=21))
    lut = _random_lut(64, seed=22)
    m = _matcher(fx, geom, max_scans=40, max_beams=4096, max_half_x=64, max_half_y=64, max_half_theta=3)
    m.set_field(df, lut, stream=K.stream())
    Sh = G.field(d2, lut)
    GC.same_bytes(m.field(K.stream()), Sh, "the world's field")
    assert len(np.unique(Sh)) > 300                       # (the test's own data: a few hundred different values, not a handful)
    yield m, Sh, geom
    m.close()
    df.close()


def _set(m, xyz, kind, levels=None):
    m.set_scans(_up(GC.pack_beams(xyz, kind)), levels=levels, stream=K.stream())
    return G.points(xyz, kind, levels)


def _search(m, Sh, geom, pts, centres, cfg, first=0, what=""):
    """one search with every output against the restatement's, and once more with none but the best"""
    want = G.search(Sh, pts, centres, cfg, geom)
    best, sl, vol = m.search(centres, cfg, first=first, slice_best=True, volume=True, stream=K.stream())
    alone, none_sl, none_vol = m.search(centres, cfg, first=first, stream=K.stream())
    K.sync()
    assert none_sl is None and none_vol is None
    GC.same_bytes(GC.as_u32(vol), want[2], (what, "volume"))
    GC.same_bytes(GC.as_u32(sl), want[1], (what, "slice_best"))
    GC.same_bytes(GC.as_u32(best), want[0], (what, "best"))
    GC.same_bytes(GC.as_u32(alone), want[0], (what, "best alone"))
    return want


# --- the field ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", GC.FIELD_SIZES + [GC.FIELD_STRIDE_SIZE], ids=lambda s: "%dx%d" % s)
def test_field(fx, size):
    w, h = size
    grid = GC.random_grid(h, w, 0.004 if w * h > 4 else 1.0, seed=w)
    if w * h > 4:
        grid[0, 0] = 100
    m = _matcher(fx, _geom(w, h))
    seen = set()
    for cap, tables in ((0, (0, 2, 64)), (70, (0, 2, 64)), (3, (0, 2))):         # (a cap of 3 cells covers Rs = 2, and leaves FAR cells)
        df, d2 = _distance(fx, grid, max_cells=cap)
        for rs in tables:
            lut = _random_lut(rs, seed=rs) + 1
            m.set_field(df, lut, stream=K.stream())
            GC.same_bytes(m.field(K.stream()), G.field(d2, lut), (size, cap, rs))
            assert m.info()["field_set"] == 1 and m.info()["table_cells"] == rs
            if rs == 2:
                seen |= {int(v) for v in np.unique(d2) if v in (0, 4, 5, G.FAR)}
        df.close()
    if w * h > 300:
        assert seen == {0, 4, 5, G.FAR}, seen              # d2 of 0, n - 1, n and FAR have all been looked up
    # the library's own table at the defaults goes the same way
    df, d2 = _distance(fx, grid)
    m.set_field(df, stream=K.stream())
    from lidar_feature_extraction_amd import grid_match_table
    GC.same_bytes(m.field(K.stream()), G.field(d2, grid_match_table(None, RES)), (size, "default table"))
    df.close()
    m.close()


def test_field_refusals(fx):
    from lidar_feature_extraction_amd import DistanceField
    from lidar_feature_extraction_amd import binding as B
    w, h = 67, 5
    grid = GC.random_grid(h, w, 0.02, seed=5)
    m = _matcher(fx, _geom(w, h))
    df, d2 = _distance(fx, grid, max_cells=3)
    m.set_field(df, _random_lut(3, 1), stream=K.stream())                        # (covered: Rs = 3)
    before = m.field(K.stream())
    fresh, other = DistanceField(fx, w, h), DistanceField(fx, w, h + 1)
    other.from_grid(_up(GC.random_grid(h + 1, w, 0.02, seed=6)), stream=K.stream())
    for call in (lambda: m.set_field(df, _random_lut(4, 1), stream=K.stream()),  # the transform's cap of 3 is below Rs = 4
                 lambda: m.set_field(other, _random_lut(3, 1), stream=K.stream()),
                 lambda: m.set_field(fresh, _random_lut(3, 1), stream=K.stream()),
                 lambda: m.set_field(df, np.zeros(11, np.uint16), stream=K.stream()),
                 lambda: m.set_field(df, np.zeros(65 * 65 + 1, np.uint16), stream=K.stream()),
                 lambda: m.set_field(df, np.zeros(0, np.uint16), stream=K.stream())):
        with pytest.raises(B.LfxError):
            call()
    GC.same_bytes(m.field(K.stream()), before, "the field after the refusals")
    assert m.info()["table_cells"] == 3
    for bad in (dict(max_scans=0), dict(max_scans=1025), dict(max_beams=3), dict(max_beams=4097), dict(max_half_x=257), dict(max_half_y=257),
                dict(max_half_theta=181)):
        with pytest.raises(B.LfxError):
            _matcher(fx, _geom(w, h), **bad)
    for geom in (_geom(0, 4), _geom(4, 16385), _geom(4, 4, res=0.0), _geom(4, 4, origin=(float("nan"), 0.0))):
        with pytest.raises(B.LfxError):
            _matcher(fx, geom)
    for o in (fresh, other, df, m):
        o.close()


# --- the scans ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_hit", GC.HIT_COUNTS)
def test_scans(world, n_hit):
    m, Sh, geom = world
    xyz, kind = GC.beams(3, 4096, n_hit, seed=n_hit)
    tilted = OC.tilted_poses(3, seed=n_hit)[:, :, :3].copy()
    broken = tilted.copy()
    broken[1, 0, 2] = float("nan")                                               # a level product that is no number: scan 1 keeps nothing
    broken[2, 1, 1] = float("inf")
    for name, levels in (("identity", None), ("tilted", tilted), ("broken", broken)):
        want = _set(m, xyz, kind, levels)
        got = m.points(K.stream())
        assert [len(p) for p in got] == [len(p) for p in want], (name, n_hit)
        for s in range(3):
            GC.same_bytes(got[s], want[s], (name, n_hit, s))
        assert m.info()["n_scans"] == 3 and m.info()["n_beams"] == 4096
        if name == "identity":
            assert [len(p) for p in want] == [n_hit] * 3
        if name == "broken" and n_hit:
            assert len(want[1]) == 0 and len(want[0]) == n_hit


# --- score ----------------------------------------------------------------------------------------------------------------------------
def _border_scan(geom, W):
    """16 HIT beams whose points are the middles of the cells one outside, first and last inside, on either axis"""
    xyz, kind = np.zeros((1, W, 3), np.float32), np.zeros((1, W), np.uint32)
    k = 0
    for cx in (-1, 0, geom["width"] - 1, geom["width"]):
        for cy in (-1, 0, geom["height"] - 1, geom["height"]):
            xyz[0, k] = (geom["origin_x"] + (cx + 0.5) * geom["resolution"], geom["origin_y"] + (cy + 0.5) * geom["resolution"], 0.0)
            kind[0, k] = GC.HIT
            k += 1
    return xyz, kind


@pytest.mark.parametrize("P", GC.SCORE_P)
def test_score(world, P):
    m, Sh, geom = world
    xyz, kind = GC.beams(2, 2500, 2100, seed=P)                                  # (2100 points: three rounds through LDS)
    bx, bk = _border_scan(geom, 2500)
    xyz, kind = np.concatenate([xyz, bx]), np.concatenate([kind, bk])
    pts = _set(m, xyz, kind)
    cand = GC.candidates(P, geom, seed=P, reach=40.0)
    far = 2.0 ** 30 * geom["resolution"]
    specials = np.array([[float("nan"), 0, 1, 0], [0, float("inf"), 1, 0], [0, float("-inf"), 1, 0], [far + 100.0, 0, 1, 0], [0, -far - 100.0, 1, 0],
                         [0, 0, float("nan"), 0], [0, 0, 1, float("inf")], [0.0, 0.0, 1.0, 0.0]])
    cand[:min(P, len(specials))] = specials[-min(P, len(specials)):]
    for scan in range(3):
        sc, ins = m.score(scan, cand, stream=K.stream())
        only, none = m.score(scan, _up(cand), inside=False, stream=K.stream())
        K.sync()
        want = G.score(Sh, pts[scan], cand, geom)
        GC.same_bytes(GC.as_u32(sc), want[0], (P, scan, "score"))
        GC.same_bytes(GC.as_u32(ins), want[1], (P, scan, "inside"))
        GC.same_bytes(GC.as_u32(only), want[0], (P, scan, "score alone"))
        assert none is None
        assert want[1].max() > 0 and want[0].max() > 0
    # the border scan under the identity: 4 of its 16 points are inside, by hand
    sc, ins = m.score(2, np.array([[0.0, 0.0, 1.0, 0.0]]), stream=K.stream())
    K.sync()
    assert GC.as_u32(ins).tolist() == [4]
    w, h = geom["width"], geom["height"]
    assert GC.as_u32(sc).tolist() == [int(Sh[0, 0]) + int(Sh[0, w - 1]) + int(Sh[h - 1, 0]) + int(Sh[h - 1, w - 1])]


def test_score_at_its_largest(fx):
    """lut[0] = 65535 on a grid of obstacles only, 4096 points inside: 4096 * 65535 in 32 bits"""
    w, h = 67, 5
    geom = _geom(w, h)
    df, d2 = _distance(fx, np.full((h, w), 100, np.int8))
    m = _matcher(fx, geom, max_scans=1, max_beams=4096)
    m.set_field(df, np.array([65535], np.uint16), stream=K.stream())
    rng = np.random.default_rng(4)
    xyz = np.zeros((1, 4096, 3), np.float32)
    xyz[0, :, 0] = rng.uniform(ORIGIN[0] + 0.1, ORIGIN[0] + w * RES - 0.1, 4096)
    xyz[0, :, 1] = rng.uniform(ORIGIN[1] + 0.1, ORIGIN[1] + h * RES - 0.1, 4096)
    m.set_scans(_up(GC.pack_beams(xyz, np.full((1, 4096), GC.HIT, np.uint32))), stream=K.stream())
    sc, ins = m.score(0, np.array([[0.0, 0.0, 1.0, 0.0]]), stream=K.stream())
    best, _, _ = m.search([[0.0, 0.0, 0.0]], dict(half_x=0, half_y=0), stream=K.stream())
    K.sync()
    assert GC.as_u32(sc).tolist() == [268431360] and GC.as_u32(ins).tolist() == [4096]
    assert GC.as_u32(best).tolist() == [[268431360, 0, 4096, 4096]]
    m.close()
    df.close()


# --- search ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", GC.WINDOWS, ids=lambda w: "%dx%dx%d_step%d" % (2 * w[0] + 1, 2 * w[1] + 1, 2 * w[2] + 1, w[3]))
def test_search_windows(world, window):
    m, Sh, geom = world
    cfg = GC.window(*window)
    xyz, kind = GC.beams(2, 300, 200, seed=sum(window), reach=15.0)
    pts = _set(m, xyz, kind, GC.yaw_levels(2, seed=3))
    mid = (ORIGIN[0] + 0.5 * WORLD[0] * RES, ORIGIN[1] + 0.5 * WORLD[1] * RES)
    centres = [[mid[0] + 1.3, mid[1] - 0.7, 0.3], [ORIGIN[0] + 2.0, ORIGIN[1] + WORLD[1] * RES - 1.0, -2.0]]       # the middle, and a corner
    want = _search(m, Sh, geom, pts, centres, cfg, what=window)
    assert want[0][0, 0] > 0 and want[0][0, 2] > 100 and 0 < want[0][1, 2] < 200
    # the centre candidate of every heading is `score` at the centre under that heading
    for k in range(2):
        cs = G.rotations(centres[k][2], cfg["half_theta"], cfg["theta_step"])
        sc, _ = m.score(k, np.array([[centres[k][0], centres[k][1], c, s] for c, s in cs]), stream=K.stream())
        K.sync()
        assert GC.as_u32(sc).tolist() == want[2][k, :, cfg["half_y"], cfg["half_x"]].tolist(), (window, k)
    # the second scan alone, as scan `first` = 1 of the object
    _search(m, Sh, geom, pts[1:], centres[1:], cfg, first=1, what=(window, "first = 1"))


def test_search_overhangs_and_an_empty_scan(world):
    """windows of 65 x 65 x 3 at 3 cells a step around centres near each side of the grid, one far outside it, and a scan
    without a HIT beam"""
    m, Sh, geom = world
    xyz, kind = GC.beams(6, 300, 150, seed=77, reach=12.0)
    kind[5][kind[5] == GC.HIT] = GC.CLEAR
    pts = _set(m, xyz, kind)
    x0, y0, x1, y1 = ORIGIN[0], ORIGIN[1], ORIGIN[0] + WORLD[0] * RES, ORIGIN[1] + WORLD[1] * RES
    centres = [[x0 - 5.0, 0.5 * (y0 + y1), 0.1], [x1 + 5.0, 0.5 * (y0 + y1), 0.2], [0.5 * (x0 + x1), y0 - 5.0, 0.3], [0.5 * (x0 + x1), y1 + 5.0, 0.4],
               [x1 + 4000.0, y1 + 4000.0, 0.5], [0.5 * (x0 + x1), 0.5 * (y0 + y1), 0.0]]
    want = _search(m, Sh, geom, pts, centres, GC.window(32, 32, 1, 3), what="overhangs")
    assert all(want[0][k, 0] > 0 for k in range(4))
    assert want[0][4].tolist() == [0, 0, 0, 150] and want[0][5].tolist() == [0, 0, 0, 0] and len(pts[5]) == 0


def test_search_33_scans_in_one_call(world):
    m, Sh, geom = world
    xyz, kind = GC.beams(33, 64, 40, seed=33, reach=10.0)
    pts = _set(m, xyz, kind, GC.yaw_levels(33, seed=34))
    rng = np.random.default_rng(35)
    centres = np.stack([rng.uniform(ORIGIN[0], ORIGIN[0] + WORLD[0] * RES, 33), rng.uniform(ORIGIN[1], ORIGIN[1] + WORLD[1] * RES, 33),
                        rng.uniform(-3, 3, 33)], axis=1)
    cfg = GC.window(2, 2, 1, 1)
    want = _search(m, Sh, geom, pts, centres, cfg, what="33 scans")
    assert len({tuple(r) for r in want[0].tolist()}) > 25
    _search(m, Sh, geom, pts[:1], centres[:1], cfg, what="1 scan")
    _search(m, Sh, geom, pts[7:9], centres[7:9], cfg, first=7, what="2 scans")


def test_equal_maxima_go_to_the_lowest_index(fx):
    """four obstacles in a square and one point in its middle: four candidates of 7, the lowest index wins"""
    geom = G.geometry(9, 9, 1.0)
    grid = np.zeros((9, 9), np.int8)
    grid[2, 2] = grid[2, 6] = grid[6, 2] = grid[6, 6] = 100
    df, d2 = _distance(fx, grid)
    m = _matcher(fx, geom, max_scans=1, max_beams=4, max_half_x=3, max_half_y=3, max_half_theta=0)
    m.set_field(df, np.array([7], np.uint16), stream=K.stream())
    xyz, kind = np.zeros((1, 4, 3), np.float32), np.zeros((1, 4), np.uint32)
    xyz[0, 2], kind[0, 2] = (4.5, 4.5, 0.0), GC.HIT
    pts = _set(m, xyz, kind)
    Sh = G.field(d2, [7])
    want = _search(m, Sh, geom, pts, [[0.0, 0.0, 0.0]], G.search_config(half_x=3, half_y=3), what="equal maxima")
    assert want[0][0].tolist() == [7, 8, 1, 1] and (want[2] == 7).sum() == 4
    m.close()
    df.close()


def test_refusals_leave_the_object_as_it_was(world):
    from lidar_feature_extraction_amd import binding as B
    m, Sh, geom = world
    xyz, kind = GC.beams(2, 64, 30, seed=9)
    pts = _set(m, xyz, kind)
    before, info = m.points(K.stream()), m.info()
    d_beams = _up(GC.pack_beams(xyz, kind))
    cand = _up(GC.candidates(4, geom, 1))
    mid = [0.0, 0.0, 0.0]
    calls = [lambda: m.set_scans(d_beams.data_ptr(), 0, 64), lambda: m.set_scans(d_beams.data_ptr(), 2, 0), lambda: m.set_scans(d_beams.data_ptr(), 41, 2),
             lambda: m.set_scans(d_beams.data_ptr(), 1, 4097), lambda: m.score(2, cand), lambda: m.search([mid], first=2), lambda: m.search([mid, mid, mid]),
             lambda: m.search([mid], half_x=65), lambda: m.search([mid], half_y=65), lambda: m.search([mid], half_theta=4, theta_step=0.1),
             lambda: m.search([mid], step_cells=0), lambda: m.search([mid], step_cells=17), lambda: m.search([mid], half_theta=1, theta_step=0.0),
             lambda: m.search([[float("nan"), 0.0, 0.0]]), lambda: m.search([[0.0, 0.0, float("inf")]])]
    for k, call in enumerate(calls):
        with pytest.raises(B.LfxError):
            call()
    L, null, st = m._L, C.c_void_p(0), C.c_void_p(K.stream())
    ctx, hd = m._fx._ctx, m.handle
    assert L.lfx_grid_match_score(ctx, hd, 0, null, 4, C.c_void_p(cand.data_ptr()), null, st) == -1
    assert L.lfx_grid_match_score(ctx, hd, 0, C.c_void_p(cand.data_ptr()), 0, C.c_void_p(cand.data_ptr()), null, st) == -1
    assert L.lfx_grid_match_score(ctx, hd, 0, C.c_void_p(cand.data_ptr()), (1 << 24) + 1, C.c_void_p(cand.data_ptr()), null, st) == -1
    assert L.lfx_grid_match_search(ctx, hd, 0, 1, null, None, null, null, null, st) == -1 and L.lfx_grid_match_info(hd, None) == -1
    assert L.lfx_grid_match_set_scans(ctx, hd, null, 1, 4, null, st) == -1 and L.lfx_grid_match_set_field(ctx, hd, null, null, 1, st) == -1
    assert L.lfx_grid_match_set_scans_occupancy(ctx, hd, null, 0, 1, 1, st) == -1 and L.lfx_grid_match_view(ctx, hd, None, st) == -1
    assert L.lfx_grid_match_create(ctx, None, None) == -1
    L.lfx_grid_match_destroy(null)
    after = m.points(K.stream())
    assert m.info() == info and all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    GC.same_bytes(m.field(K.stream()), Sh, "the field after the refusals")
    # a matcher without a field or scans refuses to score and search
    fresh = _matcher(m._fx, geom)
    for call in (lambda: fresh.score(0, cand), lambda: fresh.search([mid])):
        with pytest.raises(B.LfxError):
            call()
    assert fresh.info()["field_set"] == 0 and fresh.info()["n_scans"] == 0 and fresh.info()["device_bytes"] >= 2 * WORLD[0] * WORLD[1]
    fresh.close()


# --- end to end, the store's scans, truncate -------------------------------------------------------------------------------------------
def _occupancy(fx, cfg):
    from lidar_feature_extraction_amd import OccupancyGrid
    return OccupancyGrid(fx, cfg.width, cfg.height, cfg.resolution, (cfg.origin_x, cfg.origin_y), cfg.max_scans, config=cfg)


def test_end_to_end_on_the_room(fx):
    """add_batch, render, from_occupancy, set_field, set_scans_occupancy, then a search from a centre 3 cells and 2 heading
    steps off: the conditions tests/test_grid_match_expect.py checks on the restatement, on the device"""
    from lidar_feature_extraction_amd import DistanceField, grid_match_candidate, grid_match_table
    cfg = GC.e2e_config()
    geom = G.geometry(cfg.width, cfg.height, cfg.resolution, cfg.origin_x, cfg.origin_y)
    clouds, poses = GC.e2e_scans()
    g = _occupancy(fx, cfg)
    d = S.device_batch(fx, clouds)
    assert g.add_batch(poses, stream=K.stream()) == 0
    g.render(stream=K.stream())
    df = DistanceField(fx, cfg.width, cfg.height)
    df.from_occupancy(g, stream=K.stream())
    m = _matcher(fx, geom, max_scans=4, max_beams=GC.E2E_BEAMS, max_half_x=5, max_half_y=4, max_half_theta=3)
    m.set_field(df, stream=K.stream())
    lut = grid_match_table(None, cfg.resolution)
    Sh = G.field(df.fields(K.stream())[1], lut)
    GC.same_bytes(m.field(K.stream()), Sh, "the room's field")
    # the store's scans under the store's rotations are set_scans of the view's beams with the poses read back
    m.set_scans_occupancy(g, stream=K.stream())
    xyz, kind = g.beams(K.stream())
    stored = g.poses(stream=K.stream())
    want = G.points(xyz, kind, stored[:, :, :3])
    got = m.points(K.stream())
    for s in range(4):
        GC.same_bytes(got[s], want[s], ("the store's scans", s))
    m.set_scans(_up(GC.pack_beams(xyz, kind)), levels=stored[:, :, :3], stream=K.stream())
    for s, p in enumerate(m.points(K.stream())):
        GC.same_bytes(p, want[s], ("the view's beams", s))
    m.set_scans_occupancy(g, use_rotation=False, stream=K.stream())
    for s, p in enumerate(m.points(K.stream())):
        GC.same_bytes(p, G.points(xyz, kind)[s], ("without the rotations", s))
    # every scan at its own stored pose: n_points * lut[0]
    m.set_scans_occupancy(g, stream=K.stream())
    for s in range(4):
        sc, ins = m.score(s, np.array([[stored[s][0, 3], stored[s][1, 3], 1.0, 0.0]]), stream=K.stream())
        K.sync()
        assert GC.as_u32(sc).tolist() == [GC.E2E_BEAMS * int(lut[0])] and GC.as_u32(ins).tolist() == [GC.E2E_BEAMS]
    # the query scan alone, from the wrong centre
    m.set_scans_occupancy(g, GC.E2E_QUERY, 1, stream=K.stream())
    window = G.search_config(**GC.E2E_WINDOW)
    centre = GC.e2e_centre(poses)
    res = _search(m, Sh, geom, [want[GC.E2E_QUERY]], [centre], window, what="the room")
    true = GC.e2e_true_index()
    assert res[2][0].reshape(-1)[true] == GC.E2E_BEAMS * int(lut[0]) == res[0][0, 0] == res[2][0].max() and res[0][0, 1] <= true
    GC.same_bytes(grid_match_candidate(window, cfg.resolution, centre, int(res[0][0, 1])), G.candidate(window, cfg.resolution, centre, int(res[0][0, 1])), "candidate")
    for o in (m, df, g):
        o.close()
    del d


def test_truncate(fx):
    """truncate(0) and the same batch added again: ids from 0, the same beams, the counts untouched; a count above the store's
    is refused"""
    from lidar_feature_extraction_amd import binding as B
    cfg = GC.e2e_config()
    clouds, poses = GC.e2e_scans()
    g = _occupancy(fx, cfg)
    d = S.device_batch(fx, clouds)
    assert g.add_batch(poses, stream=K.stream()) == 0
    g.render(stream=K.stream())
    xyz, kind = g.beams(K.stream())
    hits, misses = g.counts(K.stream())
    assert hits.any() and len(g) == 4
    with pytest.raises(B.LfxError):
        g.truncate(5)
    assert len(g) == 4
    g.truncate(3)
    assert len(g) == 3
    g.truncate(0)
    assert len(g) == 0 and g.beams(K.stream())[0].shape[0] == 0
    moved = poses.copy()
    moved[:, 0, 3] += 1.0
    assert g.add_batch(moved, stream=K.stream()) == 0 and len(g) == 4
    again = g.beams(K.stream())
    OC.same_bytes(again[0], xyz, "the beams after truncate and add")
    OC.same_bytes(again[1], kind, "the kinds after truncate and add")
    OC.same_bytes(g.poses(stream=K.stream()), moved, "the poses after truncate and add")
    after = g.counts(K.stream())
    OC.same_bytes(after[0], hits, "hits")
    OC.same_bytes(after[1], misses, "misses")
    g.truncate(2)
    assert len(g) == 2 and g.add_batch(poses[:4], select=[0, 1, 0, 0], stream=K.stream()) == 2 and len(g) == 3
    OC.same_bytes(g.beams(K.stream())[0][2], xyz[1], "the scan added at id 2")
    g.close()
    del d


def test_a_reducer_grid_feeds_live_scans(fx):
    """a second grid of 1 x 1 cells as the reducer of live batches: truncate(0), add_batch, set_scans_occupancy -- the points
    are those of the map's own store for the same scans"""
    cfg = GC.e2e_config()
    geom = G.geometry(cfg.width, cfg.height, cfg.resolution, cfg.origin_x, cfg.origin_y)
    clouds, poses = GC.e2e_scans()
    small = OC.hand_config(GC.E2E_BEAMS, 1, 1, max_range=60.0, max_scans=4)
    g, r = _occupancy(fx, cfg), _occupancy(fx, small)
    m = _matcher(fx, geom, max_scans=4, max_beams=GC.E2E_BEAMS)
    d = S.device_batch(fx, clouds)
    g.add_batch(poses, stream=K.stream())
    m.set_scans_occupancy(g, stream=K.stream())
    want = m.points(K.stream())
    for turn in range(2):
        r.truncate(0)
        assert r.add_batch(poses, stream=K.stream()) == 0
        m.set_scans_occupancy(r, stream=K.stream())
        for s, p in enumerate(m.points(K.stream())):
            GC.same_bytes(p, want[s], ("the reducer", turn, s))
    for o in (m, r, g):
        o.close()
    del d


# --- streams --------------------------------------------------------------------------------------------------------------------------
def test_producers_on_another_stream(fx, hold):
    """The field's transform and the store's add queued on a held stream A, then at once set_field, set_scans_occupancy and a
    search on B: the search sees both, through the two objects' events."""
    from lidar_feature_extraction_amd import DistanceField, grid_match_table
    cfg = GC.e2e_config()
    geom = G.geometry(cfg.width, cfg.height, cfg.resolution, cfg.origin_x, cfg.origin_y)
    clouds, poses = GC.e2e_scans()
    g = _occupancy(fx, cfg)
    d = S.device_batch(fx, clouds)
    grid = GC.random_grid(cfg.height, cfg.width, 0.01, seed=50)
    d_grid = _up(grid)
    df = DistanceField(fx, cfg.width, cfg.height)
    m = _matcher(fx, geom, max_scans=4, max_beams=GC.E2E_BEAMS, max_half_x=5, max_half_y=4, max_half_theta=3)
    window = G.search_config(**GC.E2E_WINDOW)
    centres = [[40.0, 20.0, 0.1 * k] for k in range(4)]
    K.sync()
    a, b = S.two_streams()
    hold(a)
    df.from_grid(d_grid, stream=a.cuda_stream)
    g.add_batch(poses, stream=a.cuda_stream)
    e = S.event_behind(a)
    hold.still_held(e, "grid match: producers on A, the matcher on B")
    m.set_field(df, stream=b.cuda_stream)
    m.set_scans_occupancy(g, stream=b.cuda_stream)
    best, sl, vol = m.search(centres, window, slice_best=True, volume=True, stream=b.cuda_stream)
    g.truncate(0)
    K.sync()
    d2 = df.fields(K.stream())[1]
    Sh = G.field(d2, grid_match_table(None, cfg.resolution))
    assert len(g) == 0 and g.add_batch(poses, stream=K.stream()) == 0
    xyz, kind = g.beams(K.stream())
    pts = G.points(xyz, kind, poses[:, :, :3])
    want = G.search(Sh, pts, centres, window, geom)
    assert want[0][:, 0].min() > 0
    GC.same_bytes(GC.as_u32(best), want[0], "two streams: best")
    GC.same_bytes(GC.as_u32(sl), want[1], "two streams: slice_best")
    GC.same_bytes(GC.as_u32(vol), want[2], "two streams: volume")
    for o in (m, df, g):
        o.close()
    del d


def test_a_transform_on_the_other_stream_waits_for_a_held_set_field(fx, hold):
    """The reader's half of the two-object call: a set_field queued on a held stream B records the distance field's event
    too, so a transform of another grid into the same field, issued on A while B is still held, does not reach d2 before the
    look-up has read it."""
    from lidar_feature_extraction_amd import DistanceField, grid_match_table
    cfg = GC.e2e_config()
    geom = G.geometry(cfg.width, cfg.height, cfg.resolution, cfg.origin_x, cfg.origin_y)
    d_first = _up(GC.random_grid(cfg.height, cfg.width, 0.01, seed=50))
    d_second = _up(GC.random_grid(cfg.height, cfg.width, 0.01, seed=51))
    df = DistanceField(fx, cfg.width, cfg.height)
    m = _matcher(fx, geom, max_scans=4, max_beams=GC.E2E_BEAMS)
    df.from_grid(d_first, stream=K.stream())
    d2 = df.fields(K.stream())[1]
    K.sync()
    a, b = S.two_streams()
    hold(b)
    m.set_field(df, stream=b.cuda_stream)
    e = S.event_behind(b)
    hold.still_held(e, "grid match: set_field on B, a transform into its field on A")
    df.from_grid(d_second, stream=a.cuda_stream)
    got = m.field(b.cuda_stream)
    K.sync()
    GC.same_bytes(got, G.field(d2, grid_match_table(None, cfg.resolution)), "a held reader: the first transform's field")
    assert (df.fields(K.stream())[1] != d2).any()            # (and the second transform did run)
    m.close()
    df.close()
