"""The occupancy restatement (tests/occupancy_restatement.py) held to cases worked out by hand from include/lfx.h, the
occupancy section: the lines of tests/occupancy_cases.py cell by cell, the votes of one and of two scans, the column winners on
ties, the height band and the range gates at equality and one float on either side, the column boundaries (the probes of the
segmentation's hand tests), a direction that a tilted pose makes vertical, the emit at its clamps, and the PGM's bytes.  No
device: the tables are the library's (host only).  tests/test_occupancy_gpu.py holds the device to the same restatement."""
import numpy as np
import pytest

from tests import occupancy_cases as OC
from tests import occupancy_restatement as O
from tests import segment_restatement as R
from tests.test_segment_hand_gpu import ALONE, _boundary_records, _four_column_cases, _sign_records

f32 = np.float32


def _up(v):
    return np.nextafter(f32(v), f32(np.inf))


def _down(v):
    return np.nextafter(f32(v), f32(-np.inf))


def test_lines_by_hand():
    """line_cells against the cell lists written out in the cases (the free cells in order, then the end cell)."""
    assert O.line_cells(10, 10, 15, 10) == OC.row(10, 10, 15)
    assert O.line_cells(10, 10, 10, 6) == [(10, 10), (10, 9), (10, 8), (10, 7), (10, 6)]
    assert O.line_cells(10, 10, 13, 13) == [(10, 10), (11, 11), (12, 12), (13, 13)]
    assert O.line_cells(10, 10, 14, 12) == [(10, 10), (11, 10), (12, 11), (13, 11), (14, 12)]
    assert O.line_cells(10, 10, 12, 14) == [(10, 10), (10, 11), (11, 12), (11, 13), (12, 14)]
    assert O.line_cells(10, 10, 6, 8) == [(10, 10), (9, 10), (8, 9), (7, 9), (6, 8)]
    assert O.line_cells(10, 10, 10, 10) == [(10, 10)]
    assert O.line_cells(-3, 5, 3, 5) == OC.row(5, -3, 3)


def test_lines_end_where_they_should():
    """max(ax, ay) + 1 cells, the first the origin, the last the end, every step to one of the 8 neighbours -- 2 000 lines."""
    rng = np.random.default_rng(3)
    for _ in range(2000):
        ox, oy, ex, ey = (int(v) for v in rng.integers(-40, 40, 4))
        cells = O.line_cells(ox, oy, ex, ey)
        assert len(cells) == max(abs(ex - ox), abs(ey - oy)) + 1 and cells[0] == (ox, oy) and cells[-1] == (ex, ey)
        assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) == 1 for a, b in zip(cells, cells[1:]))


@pytest.mark.parametrize("grid", OC.HAND_GRIDS)
@pytest.mark.parametrize("W", OC.HAND_BEAMS)
@pytest.mark.parametrize("name", sorted(OC.HAND))
def test_hand_cases(name, W, grid):
    cfg = OC.hand_config(W, *grid)
    clouds, poses = OC.hand_scans(name)
    g = O.Grid(cfg)
    g.add_scans(clouds, poses)
    xyz, kind = g.beams()
    n_records = sum(len(recs) for _, recs in OC.HAND[name][0])
    assert int((kind != O.NONE).sum()) == n_records                       # (every record of a case is a beam of its own)
    g.render()
    hits, misses = OC.hand_counts(name, *grid)
    OC.same_bytes(g.hits, hits, (name, "hits"))
    OC.same_bytes(g.misses, misses, (name, "misses"))
    assert g.counters["n_occupied_votes"] == int(hits.sum()) and g.counters["n_free_votes"] == int(misses.sum())
    assert g.counters["n_hit_beams"] + g.counters["n_clear_beams"] == n_records
    assert g.counters["n_skipped_beams"] == 0 and g.counters["n_window_miss"] == 0
    # render accumulates; clear and render gives the same again
    g.render()
    OC.same_bytes(g.hits, 2 * hits, (name, "twice"))
    g.clear()
    g.render()
    OC.same_bytes(g.misses, misses, (name, "again"))


def test_the_vectorised_walk_is_the_scalar_one():
    """scan_votes walks all beams of a scan in step; its cells are line_cells's."""
    cfg = OC.hand_config(16, 40, 40)
    rng = np.random.default_rng(7)
    xyz = np.zeros((16, 3), np.float32)
    xyz[:, :2] = rng.uniform(-19, 19, (16, 2))
    kind = rng.integers(0, 3, 16).astype(np.uint32)
    pose = OC.pose_at(17.3, 22.9)
    occupied, free, res = O.scan_votes(cfg, xyz, kind, pose)
    want_o, want_p = np.zeros((40, 40), bool), np.zeros((40, 40), bool)
    for b in range(16):
        if kind[b] == O.NONE:
            continue
        cells = O.line_cells(17, 22, int(np.floor(17.3 + float(xyz[b, 0]))), int(np.floor(22.9 + float(xyz[b, 1]))))
        for i, (x, y) in enumerate(cells):
            if 0 <= x < 40 and 0 <= y < 40:
                (want_o if (i == len(cells) - 1 and kind[b] == O.HIT) else want_p)[y, x] = True
    assert (occupied == want_o).all() and (free == (want_p & ~want_o)).all() and occupied.any() and free.any()
    assert res["n_hit_beams"] == int((kind == O.HIT).sum()) and res["n_clear_beams"] == int((kind == O.CLEAR).sum())


def _one(cfg, records, pose=None, **kw):
    """the beams of one scan of (x, y, z) records under an unrotated pose: (xyz, kind)"""
    a = np.array(records, np.float32).reshape(-1, 3)
    return O.reduce_scan(cfg, a[:, 0], a[:, 1], a[:, 2], OC.pose_at(0, 0) if pose is None else pose, **kw)


def test_ties_go_to_the_lower_index():
    """Two records of one column with the same kf (x and y equal; z does not enter it) -- the winner's z tells which won."""
    cfg = OC.hand_config(8)
    for a, b, kind in ((0.0, 0.25, O.HIT), (0.25, 0.0, O.HIT), (2.0, 3.0, O.CLEAR), (3.0, 2.0, O.CLEAR)):
        xyz, k = _one(cfg, [(3, 0.1, a), (3, 0.1, b)])
        m = np.flatnonzero(k)
        assert len(m) == 1 and k[m[0]] == kind and xyz[m[0]].tolist() == [3.0, f32(0.1), a]
    # without a tie: the nearest obstacle, the farthest clear record; an obstacle beats any clear record
    xyz, k = _one(cfg, [(4, 0.1, 0), (3, 0.1, 0), (5, 0.1, 0)])
    assert xyz[np.flatnonzero(k)[0], 0] == 3.0
    xyz, k = _one(cfg, [(4, 0.1, 2), (6, 0.1, 2), (5, 0.1, 2)])
    assert xyz[np.flatnonzero(k)[0], 0] == 6.0 and k.max() == O.CLEAR
    xyz, k = _one(cfg, [(9, 0.1, 2), (6, 0.1, 0)])
    assert xyz[np.flatnonzero(k)[0], 0] == 6.0 and k.max() == O.HIT


def band_records():
    """[(z, kind)] at z_min = -1.5 and z_max = 0.5 and one float on either side of each"""
    return [(f32(-1.5), O.HIT), (_down(-1.5), O.CLEAR), (_up(-1.5), O.HIT), (f32(0.5), O.HIT), (_up(0.5), O.CLEAR), (_down(0.5), O.HIT)]


def test_the_band_at_equality():
    cfg = OC.hand_config(8)
    for z, kind in band_records():
        _, k = _one(cfg, [(3, 1, z)])
        assert k[np.flatnonzero(k)].tolist() == [kind], (z, kind)


def gate_records():
    """[(x, kept)] for min_range 1 and max_range 20, y = z = 0: r is x exactly"""
    return [(f32(1.0), True), (_down(1.0), False), (f32(20.0), False), (_down(20.0), True)]


def test_the_range_gates_at_equality():
    cfg = OC.hand_config(8, min_range=1.0)
    for x, kept in gate_records():
        _, k = _one(cfg, [(x, 0, 0)])
        assert int((k != O.NONE).sum()) == (1 if kept else 0), x
    # not finite, and on the sensor's axis
    _, k = _one(cfg, [(np.nan, 1, 0), (1, np.inf, 0), (1, 1, -np.inf), (0, 0, 3)])
    assert (k == O.NONE).all()


def test_column_boundaries():
    """The probes of the segmentation's hand tests: under an unrotated pose the beam's column is the segmentation's."""
    cfg4 = OC.hand_config(4)
    for (x, y), col in _four_column_cases():
        _, k = _one(cfg4, [(x, y, 0)])
        assert np.flatnonzero(k).tolist() == [col], (x, y, col)
    for W in (16, 4096):
        cfg = OC.hand_config(W, max_range=100.0)
        seg = R.config(n_rows=1, n_columns=W, min_range=0.5, **ALONE)
        records = [r for recs in _boundary_records(seg).values() for r in recs] + _sign_records(W)
        want = R.columns(seg, [r[0] for r in records], [r[1] for r in records]).tolist()
        got = [np.flatnonzero(_one(cfg, [(x, y, 0)])[1]).tolist() for x, y in records]
        assert got == [[w] for w in want]
        assert want[-4:] == [W - 1, W - 1, W - 1, 0]


def tilt_pose():
    """a quarter turn about y: the sensor's x axis points down"""
    return np.array([[0.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 0.0], [-1.0, 0.0, 0.0, 0.0]])


def test_a_direction_made_vertical_has_no_column():
    cfg = OC.hand_config(8)
    _, k = _one(cfg, [(2, 0, 0)], pose=tilt_pose())
    assert (k == O.NONE).all()                                   # (x*x + y*y is 4, but dx = dy = 0)
    # the sensor's z axis is the world's x: a record above the sensor is a beam along +x at height 0
    xyz, k = _one(cfg, [(0.5, 0, 3)], pose=tilt_pose())
    assert k[np.flatnonzero(k)].tolist() == [O.HIT] and xyz[np.flatnonzero(k)[0]].tolist() == [0.5, 0.0, 3.0]


def test_class_masks():
    cfg = OC.hand_config(8)
    recs = [(3, 0.1, 0), (5, 0.1, 2)]
    for cls, om, cm, want in (([1, 2], 15, 15, (O.HIT, 3.0)), ([1, 2], 0b1100, 15, (O.CLEAR, 5.0)), ([1, 2], 0b1100, 0b0100, (O.CLEAR, 5.0)),
                              ([1, 2], 0b1100, 0b0010, (O.CLEAR, 3.0)), ([1, 3], 0b0100, 0b0100, None), ([9, 2], 15, 15, (O.CLEAR, 5.0))):
        xyz, k = _one(cfg, recs, cls=cls, obstacle_mask=om, clear_mask=cm)
        m = np.flatnonzero(k)
        assert (len(m) == 0) if want is None else (k[m[0]] == want[0] and xyz[m[0], 0] == want[1]), (cls, om, cm)


def emit_cases():
    """(emit fields, hits, misses, cell) by hand: 100 / (1 + e^2) = 11.9, 100 / (1 + e^-3.5) = 97.1, 100 / (1 + e^-0.85) = 70.1,
    100 / (1 + e^0.4) = 40.1, 100 / (1 + e^-1.3) = 78.6"""
    return [({}, 0, 0, -1), ({}, 1, 0, 70), ({}, 0, 1, 40), ({}, 5, 0, 97), ({}, 4, 0, 97), ({}, 0, 6, 12), ({}, 0, 5, 12), ({}, 8, 17, 50),
            (dict(min_observations=3), 1, 1, -1), (dict(min_observations=3), 2, 1, 79), (dict(l_min=-1000, l_max=1000), 0, 30, 0),
            (dict(l_min=-1000, l_max=1000), 12, 0, 100)]


def test_emit_by_hand():
    lut = O.emit_table(O.emit_config())
    assert len(lut) == 551 and lut[0] == 12 and lut[-1] == 97 and lut[200] == 50
    for fields, h, m, want in emit_cases():
        got = O.emit(np.array([[h]], np.uint32), np.array([[m]], np.uint32), O.emit_config(**fields))
        assert got.dtype == np.int8 and got.tolist() == [[want]], (fields, h, m, got, want)
    # counts near 2^32 do not wrap
    assert O.emit(np.array([[0xFFFFFFFF]], np.uint32), np.array([[0xFFFFFFFF]], np.uint32), O.emit_config()).tolist() == [[97]]


GRID_2X4 = np.array([[-1, 0, 25, 26], [64, 65, 100, 50]], np.int8)


def test_pgm_and_yaml_by_hand():
    """The top row of the image is the grid's last row; -1 and the cells between the thresholds are 205, >= 65 is 0, <= 25 is 254."""
    assert O.pgm_bytes(GRID_2X4) == b"P5\n4 2\n255\n" + bytes([205, 0, 0, 205, 205, 254, 254, 205])
    assert O.yaml_bytes(0.5, -12.25, 3.0) == (b"image: map.pgm\nresolution: 0.5\norigin: [-12.25, 3, 0.0]\nnegate: 0\noccupied_thresh: 0.65000000000000002\n"
                                               b"free_thresh: 0.25\n")
    assert b"resolution: 0.10000000149011612\n" in O.yaml_bytes(0.1, 0, 0)
