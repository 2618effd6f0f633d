"""The restatement of the packed payloads (tests/wire_cases.py) on a batch written out by hand, and the pool of scan
contents the GPU tests of the payloads draw from: every condition those tests lean on is checked here, with the oracle, on
a machine without a GPU."""
import numpy as np

from oracle import binding as OB
from tests import wire_cases as W


def _f32(v):
    return int(np.float32(v).view(np.uint32))


def _hand_made():
    """Three scans: one with a ring the reference abandoned between two it labelled, one without a record, one without an
    edge.  Coordinates are x = 10 i, y = 10 i + 1, z = 10 i + 2 for record i, so that a wrong gather shows."""
    def cloud(n):
        c = np.zeros(n, OB.POINT_DTYPE)
        c["x"], c["y"], c["z"] = 10.0 * np.arange(n), 10.0 * np.arange(n) + 1, 10.0 * np.arange(n) + 2
        return c

    a = W.empty_result()
    a.update(ring_id=np.array([0, 1, 2], np.int32), ring_count=np.array([3, 2, 2], np.int32), ring_status=np.array([0, 1, 0], np.int32),
             sorted_index=np.array([4, 0, 6, 1, 5, 3, 2], np.int32), labels=np.array([1, 0, 3, 7, 2, 0, 6], np.uint8),
             edge_points=np.array([[0, 1, 2, 0.5], [40, 41, 42, 0.25]], np.float32), surface_points=np.array([[20, 21, 22, 0.125]], np.float32))
    b = W.empty_result()
    c = W.empty_result()
    c.update(ring_id=np.array([7], np.int32), ring_count=np.array([2], np.int32), ring_status=np.array([0], np.int32),
             sorted_index=np.array([1, 0], np.int32), labels=np.array([4, 5], np.uint8),
             surface_points=np.array([[10, 11, 12, -1.0], [0, 1, 2, np.nan]], np.float32))
    return [(cloud(7), a), (cloud(0), b), (cloud(2), c)]


def test_restatement_on_a_hand_made_batch():
    exp = W.batch_expect([W.scan_piece(c, w) for c, w in _hand_made()])
    assert exp.batch == 3
    assert exp.offsets.tolist() == [0, 2, 2, 2, 0, 1, 1, 3] and exp.offsets.dtype == np.uint32
    assert exp.colored_offsets.tolist() == [0, 5, 5, 7]
    one = W.ONE
    assert one == 0x3F800000
    nan = int(np.array([[0, 1, 2, np.nan]], np.float32).view(np.uint32)[0, 3])
    e, s = exp.records("pack_features")
    assert e.tolist() == [[_f32(0), _f32(1), _f32(2), _f32(0.5)], [_f32(40), _f32(41), _f32(42), _f32(0.25)]]
    assert s.tolist() == [[_f32(20), _f32(21), _f32(22), _f32(0.125)], [_f32(10), _f32(11), _f32(12), _f32(-1.0)], [_f32(0), _f32(1), _f32(2), nan]]
    e, s = exp.records("pack_xyz")
    assert e.tolist() == [[_f32(0), _f32(1), _f32(2), one], [_f32(40), _f32(41), _f32(42), one]]
    assert s[:, 3].tolist() == [one] * 3 and s[:, :3].tolist() == exp.surface[:, :3].tolist()
    e, s = exp.records("pack_xyz12")
    assert e.shape == (2, 3) and s.shape == (3, 3) and e.flags["C_CONTIGUOUS"] and s.flags["C_CONTIGUOUS"]
    assert e.tolist() == [[_f32(0), _f32(1), _f32(2)], [_f32(40), _f32(41), _f32(42)]]
    assert exp.edge[:, 3].tolist() == [_f32(0.5), _f32(0.25)], "records() hands out copies"
    # colored_scan: ring 0's slice, not ring 1's (abandoned), ring 2's; then the third scan's ring
    (col,) = exp.records("pack_colored")
    white, red, orange, grey, magenta, green = 0xFFFFFFFF, 0xFFFF0000, 0xFFFF3F00, 0xFF7F7F7F, 0xFFFF00FF, 0xFF00FF00
    table = W.color_table().tolist()
    assert table == [white, red, orange, red, orange, grey, magenta, green]        # color_points.cpp:39-68
    for label in range(8):                                                         # the oracle's table says the same
        rgb = np.zeros(3, np.uint8)
        OB.lib().orc_label_to_color(label, rgb.ctypes.data_as(OB._pu8))
        assert table[label] == 0xFF000000 | int(rgb[0]) << 16 | int(rgb[1]) << 8 | int(rgb[2])
    want = [(4, orange), (0, red), (6, magenta), (3, green), (2, red), (1, grey), (0, orange)]     # (record, rgba)
    assert col.tolist() == [[_f32(10 * i), _f32(10 * i + 1), _f32(10 * i + 2), one, rgba, 0, 0, 0] for i, rgba in want]
    for call in W.CALLS:
        assert all(r.shape[1] == W.WORDS[call] and r.dtype == np.uint32 for r in exp.records(call))


def test_a_short_capacity_leaves_the_rest_at_the_sentinel():
    exp = W.batch_expect([W.scan_piece(c, w) for c, w in _hand_made()])
    before = exp.offsets.copy(), exp.colored_offsets.copy()
    (col,) = exp.records("pack_colored")
    S = W.SENTINEL
    assert S < 2 ** 31 and np.isnan(np.array([S], np.uint32).view(np.float32)[0])
    for capacity in (0, 1, 4, 5, 6, 7, 10, 2 ** 32 + 5):
        out = W.apply_capacity(col, capacity, 10)
        k = min(capacity, 7)
        assert out.shape == (10, 8) and out[:k].tolist() == col[:k].tolist() and (out[k:] == S).all(), capacity
    out = W.apply_capacity(exp.records("pack_xyz12")[1], 2, 6)
    assert out.shape == (6, 3) and out.reshape(-1)[:6].tolist() == exp.surface[:2, :3].reshape(-1).tolist() and (out.reshape(-1)[6:] == S).all()
    assert np.array_equal(exp.offsets, before[0]) and np.array_equal(exp.colored_offsets, before[1])
    assert W.apply_capacity(np.zeros((0, 4), np.uint32), 3, 2).tolist() == [[S] * 4] * 2


def test_the_pool_of_scan_contents():
    """8 x 450: what the batches of tests/test_wire_gpu.py are made of."""
    pool = {name: (c, want, piece) for name, c, want, piece in W.pool()}
    assert list(pool) == list(W.POOL_NAMES) and len(pool) == 8
    n_full = W.POOL_RINGS * W.POOL_COLS
    c, want, piece = pool["full"]
    assert len(c) == n_full and sorted(set(want["labels"].tolist())) == list(range(8)), "the full scan carries every label"
    c, want, piece = pool["one_ring_cut"]
    assert len(c) == n_full - W.POOL_COLS + 4
    assert (want["ring_status"] != 0).sum() == 1 and want["ring_count"][want["ring_status"] != 0].tolist() == [4]
    assert want["ring_id"][want["ring_status"] != 0].tolist() == [W.CUT_RING]
    assert len(piece.edge) > 0 and len(piece.surface) > 0 and len(piece.colored) == len(c) - 4
    c, want, piece = pool["every_ring_cut"]
    assert len(c) == 4 * W.POOL_RINGS and len(want["ring_status"]) == W.POOL_RINGS and (want["ring_status"] != 0).all()
    assert len(piece.edge) == 0 and len(piece.surface) == 0 and len(piece.colored) == 0
    c, want, piece = pool["empty"]
    assert len(c) == 0 and len(want["ring_id"]) == 0 and len(piece.edge) + len(piece.surface) + len(piece.colored) == 0
    assert W.POOL_NAMES[W.EMPTY] == "empty" and W.POOL_NAMES[W.FEATURELESS] == "every_ring_cut"
    for name in ("full", "dropped", "shuffled", "one_ring_cut", "rotated", "reversed_rotated"):
        c, want, piece = pool[name]
        assert len(piece.edge) >= 50 and len(piece.surface) >= 50, (name, len(piece.edge), len(piece.surface))
        assert len(piece.edge) != len(piece.surface), name            # (the two tables of a batch differ)
        assert len(piece.colored) == sum(n for n, st in zip(want["ring_count"], want["ring_status"]) if st == 0) > 0
    assert len(pool["dropped"][0]) < n_full and len(pool["shuffled"][0]) == n_full
    # a turned scan is a turned scan: the first record is not at the first azimuth, the reversed one runs clockwise
    az = lambda c: np.arctan2(c["y"], c["x"])[c["ring"] == 0]       # noqa: E731
    assert (np.diff(az(pool["full"][0])) > 0).all()
    assert (np.diff(az(pool["rotated"][0])) < 0).sum() == 1 and (np.diff(az(pool["reversed_rotated"][0])) > 0).sum() == 1
    assert (np.diff(az(pool["shuffled"][0])) < 0).sum() > 100


def test_where_the_empty_and_the_feature_less_scans_fall():
    """Position p takes content (3 p + 1) mod 8: over the batch sizes of the offsets test the empty scan is first in every
    batch, last in some; the feature-less one last in others; both lie inside every batch of more than two scans."""
    sizes = [769, 1, 513, 2, 257, 256, 255, 512, 511]
    last = {}
    for n in sizes:
        ids = W.contents_for(n)
        assert len(ids) == n and ids[0] == W.EMPTY
        last[n] = ids[-1]
        if n > 2:
            assert W.EMPTY in ids[1:-1] and W.FEATURELESS in ids[1:-1]
            assert set(ids) == set(range(8))
    assert [n for n in sizes if last[n] == W.EMPTY] == [769, 1, 513, 257]
    assert [n for n in sizes if last[n] == W.FEATURELESS] == [256, 512]
    assert last[255] == last[511] == W.POOL_NAMES.index("one_ring_cut") and last[2] == W.POOL_NAMES.index("shuffled")
