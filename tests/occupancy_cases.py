"""The cases the occupancy tests share (tests/test_occupancy_expect.py on the restatement, tests/test_occupancy_gpu.py on the
device): scans of a few records whose beams, cells and votes are written out by hand, and the device plumbing.

The hand cases are drawn on a grid of 1 m cells whose cell (0, 0) starts at the world origin, with poses that do not rotate:
a record (x, y, z) seen from a sensor at (tx, ty) ends in cell (floor(tx + x), floor(ty + y)), and the sensor stands in cell
(floor(tx), floor(ty)).  z = 0 lies in the obstacle band (a HIT beam), z = 2 above it (a CLEAR beam)."""
import numpy as np

from tests import occupancy_restatement as O
from tests import segment_restatement as R

f32 = np.float32
HAND_GRIDS = [(32, 32), (96, 40)]                   # (width, height): the second one is not square -- a swapped stride shows
HAND_BEAMS = [8, 16]


def hand_config(W=8, width=32, height=32, **fields):
    return O.config(**dict(dict(n_beams=W, max_scans=16, width=width, height=height, resolution=1.0, origin_x=0.0, origin_y=0.0, min_range=0.1,
                                max_range=20.0, z_min=-1.5, z_max=0.5, chunk_scans=2), **fields))


def pose_at(tx, ty, tz=0.0):
    return np.array([[1.0, 0.0, 0.0, tx], [0.0, 1.0, 0.0, ty], [0.0, 0.0, 1.0, tz]])


def row(y, x0, x1):
    """the cells (x0, y) .. (x1, y)"""
    return [(x, y) for x in range(x0, x1 + 1)]


def votes(cells, n=1):
    return {c: n for c in cells}


MID = (10.5, 10.5)                                  # a sensor in cell (10, 10)
# name: (scans [(sensor (tx, ty), records [(x, y, z)])], occupied votes {(x, y): n}, free votes {(x, y): n}) -- every cell
# list below is the Bresenham of include/lfx.h walked by hand
HAND = {
    "plus_x": ([(MID, [(5, 0, 0)])], votes([(15, 10)]), votes(row(10, 10, 14))),
    "minus_y": ([(MID, [(0, -4, 0)])], votes([(10, 6)]), votes([(10, 10), (10, 9), (10, 8), (10, 7)])),
    "diagonal": ([(MID, [(3, 3, 0)])], votes([(13, 13)]), votes([(10, 10), (11, 11), (12, 12)])),
    "slope_half": ([(MID, [(4, 2, 0)])], votes([(14, 12)]), votes([(10, 10), (11, 10), (12, 11), (13, 11)])),
    "slope_two": ([(MID, [(2, 4, 0)])], votes([(12, 14)]), votes([(10, 10), (10, 11), (11, 12), (11, 13)])),
    "slope_half_backwards": ([(MID, [(-4, -2, 0)])], votes([(6, 8)]), votes([(10, 10), (9, 10), (8, 9), (7, 9)])),
    "end_is_origin_hit": ([(MID, [(0.2, 0.2, 0)])], votes([(10, 10)]), {}),
    "end_is_origin_clear": ([(MID, [(0.2, 0.2, 2)])], {}, votes([(10, 10)])),
    # the end cell (-3, 10) and the cells (-1, 10), (-2, 10) are outside: the ray is clipped, not dropped
    "leaves_the_grid": ([((2.5, 10.5), [(-5, 0, 0)])], {}, votes(row(10, 0, 2))),
    # the sensor stands in cell (-3, 5)
    "starts_outside": ([((-2.5, 5.5), [(6, 0, 0)])], votes([(3, 5)]), votes(row(5, 0, 2))),
    # two beams of one scan (y = +0.2 and -0.2: the two columns at azimuth 0) along the row 10: one free vote per cell, and
    # the cell (15, 10) where the first one ends in a hit is passed by the second one: occupied, not free
    "two_beams_of_one_scan": ([(MID, [(5, 0.2, 0), (6, -0.2, 0)])], votes([(15, 10), (16, 10)]), votes(row(10, 10, 14))),
    # the same cell hit in one scan and passed in the next one: one vote of each
    "hit_then_passed": ([(MID, [(5, 0, 0)]), (MID, [(8, 0, 0)])], votes([(15, 10), (18, 10)]), {**votes(row(10, 10, 14), 2), **votes(row(10, 15, 17))}),
    "clear_beam": ([(MID, [(5, 0, 2)])], {}, votes(row(10, 10, 15))),
}


def hand_scans(name):
    """(clouds, poses) of a hand case: every scan 2 x 16 records -- the case's own in front, the rest (0, 0, 0), which the
    gates skip."""
    scans, _, _ = HAND[name]
    clouds, poses = [], []
    for (tx, ty), records in scans:
        recs = [(f32(x), f32(y), f32(z), 0) for x, y, z in records]
        recs += [(f32(0), f32(0), f32(0), k // 16) for k in range(len(recs), 32)]
        clouds.append(R.cloud_of(recs))
        poses.append(pose_at(tx, ty))
    return clouds, np.stack(poses)


def hand_counts(name, width, height):
    """(hits, misses) uint32 [height][width] of a hand case, from its dictionaries."""
    _, occupied, free = HAND[name]
    hits, misses = np.zeros((height, width), np.uint32), np.zeros((height, width), np.uint32)
    for (x, y), n in occupied.items():
        hits[y, x] = n
    for (x, y), n in free.items():
        misses[y, x] = n
    return hits, misses


def same_bytes(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        g, w = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
        bad = np.argwhere(g != w)
        raise AssertionError((what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def tilted_poses(n, seed=5):
    """n poses in a room: a yaw of any size, a few degrees of roll and pitch, a translation of a few metres (rotations
    orthonormal to rounding, as an estimator's)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        yaw, pitch, roll = rng.uniform(-np.pi, np.pi), rng.uniform(-0.06, 0.06), rng.uniform(-0.06, 0.06)
        cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
        Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
        Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
        Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
        t = np.array([rng.uniform(-6, 6), rng.uniform(-6, 6), rng.uniform(-0.2, 0.2)])
        out.append(np.concatenate([Rz @ Ry @ Rx, t[:, None]], axis=1))
    return np.stack(out)
