"""The host side of the de-skew section (include/lfx.h): the time channel of a field list, the motion helpers against
numpy, and the model itself against rays cast from a moving sensor (tests/deskew_restatement.py).  No device."""
import os

import numpy as np
import pytest

from lidar_feature_extraction_amd import binding as B
from tests import deskew_restatement as R


@pytest.fixture(scope="module")
def lfx():
    if not os.path.exists(B.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    import lidar_feature_extraction_amd as pkg
    B.load()
    return pkg


X, Y, Z, RING = ("x", 0, B.FLOAT32, 1), ("y", 4, B.FLOAT32, 1), ("z", 8, B.FLOAT32, 1), ("ring", 20, B.UINT16, 1)
FIELD_TABLE = [
    # name of the case, fields, point_step, big-endian, expected (offset, datatype, scale) or the error code
    ("velodyne", [X, Y, Z, ("intensity", 16, B.FLOAT32, 1), RING, ("time", 24, B.FLOAT32, 1)], 32, False, (24, B.FLOAT32, 1.0)),
    ("ouster", [X, Y, Z, ("intensity", 16, B.FLOAT32, 1), ("t", 20, B.UINT32, 1), ("ring", 26, B.UINT8, 1)], 48, False, (20, B.UINT32, 1e-9)),
    ("hesai", [X, Y, Z, ("intensity", 16, B.FLOAT32, 1), ("timestamp", 24, B.FLOAT64, 1), RING], 32, False, (24, B.FLOAT64, 1.0)),
    ("livox", [X, Y, Z, ("offset_time", 12, B.UINT32, 1), RING], 32, False, (12, B.UINT32, 1e-9)),
    ("time_stamp", [X, Y, Z, RING, ("time_stamp", 24, B.FLOAT64, 1)], 32, False, (24, B.FLOAT64, 1.0)),
    ("two candidates, first in the list wins", [X, Y, Z, RING, ("timestamp", 24, B.FLOAT64, 1), ("t", 12, B.UINT32, 1)], 32, False, (24, B.FLOAT64, 1.0)),
    ("two candidates, the other order", [X, Y, Z, RING, ("t", 12, B.UINT32, 1), ("timestamp", 24, B.FLOAT64, 1)], 32, False, (12, B.UINT32, 1e-9)),
    ("a candidate with count 2 is passed over", [X, Y, Z, RING, ("time", 12, B.FLOAT32, 2), ("t", 24, B.UINT32, 1)], 32, False, (24, B.UINT32, 1e-9)),
    ("none", [X, Y, Z, ("intensity", 16, B.FLOAT32, 1), RING], 32, False, B.ERR_NO_TIME_FIELD),
    ("no fields", [], 32, False, B.ERR_NO_TIME_FIELD),
    ("INT16 time", [X, Y, Z, RING, ("time", 24, B.INT16, 1)], 32, False, B.ERR_UNSUPPORTED_FIELD),
    ("INT32 time", [X, Y, Z, RING, ("t", 24, B.INT32, 1)], 32, False, B.ERR_UNSUPPORTED_FIELD),
    ("past point_step", [X, Y, Z, RING, ("time", 30, B.FLOAT32, 1)], 32, False, B.ERR_UNSUPPORTED_FIELD),
    ("FLOAT64 ends past point_step", [X, Y, Z, RING, ("timestamp", 28, B.FLOAT64, 1)], 32, False, B.ERR_UNSUPPORTED_FIELD),
    ("an offset near 2^32", [X, Y, Z, RING, ("time", 0xFFFFFFFE, B.FLOAT32, 1)], 32, False, B.ERR_UNSUPPORTED_FIELD),
    ("ends exactly at point_step", [X, Y, Z, RING, ("time", 28, B.FLOAT32, 1)], 32, False, (28, B.FLOAT32, 1.0)),
    ("big-endian", [X, Y, Z, RING, ("time", 24, B.FLOAT32, 1)], 32, True, (24, B.FLOAT32, 1.0)),
]


@pytest.mark.parametrize("name,fields,step,be,want", FIELD_TABLE, ids=[c[0] for c in FIELD_TABLE])
def test_time_field_from_fields(lfx, name, fields, step, be, want):
    if isinstance(want, int):
        with pytest.raises(B.LfxError) as e:
            lfx.time_field_from_fields(fields, step, be)
        assert e.value.code == want
        return
    tf = lfx.time_field_from_fields(fields, step, be)
    assert (tf.source, tf.offset, tf.datatype, tf.scale) == (B.TIME_FROM_FIELD,) + want
    assert tf.big_endian == int(be)


def test_time_field_null_arguments(lfx):
    L = B.load()
    out = B.TimeField()
    arr = (B.PointField * 1)(B.PointField(b"time", 24, B.FLOAT32, 1))
    assert L.lfx_time_field_from_fields(arr, 1, 32, 0, None) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_time_field_from_fields(None, 1, 32, 0, out) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_time_field_from_fields(arr, 1, 0, 0, out) == B.ERR_INVALID_ARGUMENT
    arr[0].name = None
    assert L.lfx_time_field_from_fields(arr, 1, 32, 0, out) == B.ERR_INVALID_ARGUMENT


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def test_motion_helpers_against_numpy(lfx):
    """1 000 seeded motions, |w| <= 1 rad, |t| <= 10 m: every entry within 1e-12 (about 50 double roundings at a conditioning
    below 10 give 1e-13; ten times that)."""
    rng = np.random.default_rng(20261)
    tol = 1e-12
    for i in range(1000):
        w = _unit(rng) * rng.uniform(0.0, 1.0) if i % 50 else _unit(rng) * 10.0 ** rng.uniform(-12, -7)
        t = _unit(rng) * rng.uniform(0.0, 10.0)
        D = R.pose(w, t)
        P0 = R.pose(_unit(rng) * rng.uniform(0.0, 3.0), rng.uniform(-50, 50, 3))
        P1 = R.compose(P0, D)
        got = lfx.motion_between(P0, P1)
        inv = np.hstack([P0[:, :3].T, (-P0[:, :3].T @ P0[:, 3]).reshape(3, 1)])
        assert np.abs(got - R.compose(inv, P1)).max() <= tol, i
        assert np.abs(got[:, :3] - D[:, :3]).max() <= tol, i
        tw, th = lfx.motion_twist(D)
        assert np.abs(tw - w).max() <= tol and abs(th - np.linalg.norm(w)) <= tol, (i, tw, w)
        ratio = rng.uniform(-0.5, 1.5)
        assert np.abs(lfx.motion_scale(D, ratio) - R.pose(ratio * w, ratio * t)).max() <= tol, i
        assert np.abs(lfx.motion_scale(D, 1.0) - D).max() <= tol, i
        # the restatement of the same arithmetic agrees far below the bound
        assert np.abs(R.between(P0, P1) - got).max() <= 1e-13 and np.abs(R.scale(D, ratio) - lfx.motion_scale(D, ratio)).max() <= 1e-13
        rw, rth = R.twist(D)
        assert np.abs(rw - tw).max() <= 1e-15 and abs(rth - th) <= 1e-15
        assert lfx.motion_between(P0, P0).tobytes() == R.IDENTITY.tobytes(), i
    tw, th = lfx.motion_twist(R.IDENTITY)
    assert tw.tobytes() == np.zeros(3).tobytes() and th == 0.0
    assert lfx.motion_scale(R.IDENTITY, 0.7).tobytes() == R.IDENTITY.tobytes()
    # rotations beyond the quaternion's first branch (trace <= 0)
    for axis in np.eye(3):
        w = axis * 2.8
        tw, th = lfx.motion_twist(R.pose(w, [0, 0, 0]))
        assert np.abs(tw - w).max() <= tol and abs(th - 2.8) <= tol
    L = B.load()
    assert L.lfx_motion_between(None, None, None) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_motion_twist(None, None, None) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_motion_scale(None, 1.0, None) == B.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("to_end", [True, False], ids=["to_end", "to_start"])
def test_the_model_is_physically_right(lfx, to_end):
    """A 16 x 900 sweep at 15 m/s and 35 deg/s of yaw with some roll and pitch: the restatement's float32 output carried to
    the world by P1 (P0 for TO_START) is within 4 * 2^-24 * max|coordinate| of the measured world points (the input's and
    the output's float rounding, each at most sqrt(3) * 2^-24 * max|coordinate| in norm); the raw points miss by more than
    0.5 m on average."""
    w, v = np.array([0.01, -0.02, 0.06]), np.array([1.5, 0.1, -0.05])
    D = R.pose(w, v)
    P0 = R.pose([0.0, 0.0, 0.4], [-2.0, 1.0, 1.8])
    P1 = R.compose(P0, D)
    rec, world, alpha = lfx.make_sweep(16, 900, seed=77, pose0=P0, motion=D, sigma=0.01)
    assert len(rec) == 16 * 900 and np.array_equal(alpha, np.arange(len(rec)) / len(rec))
    raw = np.stack([rec["x"], rec["y"], rec["z"], rec["pad"]], axis=1)
    out = R.deskew(raw, R.alpha_from_index(np.arange(len(rec)), len(rec)), D, to_end)
    assert np.array_equal(out[:, 3], raw[:, 3])
    carry = P1 if to_end else P0
    err = np.linalg.norm(R.apply(carry, out[:, :3].astype(np.float64)) - world, axis=1)
    bound = 4.0 * 2.0 ** -24 * max(np.abs(raw[:, :3]).max(), np.abs(out[:, :3]).max())
    miss = np.linalg.norm(R.apply(carry, raw[:, :3].astype(np.float64)) - world, axis=1)
    print("de-skewed: max %.3g m (bound %.3g m); raw: mean %.3f m, max %.3f m" % (err.max(), bound, miss.mean(), miss.max()))
    assert err.max() <= bound
    assert miss.mean() > 0.5
    # the time the records carry at byte 24 gives the same alpha to float32 precision
    t = rec.view(np.uint8).reshape(len(rec), 32)[:, 24:28].copy().view("<f4")[:, 0]
    assert np.abs(R.alpha_from_time(t, 1.0, 0.0, 0.1) - alpha).max() < 1e-6


def test_make_sweep_is_a_closed_room_and_static_without_motion(lfx):
    rec, world, alpha = lfx.make_sweep(16, 900, seed=5)
    assert np.isfinite(world).all() and world[:, 0].min() > -10.1 and world[:, 0].max() < 10.1
    assert world[:, 1].min() > -6.1 and world[:, 1].max() < 6.1 and world[:, 2].min() > -0.1 and world[:, 2].max() < 3.1
    assert np.array_equal(rec["ring"], np.arange(len(rec)) % 16)
    local = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float64)
    assert np.abs(local + [1.3, -0.7, 1.8] - world).max() < 1e-5
