"""lfx_pose_diff (include/lfx.h) -- the keyframe test of the mapping node, PoseDiffIsSufficientlySmall (map.hpp:49-60) --
against the reference's own vectors (test_map.cpp:34-65, restated in tests/golden/mapping_vectors.json) and, bit for bit,
against the test-side restatement in the operation order lfx.h states (tests/mapping_restatement.py).  No device."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from lidar_feature_extraction_amd import binding as LB
from tests.mapping_restatement import pose, pose_diff, quaternion_matrix, small

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = json.load(open(os.path.join(ROOT, "tests", "golden", "mapping_vectors.json")))
PD = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LB.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return LB.load()


def _lib_diff(lib, p0, p1):
    a = np.ascontiguousarray(p0, np.float64).reshape(12)
    b = np.ascontiguousarray(p1, np.float64).reshape(12)
    t, r = C.c_double(0), C.c_double(0)
    assert lib.lfx_pose_diff(a.ctypes.data_as(PD), b.ctypes.data_as(PD), C.byref(t), C.byref(r)) == 0
    return t.value, r.value


def _reference_pairs():
    v = VECTORS["pose_diff"]
    q0 = v["pose0"]
    R0 = quaternion_matrix(*q0["quaternion_wxyz"], normalize=q0["normalized"])
    t0 = np.asarray(q0["translation"], np.float64)
    p0 = pose(R0, t0)
    for case in v["cases"]:
        if "dt" in case:
            p1 = pose(R0, t0 + np.asarray(case["dt"], np.float64))
        else:
            p1 = pose(R0 @ quaternion_matrix(*case["dq_wxyz"], normalize=case["normalized"]), t0)
        yield case, p0, p1


def test_reference_decisions(lib):
    """test_map.cpp:34-65: every EXPECT_TRUE / EXPECT_FALSE of PoseDiffIsSufficientlySmall through lfx_pose_diff."""
    n = 0
    for case, p0, p1 in _reference_pairs():
        t, r = _lib_diff(lib, p0, p1)
        for chk in case["checks"]:
            assert (t < chk["translation_threshold"] and r < chk["rotation_threshold"]) == chk["small"], (case["name"], t, r, chk)
            assert small(p0, p1, chk["translation_threshold"], chk["rotation_threshold"]) == chk["small"]
            n += 1
    assert n == 4


def _rotation(axis, angle):
    u = np.asarray(axis, np.float64)
    u = u / np.linalg.norm(u)
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


def test_restatement_bit_for_bit(lib):
    """About 10 000 random pose pairs: near identity, turns near 180 degrees (where the quaternion takes the branch of the
    largest diagonal entry, every one of the three), far poses, and pairs on either side of both default thresholds --
    the library equals the restatement bit for bit."""
    rng = np.random.default_rng(20261016)
    pairs = []
    for k in range(10000):
        R0 = _rotation(rng.normal(size=3), rng.uniform(-math.pi, math.pi))
        t0 = rng.normal(0, 50, 3)
        kind = k % 5
        if kind == 0:                                       # near identity
            R1, t1 = R0 @ _rotation(rng.normal(size=3), rng.normal(0, 1e-6)), t0 + rng.normal(0, 1e-6, 3)
        elif kind == 1:                                     # near 180 degrees about a random, then a coordinate, axis
            axis = rng.normal(size=3) if k % 2 else np.eye(3)[k % 3] + rng.normal(0, 1e-3, 3)
            R1, t1 = R0 @ _rotation(axis, math.pi - abs(rng.normal(0, 1e-3))), t0 + rng.normal(0, 2, 3)
        elif kind == 2:                                     # anything
            R1, t1 = _rotation(rng.normal(size=3), rng.uniform(-math.pi, math.pi)), rng.normal(0, 50, 3)
        elif kind == 3:                                     # translation on either side of 1.0
            d = rng.normal(size=3)
            R1, t1 = R0, t0 + R0 @ (d / np.linalg.norm(d) * (1.0 + rng.choice([-1, 1]) * 10.0 ** rng.uniform(-12, -3)))
        else:                                               # rotation on either side of |sin(angle / 2)| = 0.1
            ang = 2 * math.asin(0.1) * (1.0 + rng.choice([-1, 1]) * 10.0 ** rng.uniform(-12, -3))
            R1, t1 = R0 @ _rotation(rng.normal(size=3), ang), t0
        pairs.append((pose(R0, t0), pose(R1, t1)))
    branches = set()
    sides = {3: set(), 4: set()}
    for k, (p0, p1) in enumerate(pairs):
        got = _lib_diff(lib, p0, p1)
        want = pose_diff(p0, p1)
        assert np.float64(got[0]).tobytes() == np.float64(want[0]).tobytes() and \
            np.float64(got[1]).tobytes() == np.float64(want[1]).tobytes(), (k, got, want)
        R = p0[:, :3].T @ p1[:, :3]
        branches.add(-1 if np.trace(R) > 0 else int(np.argmax(np.diag(R))))
        if k % 5 == 3:
            sides[3].add(got[0] < 1.0)
        if k % 5 == 4:
            sides[4].add(got[1] < 0.1)
    assert branches == {-1, 0, 1, 2}
    assert sides[3] == {True, False} and sides[4] == {True, False}


def test_null_arguments(lib):
    p = np.eye(4)[:3].copy()
    t = C.c_double(0)
    assert lib.lfx_pose_diff(None, p.ctypes.data_as(PD), C.byref(t), C.byref(t)) == -1
    assert lib.lfx_pose_diff(p.ctypes.data_as(PD), p.ctypes.data_as(PD), None, C.byref(t)) == -1
    assert _lib_diff(lib, p, p) == (0.0, 0.0)
