"""The keyframe store's restatement (tests/keyframes_restatement.py) held to hand-written cases, and the conditions the GPU
cases (tests/test_keyframes_gpu.py) rest on.  No GPU."""
import numpy as np

from tests import keyframes_restatement as KR


def f32(rows):
    return np.array(rows, np.float32).reshape(-1, 4)


def test_three_keyframes_by_hand():
    """Keyframes of 2, 0 and 1 edge records (1, 1 and 0 surface records).  Poses: a quarter turn about z with t = (10, 20, 30);
    any pose for the empty one; the identity with t = (-1, -2, -3).  The quarter turn maps (x, y, z) to (-y, x, z)."""
    s = KR.Store(3, (3, 2))
    quarter = np.array([[0.0, -1.0, 0.0, 10.0], [1.0, 0.0, 0.0, 20.0], [0.0, 0.0, 1.0, 30.0]])
    shift = np.array([[1.0, 0.0, 0.0, -1.0], [0.0, 1.0, 0.0, -2.0], [0.0, 0.0, 1.0, -3.0]])
    edge = [f32([[1, 2, 3, 0.5], [-4, 5, -6, -0.0]]), f32([]), f32([[0.25, 0.5, 0.75, 9]])]
    surface = [f32([[1, 0, 0, 7]]), f32([[0, 0, 1, 8]]), f32([])]
    assert s.add(edge, surface, [quarter, KR.pose([1.0, 2.0, 3.0], [4.0, 5.0, 6.0]), shift]) == 0
    assert s.begin(KR.EDGE).tolist() == [0, 2, 2, 3] and s.begin(KR.SURFACE).tolist() == [0, 1, 2, 2]
    assert s.records(KR.EDGE).tobytes() == np.concatenate(edge).tobytes()
    want = f32([[8, 21, 33, 0.5], [5, 16, 24, -0.0], [-0.75, -1.5, -2.25, 9]])
    assert s.build(KR.EDGE).tobytes() == want.tobytes()
    assert np.signbit(s.build(KR.EDGE)[1, 3])                       # the 4th float is copied: -0.0 stays -0.0
    assert s.build(KR.EDGE, 1, 1).shape == (0, 4) and s.build(KR.EDGE, 1, 2).tobytes() == want[2:].tobytes()
    assert s.build(KR.SURFACE, 0, 1).tobytes() == f32([[10, 21, 30, 7]]).tobytes()
    # the poses move, the records do not: the same function of (record, pose)
    s.set_poses([shift], first=0)
    assert s.build(KR.EDGE, 0, 1).tobytes() == f32([[0, 0, 0, 0.5], [-5, 3, -9, -0.0]]).tobytes()
    assert s.poses()[2].tobytes() == shift.tobytes()
    # refusals change nothing
    assert s.add([f32([])], [f32([])], [shift]) == "capacity"
    t = KR.Store(3, (3, 2))
    assert t.add([f32([[0, 0, 0, 0]] * 4)], [f32([])], [shift]) == "capacity" and len(t) == 0
    assert t.add([f32([])], [f32([])], [np.full((3, 4), np.inf)]) == "invalid" and len(t) == 0


def test_selection_on_the_sphere():
    s, c, _, _, _ = KR.sphere_case()
    for radius, want in KR.SPHERE_WANT.items():
        assert s.select(c, radius).tolist() == want, radius
    # a window: the same flags, cut
    assert s.select(c, 7.0, 2, 3).tolist() == KR.SPHERE_WANT[7.0][2:5]
    assert s.select(c, 0.0).tolist() == [False] * 7


def test_truncation_at_the_capacity_and_one_short():
    """Radius 5 selects keyframes 0, 1 and 3 of 3, 2 and 0 edge records; radius 7 selects 0 .. 5 of 3, 2, 4, 0, 5, 6."""
    s, c, edge, _, _ = KR.sphere_case()
    cloud, res = s.submap(KR.EDGE, c, 7.0, capacity=14)              # 3 + 2 + 4 + 0 + 5 = 14: stops exactly at the capacity
    assert res == dict(n_selected=6, n_written_keyframes=5, n_points=14, first_id=0, last_id=4, truncated=True)
    assert cloud.tobytes() == s.build(KR.EDGE, 0, 5).tobytes()
    cloud, res = s.submap(KR.EDGE, c, 7.0, capacity=13)              # one record short of keyframe 4: it and keyframe 5 are left out
    assert res == dict(n_selected=6, n_written_keyframes=4, n_points=9, first_id=0, last_id=3, truncated=True)
    assert cloud.tobytes() == s.build(KR.EDGE, 0, 3).tobytes()
    cloud, res = s.submap(KR.EDGE, c, 7.0, capacity=20)
    assert res == dict(n_selected=6, n_written_keyframes=6, n_points=20, first_id=0, last_id=5, truncated=False)
    cloud, res = s.submap(KR.EDGE, c, 5.0)
    assert res == dict(n_selected=3, n_written_keyframes=3, n_points=5, first_id=0, last_id=3, truncated=False)
    assert cloud.tobytes() == np.concatenate([KR.transform(s.pose[0], edge[0]), KR.transform(s.pose[1], edge[1])]).tobytes()
    # a smaller keyframe behind the first that does not fit is NOT written: writing stops
    cloud, res = s.submap(KR.EDGE, c, 7.0, capacity=4)
    assert (res["n_written_keyframes"], res["n_points"], res["last_id"]) == (1, 3, 0)
    # a window that leaves the near keyframes out; nothing selected
    cloud, res = s.submap(KR.EDGE, c, 7.0, 4, 3)
    assert (res["n_selected"], res["first_id"], res["last_id"], res["n_points"]) == (2, 4, 5, 11)
    cloud, res = s.submap(KR.EDGE, c, 0.5)
    assert res == dict(n_selected=0, n_written_keyframes=0, n_points=0, first_id=None, last_id=None, truncated=False) and cloud.shape == (0, 4)
    cloud, res = s.submap(KR.EDGE, c, 7.0, capacity=2)               # the first one does not fit: nothing is written
    assert res == dict(n_selected=6, n_written_keyframes=0, n_points=0, first_id=None, last_id=None, truncated=True)


def test_what_the_gpu_build_case_rests_on():
    counts = np.array(KR.bits_counts())
    begin = np.concatenate([[0], np.cumsum(counts)])
    bounds = set(begin.tolist())
    for m in range(KR.WAVE, 4096 + 1, KR.WAVE):
        assert {m - 1, m, m + 1} <= bounds, m
    ones = "".join("1" if c == 1 else "." for c in counts)
    zeros = "".join("0" if c == 0 else "." for c in counts)
    assert "1" * 300 in ones and "0" * 40 in zeros
    assert set(counts.tolist()) >= set(KR.DRAWN), "every size of the list is drawn"
    assert 50000 <= begin[-1] <= 70000 and (counts > KR.RUN).any()
    # the surface store has the counts reversed: another set of boundaries
    rbegin = np.concatenate([[0], np.cumsum(counts[::-1])])
    assert rbegin.tolist() != begin.tolist()
    s, edge, surface, poses = KR.bits_case()
    assert s.begin(KR.EDGE).tolist() == begin.tolist() and s.begin(KR.SURFACE).tolist() == rbegin.tolist()
    rec = s.records(KR.EDGE)
    assert np.signbit(rec[0]).all() and np.isinf(rec).any() and (np.abs(rec[rec != 0]) < 1e-38).any()
    # the ranges: start and end inside a run; one of only empty keyframes, one keyframe, the last, none
    ranges = KR.bits_ranges(s.begin(KR.EDGE))
    assert ranges[0] == (0, len(counts))
    for first, count in ranges[1:3]:
        lo, hi = int(begin[first]), int(begin[first + count])
        assert lo % KR.RUN and lo % KR.WAVE and (hi - lo) % KR.RUN and (hi - lo) % KR.WAVE and hi - lo > 2 * KR.RUN, (first, count)
    assert begin[ranges[3][0]] == begin[ranges[3][0] + ranges[3][1]] and ranges[3][1] == 5
    assert counts[ranges[4][0]] == 4097 and ranges[5] == (len(counts) - 1, 1) and ranges[6][1] == 0
    # large angles, far translations
    assert np.abs(poses[:, :, 3]).max() > 100.0 and np.abs(np.einsum("kij,klj->kil", poses[:, :, :3], poses[:, :, :3]) - np.eye(3)).max() < 1e-12
