"""The restatement of the store's flags (tests/keyframes_mask_restatement.py) held to cases written out by hand, and the
conditions tests/test_keyframes_masked_gpu.py relies on.  No GPU."""
import numpy as np

from tests import keyframes_mask_restatement as KM
from tests import keyframes_restatement as KR

# sphere_case(): the edge counts are 3, 2, 4, 0, 5, 6, 1, so the keyframes begin at records 0, 3, 5, 9, 9, 14, 20; radius 7
# around the centre selects keyframes 0 .. 5.  Flagged by hand: record 1 of keyframe 0; ALL of keyframe 2; records 10 and 12
# of keyframe 4; record 19 of keyframe 5; record 20 (keyframe 6, never selected).  Kept per selected keyframe: 2, 2, 0, 0, 3, 5;
# their prefix: 2, 4, 4, 4, 7, 12.
HAND_FLAGS = np.array([0, 1, 0,  0, 0,  1, 7, 255, 2,  0, 1, 0, 1, 0,  0, 0, 0, 0, 0, 1,  1], np.uint8)
HAND_KEPT = [0, 2, 3, 4, 9, 11, 13, 14, 15, 16, 17, 18]          # record indices of the whole store's build, in order


def _hand(capacity, first=0, count=None, radius=7.0):
    store, c, _, _, _ = KR.sphere_case()
    return KM.submap_masked(store, HAND_FLAGS, KR.EDGE, c, radius, first, count, capacity)


def test_hand_cases():
    store, c, _, _, _ = KR.sphere_case()
    assert store.begin(KR.EDGE).tolist() == [0, 3, 5, 9, 9, 14, 20, 21]
    world = store.build(KR.EDGE)
    # room for everything: the fully flagged keyframe 2 and the empty keyframe 3 are written, with 0 records
    cloud, res = _hand(64)
    assert res == dict(n_selected=6, n_written_keyframes=6, n_points=12, first_id=0, last_id=5, truncated=False)
    assert cloud.tobytes() == world[HAND_KEPT].tobytes()
    # capacity exactly at the kept prefix behind the last keyframe, and one below it
    assert _hand(12)[1] == res and _hand(12)[0].tobytes() == cloud.tobytes()
    cloud, res = _hand(11)
    assert res == dict(n_selected=6, n_written_keyframes=5, n_points=7, first_id=0, last_id=4, truncated=True)
    assert cloud.tobytes() == world[HAND_KEPT[:7]].tobytes()
    # keyframe 4 (5 records, 3 kept) fits 7 only because two of its records are flagged: with those two kept, 4 + 5 > 7
    unflagged = HAND_FLAGS.copy()
    unflagged[[10, 12]] = 0
    assert KM.submap_masked(store, unflagged, KR.EDGE, c, 7.0, 0, None, 7)[1] == dict(
        n_selected=6, n_written_keyframes=4, n_points=4, first_id=0, last_id=3, truncated=True)
    cloud, res = _hand(7)
    assert res == dict(n_selected=6, n_written_keyframes=5, n_points=7, first_id=0, last_id=4, truncated=True)
    assert cloud.tobytes() == world[[0, 2, 3, 4, 9, 11, 13]].tobytes()
    # one below that prefix: keyframe 4 does not fit, and keyframe 5 behind it is not tried; 2 and 3 count, with 0 records
    cloud, res = _hand(6)
    assert res == dict(n_selected=6, n_written_keyframes=4, n_points=4, first_id=0, last_id=3, truncated=True)
    assert cloud.tobytes() == world[[0, 2, 3, 4]].tobytes()
    # capacity 0: only what keeps nothing could be written, and keyframe 0 comes first and keeps 2
    assert _hand(0)[1] == dict(n_selected=6, n_written_keyframes=0, n_points=0, first_id=None, last_id=None, truncated=True)
    # a window of the fully flagged keyframe and the empty one alone: written, nothing in them
    cloud, res = _hand(0, 2, 2)
    assert res == dict(n_selected=2, n_written_keyframes=2, n_points=0, first_id=2, last_id=3, truncated=False) and len(cloud) == 0
    # the smaller sphere: keyframes 0, 1 and 3
    cloud, res = _hand(64, radius=5.0)
    assert res == dict(n_selected=3, n_written_keyframes=3, n_points=4, first_id=0, last_id=3, truncated=False)
    assert cloud.tobytes() == world[[0, 2, 3, 4]].tobytes()
    # the counts, the whole store's masked cloud (what save_masked writes), and the flag calls
    assert KM.n_flagged(store, (HAND_FLAGS, np.zeros(28, np.uint8))) == (9, 0)
    assert KM.build_masked(store, HAND_FLAGS, KR.EDGE).tobytes() == world[HAND_KEPT].tobytes()      # (record 20 is flagged)
    f = np.zeros(21, np.uint8)
    KM.set_flags(store, f, KR.EDGE, HAND_FLAGS, 2, 3)
    assert f.tolist() == [0] * 5 + [1, 7, 255, 2] + [0, 1, 0, 1, 0] + [0] * 7
    KM.clear_flags(store, f, KR.EDGE, 2, 1)
    assert f.tolist() == [0] * 9 + [0, 1, 0, 1, 0] + [0] * 7


def test_zero_flags_are_the_plain_submap():
    store, c, _, _, _ = KR.sphere_case()
    for kind in (KR.EDGE, KR.SURFACE):
        zeros = np.zeros(int(store.begin(kind)[-1]), np.uint8)
        for radius in (5.0, 7.0, 0.5):
            for first, count, capacity in ((0, None, 64), (0, None, 14), (0, None, 13), (4, 3, 64), (0, None, 0), (2, 0, 64)):
                want = store.submap(kind, c, radius, first, count, capacity)
                got = KM.submap_masked(store, zeros, kind, c, radius, first, count, capacity)
                assert got[1] == want[1] and got[0].tobytes() == want[0].tobytes()
    store = KR.bits_case()[0]
    zeros = np.zeros(int(store.begin(KR.EDGE)[-1]), np.uint8)
    want = store.submap(KR.EDGE, [0.0, 0.0, 0.0], 80.0, 0, None, 30000)
    got = KM.submap_masked(store, zeros, KR.EDGE, [0.0, 0.0, 0.0], 80.0, 0, None, 30000)
    assert got[1] == want[1] and got[0].tobytes() == want[0].tobytes() and 0 < want[1]["n_written_keyframes"] < want[1]["n_selected"]


def test_the_conditions_the_device_case_relies_on():
    store = KR.bits_case()[0]
    for kind in (KR.EDGE, KR.SURFACE):
        n = int(store.begin(kind)[-1])
        patterns = KM.bits_patterns(kind)
        assert set(patterns) == {"none", "all", "alternate", "random", "every_other_keyframe", "first_of_each", "last_of_each", "one_run",
                                 "bytes_1_2_255"}
        for name, f in patterns.items():
            assert f.dtype == np.uint8 and len(f) == n
            if name not in KM.UNIFORM:
                assert (f != 0).any() and (f == 0).any(), name
        assert not patterns["none"].any() and patterns["all"].all()
        assert set(np.unique(patterns["bytes_1_2_255"]).tolist()) == {0, 1, 2, 255}
        # a whole aligned run of RUN source records of the window (0, n) flagged, and one kept, amid kept ones
        f = patterns["one_run"].reshape(-1)[:n // KR.RUN * KR.RUN].reshape(-1, KR.RUN)
        assert f.all(axis=1).sum() == 1 and (~f.any(axis=1)).sum() == len(f) - 1 and len(f) > 10
        lo = KM.ONE_RUN
        assert lo % KR.RUN == 0 and f[lo // KR.RUN].all() and not f[lo // KR.RUN - 1].any() and not f[lo // KR.RUN + 1].any()
    # the staircase: keyframe boundaries at -1, 0 and +1 of multiples of 64, with a flagged record before some and behind some
    b = set(store.begin(KR.EDGE).astype(np.int64).tolist())
    f = KM.bits_patterns(KR.EDGE)["random"]
    for d in (-1, 0, 1):
        at = [64 * m + d for m in range(1, 65) if 64 * m + d in b]
        assert len(at) == 64
        assert any(f[i - 1] for i in at) and any(f[i] for i in at) and any(f[i - 1] and f[i] for i in at) and any(not f[i - 1] and not f[i] for i in at)
    # the short cut the device cases take (the kept rows of the whole store's build) is the restatement itself
    world = store.build(KR.EDGE)
    args = (store, f, KR.EDGE, [0.0, 0.0, 0.0], 92.0, 195, 400, 3000)
    slow, fast = KM.submap_masked(*args), KM.submap_masked(*args, world=world)
    assert slow[1] == fast[1] and slow[0].tobytes() == fast[0].tobytes() and 0 < slow[1]["n_points"]
    # the ranges that start and end inside a run
    begin = store.begin(KR.EDGE).astype(np.int64)
    inside = [(first, count) for first, count in KR.bits_ranges(store.begin(KR.EDGE)) if count and begin[first] % KR.RUN and
              (begin[first + count] - begin[first]) % KR.RUN and begin[first + count] - begin[first] > KR.RUN]
    assert len(inside) >= 2
