"""Test-side restatement of the flags a keyframe store keeps (lfx_keyframes_reserve_flags .. lfx_keyframes_save_masked,
include/lfx.h) in numpy, no GPU, over tests/keyframes_restatement.Store plus one uint8 array per kind that is addressed by
the store's record index: a non-zero byte leaves the record out.  tests/test_keyframes_masked_expect.py holds it to
hand-written cases; tests/test_keyframes_masked_gpu.py holds the device to it, byte for byte."""
import numpy as np

from tests import keyframes_restatement as KR


def kept_of(store, flags, kind, k):
    """the records of keyframe k that stay, in record order: [n, 4] float32, sensor frame"""
    b = store.begin(kind)
    return store.clouds[kind][k][np.asarray(flags[int(b[k]):int(b[k + 1])]) == 0]


def submap_masked(store, flags, kind, center, radius, first=0, count=None, capacity=None, world=None):
    """(cloud, result): Store.submap's selection; a selected keyframe gives its kept records and is written while the kept
    records of the selected keyframes up to and including it fit `capacity`; nothing behind the first that does not fit.
    world: store.build(kind) of the whole store at the current poses, computed once by a caller with many cases -- a record's
    world bytes depend on the record and its keyframe's pose alone, so the kept rows of it are what is transformed here."""
    from tests.odometry_restatement import transform
    sel = store.select(center, radius, first, count)
    ids = [first + int(k) for k in np.nonzero(sel)[0]]
    b = store.begin(kind).astype(np.int64)
    keep = np.asarray(flags) == 0
    written, parts, n = [], [], 0
    for k in ids:
        mine = keep[b[k]:b[k + 1]]
        c = int(mine.sum())
        if capacity is not None and n + c > capacity:
            break
        written.append(k)
        parts.append(transform(store.pose[k], store.clouds[kind][k][mine]) if world is None else world[b[k]:b[k + 1]][mine])
        n += c
    res = dict(n_selected=len(ids), n_written_keyframes=len(written), n_points=n, first_id=written[0] if written else None,
               last_id=written[-1] if written else None, truncated=len(written) < len(ids))
    return np.concatenate(parts + [np.zeros((0, 4), np.float32)]), res


def build_masked(store, flags, kind, first=0, count=None):
    """the world cloud of keyframes [first, first + count) without the flagged records: what save_masked writes for the
    whole store (no file where it is empty)"""
    from tests.odometry_restatement import transform
    ks = range(first, len(store) if count is None else first + count)
    return np.concatenate([transform(store.pose[k], kept_of(store, flags, kind, k)) for k in ks] + [np.zeros((0, 4), np.float32)])


def n_flagged(store, flags):
    return tuple(int(np.count_nonzero(np.asarray(flags[kind])[:int(store.begin(kind)[-1])])) for kind in (KR.EDGE, KR.SURFACE))


def set_flags(store, flags, kind, src, first, count):
    """lfx_keyframes_set_flags on the host: the bytes of keyframes [first, first + count) taken from src, in place"""
    b = store.begin(kind)
    lo, hi = int(b[first]), int(b[first + count])
    flags[lo:hi] = np.asarray(src)[lo:hi]


def clear_flags(store, flags, kind, first, count):
    b = store.begin(kind)
    flags[int(b[first]):int(b[first + count])] = 0


# --- the flag patterns of the bits case ------------------------------------------------------------------------------------------
# the first record of the run that "one_run" flags: a whole run of KR.RUN source records of the window (0, n), well inside the store
ONE_RUN = 8 * KR.RUN


def bits_patterns(kind):
    """name -> uint8 [n_records] over KR.bits_case()'s store of `kind`"""
    store = KR.bits_case()[0]
    b = store.begin(kind).astype(np.int64)
    n = int(b[-1])
    rng = np.random.default_rng(20260 + kind)
    out = {"none": np.zeros(n, np.uint8), "all": np.ones(n, np.uint8)}
    out["alternate"] = (np.arange(n) % 2).astype(np.uint8)
    out["random"] = (rng.random(n) < 0.3).astype(np.uint8)
    f = np.zeros(n, np.uint8)
    for k in range(0, len(store), 2):
        f[b[k]:b[k + 1]] = 1
    out["every_other_keyframe"] = f
    first, last = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    nonempty = b[1:] > b[:-1]
    first[b[:-1][nonempty]] = 1
    last[b[1:][nonempty] - 1] = 1
    out["first_of_each"], out["last_of_each"] = first, last
    f = np.zeros(n, np.uint8)
    f[ONE_RUN:ONE_RUN + KR.RUN] = 1
    out["one_run"] = f
    f = (rng.random(n) < 0.3).astype(np.uint8) * rng.choice(np.array([1, 2, 255], np.uint8), n)
    out["bytes_1_2_255"] = f
    return out


UNIFORM = ("none", "all")
