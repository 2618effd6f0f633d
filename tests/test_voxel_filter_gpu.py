"""The voxel filter on the device (lfx_voxel_filter_*, lfx_keyframes_save_filtered; include/lfx.h) against its restatement
(tests/voxel_filter_restatement.py): every cloud, every count, the guard records behind capacity_points and every field of the
result are compared byte for byte -- nothing here has a tolerance.  tests/test_voxel_filter_expect.py holds the restatement to
hand cases.

What the shapes are built around (csrc/lfx_kernels_voxelfilter.hpp): an add gives a workgroup lfx::kVfRun = 1024 consecutive
records and a wave 64 consecutive ones per step, whose runs of equal voxels it merges before the atomics (VF.WAVE, VF.RUN); an
emit scans the rank bitmap in tiles of lfx::kVfScanTile = 32 768 ranks (VF.SCAN_TILE: 1024 words of 32 bits per workgroup);
add_host goes up in chunks of 2^16 records (VF.HOST_CHUNK); a voxel's probe starts at VF.home(key)."""
import os

import numpy as np
import pytest

from tests import deskew_cases as K
from tests import keyframes_mask_restatement as KM
from tests import keyframes_restatement as KR
from tests import segment_cases as S
from tests import voxel_filter_restatement as VF
from tests.test_keyframes_gpu import _device_store, _up

pytestmark = pytest.mark.gpu
GUARD = 64                                   # guard records behind capacity_points
FILL, CFILL = -123.25, 0x5A5A5A5A


@pytest.fixture(scope="module")
def fx():
    f = K.fx_for(16, 64, 3)
    yield f
    f.close()


@pytest.fixture(scope="module")
def hold():
    return S.Hold()


@pytest.fixture(scope="module")
def vf17(fx):
    """2^17 entries, 2^18 ranks: what most cases share (each resets it)"""
    v = fx.voxel_filter(17, 1 << 18)
    yield v
    v.close()


def _emit(vf, capacity, min_points=1, counts=True, stream=None):
    """one emit into buffers with GUARD records behind the capacity: (rc, result, cloud + guards, counts + guards)"""
    import torch
    out = torch.full((capacity + GUARD, 4), FILL, dtype=torch.float32, device=K.dev())
    cnt = torch.full((capacity + GUARD,), CFILL, dtype=torch.int32, device=K.dev())
    rc, res = vf.emit_raw(min_points, out.data_ptr(), capacity, cnt.data_ptr() if counts else 0, K.stream() if stream is None else stream)
    K.sync()
    return rc, res, out.cpu().numpy(), cnt.cpu().numpy().view(np.uint32)


def _holds(vf, ref, min_points=1, capacity=None, counts=True, what=None, stream=None):
    """the device filter emits what the restatement `ref` emits: status, result, cloud, counts, guards"""
    from lidar_feature_extraction_amd import binding as B
    status, cloud, cnt, res = ref.emit(min_points, capacity)
    cap = res["n_written"] if capacity is None else capacity
    rc, got, out, c = _emit(vf, cap, min_points, counts, stream)
    print(what, "result", got)
    assert got == res, (what, got, res)
    assert rc == (B.ERR_CAPACITY if status == "capacity" else 0), (what, rc, status)
    n = len(cloud)
    assert out[:n].tobytes() == cloud.tobytes(), (what, int((out[:n].view(np.uint32) != cloud.view(np.uint32)).any(axis=1).sum()), n)
    assert (out[n:] == FILL).all(), what
    if counts:
        assert c[:n].tolist() == cnt.tolist(), what
        assert (c[n:] == CFILL).all(), what
    else:
        assert (c == CFILL).all(), what
    return out[:n].copy(), c[:n].copy(), got


def _both(vf, leaf, log2_slots=17, max_records=1 << 18):
    ref = VF.Filter(log2_slots, max_records)
    ref.reset(leaf)
    vf.reset(leaf, K.stream())
    return ref


def _add(vf, ref, pts):
    pts = np.asarray(pts, np.float32).reshape(-1, 4)
    assert ref.add(pts) is None
    d = _up(pts)
    vf.add(d, stream=K.stream())
    K.sync()


def _inside(voxels, rng, leaf=1.0):
    """one record somewhere inside each voxel of the list (leaf a power of two: v + u is exact enough to stay inside)"""
    v = np.asarray(voxels, np.float64).reshape(-1, 3)
    out = rng.normal(0, 1, (len(v), 4)).astype(np.float32)
    out[:, :3] = ((v + rng.uniform(0.05, 0.95, v.shape)) * leaf).astype(np.float32)
    return out


def test_trivial_sizes_and_wave_and_launch_edges(vf17):
    """0 and 1 record; 63 / 64 / 65 and 255 / 256 / 257 records of distinct voxels; 1023 / 1024 / 1025: one workgroup and two"""
    rng = np.random.default_rng(1)
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025):
        ref = _both(vf17, 0.5)
        if n:
            _add(vf17, ref, _inside([(i, -(i % 5), i // 7 - 40) for i in range(n)], rng, 0.5))
        else:
            vf17.add(0, 0, K.stream())
        _, _, res = _holds(vf17, ref, what=n)
        assert res["n_written"] == res["n_voxels"] == res["n_records"] == n
    assert vf17.info()["slots"] == 1 << 17 and vf17.info()["max_records"] == 1 << 18 and vf17.info()["leaf"] == 0.5
    assert vf17.info()["device_bytes"] >= 64 << 17


def test_runs_of_equal_voxels_at_every_lane(vf17):
    """Runs of 1, 2, 63, 64, 65 and 300 records of one voxel that start at every lane residue of a wave: every (length, residue)
    is a segment of its own that begins on a multiple of 64 -- `residue` records of distinct voxels, the run, distinct voxels
    up to the next multiple of 64.  (Segments begin at multiples of 64 of the add, which is where waves begin.)"""
    rng = np.random.default_rng(2)
    parts, nv = [], 0
    for length in (1, 2, 63, 64, 65, 300):
        for residue in range(VF.WAVE):
            tail = -(residue + length) % VF.WAVE
            vox = [(nv + i, 1, 0) for i in range(residue)] + [(nv + residue, 2, 0)] * length + [(nv + residue + 1 + i, 3, 0) for i in range(tail)]
            nv += residue + 1 + tail
            parts.append(_inside(vox, rng))
    pts = np.concatenate(parts)
    assert len(pts) % VF.WAVE == 0 and len(pts) > 50 * VF.RUN and nv < 1 << 16 and len(pts) <= 1 << 18
    ref = _both(vf17, 1.0)
    _add(vf17, ref, pts)
    _, counts, res = _holds(vf17, ref, what="runs")
    assert res["n_voxels"] == nv and sorted(set(counts.tolist())) == [1, 2, 63, 64, 65, 300]


def _contended(n, n_voxels, rng):
    """n records in n_voxels voxels: the first n_voxels records open the voxels in order, the last n_voxels close them in order,
    the rest fall anywhere -- so the reversed sequence opens them in the reversed order"""
    which = rng.integers(0, n_voxels, n)
    which[:n_voxels] = np.arange(n_voxels)
    which[n - n_voxels:] = np.arange(n_voxels)
    return _inside([(int(w) - 100, 7, -3) for w in which], rng, 0.25)


@pytest.mark.parametrize("n_voxels", (1, 256))
def test_contention(vf17, n_voxels):
    """70 001 records into one voxel and into 256, forwards and reversed: the same centroids and counts, in the reversed order
    of appearance"""
    pts = _contended(70001, n_voxels, np.random.default_rng(3))
    ref = _both(vf17, 0.25)
    _add(vf17, ref, pts)
    fwd, fc, res = _holds(vf17, ref, what=("forward", n_voxels))
    assert res["n_written"] == n_voxels and int(fc.sum()) == 70001
    ref = _both(vf17, 0.25)
    _add(vf17, ref, pts[::-1])
    rev, rc, _ = _holds(vf17, ref, what=("reversed", n_voxels))
    assert rev.tobytes() == fwd[::-1].tobytes() and rc.tolist() == fc[::-1].tolist()


def test_probing(fx):
    """16 entries.  8 voxels that share home entry 5; 8 that share the LAST entry, whose probe chain wraps to entries 0 .. 6; both
    sets together (16 voxels: the table exactly full); 16 voxels of 3 records: OK and exact; 17 such voxels: LFX_ERR_CAPACITY,
    n_table_full == 3 (the voxels have equal size: whichever loses), the guards untouched, and the call returns."""
    from lidar_feature_extraction_amd import binding as B
    rng = np.random.default_rng(4)
    vf = fx.voxel_filter(4, 4096)
    mid, last = VF.sharing_home(4, 5, 8), VF.sharing_home(4, 15, 8, vy=1)
    assert all(VF.home(VF.key(*v), 4) == 5 for v in mid) and all(VF.home(VF.key(*v), 4) == 15 for v in last)
    for name, vox in (("one home", mid), ("wraps", last), ("both", mid + last)):
        ref = _both(vf, 1.0, 4, 4096)
        order = rng.permutation(np.repeat(np.arange(len(vox)), 5))
        _add(vf, ref, _inside([vox[i] for i in order], rng))
        _, counts, res = _holds(vf, ref, what=name)
        assert res["n_voxels"] == len(vox) and counts.tolist() == [5] * len(vox)
    for n_voxels in (16, 17):
        vox = [(3 * k, -k, k) for k in range(n_voxels)]
        ref = _both(vf, 1.0, 4, 4096)
        _add(vf, ref, np.concatenate([_inside(vox, rng) for _ in range(3)]))
        _, _, res = _holds(vf, ref, what=n_voxels, capacity=32)
        assert res["n_table_full"] == (0 if n_voxels == 16 else 3) and res["n_voxels"] == 16
    # the full table stays usable for the voxels it holds, and a reset empties it
    rc, res, out, _ = _emit(vf, 32)
    assert rc == B.ERR_CAPACITY and res["n_table_full"] == 3 and (out == FILL).all()
    ref = _both(vf, 1.0, 4, 4096)
    _add(vf, ref, _inside([(0, 0, 0)], rng))
    _holds(vf, ref, what="after the full table")
    vf.close()


ORDER_RANKS = (31, 32, 33, 63, 64, VF.SCAN_TILE - 1, VF.SCAN_TILE, VF.SCAN_TILE + 1, 2 * VF.SCAN_TILE - 1, 2 * VF.SCAN_TILE, 2 * VF.SCAN_TILE + 1)


@pytest.mark.parametrize("bulk", ("one voxel", "skipped"))
def test_order_at_word_and_tile_boundaries(vf17, bulk):
    """Least ranks at 31, 32, 33, 63, 64 (the words of the rank bitmap) and at each boundary of the emit's scan tile
    (lfx::kVfScanTile = 32 768 ranks) - 1, + 0, + 1, for the first two boundaries: every other record lies in one bulk voxel (least
    rank 0) or is not finite (skipped: it takes a rank and sets no bit, so the first word's bit 0 stays clear)."""
    rng = np.random.default_rng(5)
    n = 2 * VF.SCAN_TILE + 40
    pts = _inside([(0, 0, 0)] * n, rng)
    if bulk == "skipped":
        pts[:, 1] = np.nan
    special = _inside([(10 + i, 0, 0) for i in range(len(ORDER_RANKS))], rng)
    pts[list(ORDER_RANKS)] = special[rng.permutation(len(special))]
    ref = _both(vf17, 1.0)
    _add(vf17, ref, pts)
    cloud, counts, res = _holds(vf17, ref, what=bulk)
    assert res["n_written"] == len(ORDER_RANKS) + (bulk == "one voxel") and res["n_records"] == n
    assert res["n_nonfinite"] == (n - len(ORDER_RANKS) if bulk == "skipped" else 0)
    _holds(vf17, ref, min_points=2, what=(bulk, "min 2"))


def test_min_points_and_counts(vf17):
    """min_points 1, 2 and 3 on voxels of 1, 2 and 3 records (ten of each, interleaved); with d_counts_out and with NULL"""
    rng = np.random.default_rng(6)
    vox = [(k, k % 3, 0) for k in range(30)]
    order = rng.permutation(np.concatenate([np.repeat(np.arange(k, 30, 3), k + 1) for k in range(3)]))
    ref = _both(vf17, 0.5)
    _add(vf17, ref, _inside([vox[i] for i in order], rng, 0.5))
    for min_points, n in ((1, 30), (2, 20), (3, 10), (4, 0)):
        for counts in (True, False):
            _, c, res = _holds(vf17, ref, min_points=min_points, counts=counts, what=(min_points, counts))
            assert res["n_written"] == n and res["n_voxels"] == 30
            assert not counts or (c >= min_points).all()
    # more voxels than capacity_points: refused with the result filled and nothing written; the exact capacity is enough
    _holds(vf17, ref, capacity=29, what="capacity 29")
    _holds(vf17, ref, capacity=30, what="capacity 30")
    _holds(vf17, ref, min_points=2, capacity=20, what="capacity 20 at min 2")


def test_skipped_records_take_ranks_and_are_counted(vf17):
    rng = np.random.default_rng(7)
    pts = rng.normal(0, 20, (5000, 4)).astype(np.float32)
    bad = np.array([np.nan, np.inf, -np.inf, 3.0e38, -3.0e38, 209715.0, -209715.0, 1.0e6, -0.0, 1e-45], np.float32)
    where = rng.choice(pts[:, :3].size, 1500, replace=False)
    flat = pts[:, :3].copy().reshape(-1)
    flat[where] = bad[rng.integers(0, len(bad), len(where))]
    pts[:, :3] = flat.reshape(-1, 3)
    pts[:, 3] = np.where(rng.random(len(pts)) < 0.3, np.nan, pts[:, 3])         # the 4th float is not looked at
    ref = _both(vf17, 0.2)
    _add(vf17, ref, pts)
    _, _, res = _holds(vf17, ref, what="skips")
    assert res["n_nonfinite"] > 300 and res["n_out_of_range"] > 300 and res["n_accumulated"] > 2000
    assert res["n_accumulated"] + res["n_nonfinite"] + res["n_out_of_range"] == res["n_records"] == 5000
    # 209715 / 0.2 is voxel 2^20 - 1, the last one; 1e6 / 0.2 is out of range
    assert VF.voxel(np.float32(209715.0), VF.inverse(0.2)) == VF.LIMIT - 1 < VF.voxel(np.float32(1.0e6), VF.inverse(0.2))


def test_increments(fx):
    """One add against the same records split 1 + 7 + rest and against add_host (more than one chunk of it); emit twice; add after
    emit; reset with another leaf; max_records hit exactly and passed by one."""
    from lidar_feature_extraction_amd import binding as B
    rng = np.random.default_rng(8)
    n = VF.HOST_CHUNK + 4097
    pts = rng.normal(0, 6, (n, 4)).astype(np.float32)
    vf = fx.voxel_filter(17, n)
    ref = _both(vf, 0.4, 17, n)
    _add(vf, ref, pts)
    whole, wc, res = _holds(vf, ref, what="one add")
    assert 1000 < res["n_voxels"] < n
    again, ac, _ = _holds(vf, ref, what="emit again")
    assert again.tobytes() == whole.tobytes()
    vf.reset(0.4, K.stream())
    d = _up(pts)
    for lo, hi in ((0, 1), (1, 8), (8, n)):
        vf.add(d[lo:hi], stream=K.stream())
    _holds(vf, ref, what="1 + 7 + rest")
    vf.reset(0.4, K.stream())
    vf.add(pts, stream=K.stream())                  # a host array: lfx_voxel_filter_add_host
    _holds(vf, ref, what="add_host")
    # max_records is hit exactly: one more record is refused and nothing is queued
    with pytest.raises(B.LfxError) as e:
        vf.add(d[:1], stream=K.stream())
    assert e.value.code == B.ERR_CAPACITY and ref.add(pts[:1]) == "capacity"
    with pytest.raises(B.LfxError) as e:
        vf.add(pts[:1], stream=K.stream())
    assert e.value.code == B.ERR_CAPACITY and vf.info()["n_records"] == n
    _holds(vf, ref, what="after the refusals")
    # add after emit, then emit again: the restatement of the whole
    half = n // 2 + 13
    ref = _both(vf, 0.4, 17, n)
    _add(vf, ref, pts[:half])
    _holds(vf, ref, what="first half")
    _add(vf, ref, pts[half:])
    grown, gc, _ = _holds(vf, ref, what="both halves")
    assert grown.tobytes() == whole.tobytes() and gc.tolist() == wc.tolist()
    # another leaf on the same table leaves nothing behind
    ref = _both(vf, 1.5, 17, n)
    _add(vf, ref, pts[:3000])
    _, _, res = _holds(vf, ref, what="leaf 1.5")
    assert res["n_records"] == 3000 and vf.info()["leaf"] == 1.5
    vf.close()


def test_arguments(fx, vf17):
    from lidar_feature_extraction_amd import binding as B
    for log2_slots, max_records in ((3, 10), (31, 10), (10, 0), (10, (1 << 40) + 1)):
        with pytest.raises(B.LfxError) as e:
            fx.voxel_filter(log2_slots, max_records)
        assert e.value.code == B.ERR_INVALID_ARGUMENT
    fresh = fx.voxel_filter(4, 16)
    for call in (lambda: fresh.add(np.zeros((1, 4), np.float32)), lambda: fresh.emit()):      # before the first reset
        with pytest.raises(B.LfxError) as e:
            call()
        assert e.value.code == B.ERR_INVALID_ARGUMENT
    for leaf in (0.0, -1.0, float("nan"), float("inf"), 1e-45):
        with pytest.raises(B.LfxError) as e:
            fresh.reset(leaf)
        assert e.value.code == B.ERR_INVALID_ARGUMENT
    fresh.reset(1.0, K.stream())
    rc, _ = fresh.emit_raw(0, 0, 0, 0, K.stream())
    assert rc == B.ERR_INVALID_ARGUMENT
    fresh.close()


def test_add_on_one_stream_and_emit_on_another(fx, vf17):
    """no synchronisation between the two: the filter's event orders them"""
    import torch
    pts = _contended(70001, 256, np.random.default_rng(9))
    d = _up(pts)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    K.sync()
    ref = VF.Filter(17, 1 << 18)
    ref.reset(0.25)
    ref.add(pts)
    vf17.reset(0.25, a.cuda_stream)
    vf17.add(d, stream=b.cuda_stream)
    _holds(vf17, ref, what="streams", stream=a.cuda_stream)
    vf17.add(d, stream=a.cuda_stream)
    ref.add(pts)
    _holds(vf17, ref, what="streams again", stream=b.cuda_stream)


# --- the keyframe store straight into the filter ----------------------------------------------------------------------------------
LEAVES = (0.4, 8.0)          # edge: most voxels hold one record; surface: a few records per voxel, so sums and merges matter


@pytest.fixture(scope="module")
def bits(fx):
    store = KR.bits_case()[0]
    kf = _device_store(fx, store)
    kf.reserve_flags(K.stream())
    n = max(int(store.begin(kind)[-1]) for kind in (0, 1))
    vf = fx.voxel_filter(18, n)
    yield store, kf, vf, n
    vf.close()
    kf.close()


def _from_store(vf, kf, kind, first, count, masked, n):
    vf.reset(LEAVES[kind], K.stream())
    vf.add_keyframes(kf, kind, first, count, masked=masked, stream=K.stream())
    return _emit(vf, n)


def _from_cloud(vf, cloud, kind, n):
    vf.reset(LEAVES[kind], K.stream())
    vf.add(cloud, stream=K.stream())
    return _emit(vf, n)


def _same(a, b, what, ranks=None):
    """two emits gave the same bytes; n_records may differ (a masked add hands a rank to the flagged records too)"""
    (rc_a, res_a, out_a, cnt_a), (rc_b, res_b, out_b, cnt_b) = a, b
    assert rc_a == rc_b == 0, (what, rc_a, rc_b)
    if ranks is not None:
        assert res_a["n_records"] == ranks, (what, res_a, ranks)
        res_a = dict(res_a, n_records=res_b["n_records"])
    assert res_a == res_b, (what, res_a, res_b)
    assert out_a.tobytes() == out_b.tobytes() and cnt_a.tobytes() == cnt_b.tobytes(), what


def test_add_keyframes_is_add_of_the_build(bits):
    """over all keyframes, sub-ranges that start and end inside a workgroup's run, ranges of empty keyframes and an empty range;
    the whole store also against the restatement of the build"""
    store, kf, vf, n = bits
    for kind in (KR.EDGE, KR.SURFACE):
        for first, count in KR.bits_ranges(store.begin(kind)):
            got = _from_store(vf, kf, kind, first, count, False, n)
            want = _from_cloud(vf, kf.build(kind, first, count, stream=K.stream()), kind, n)
            _same(got, want, (kind, first, count))
            assert got[1]["n_records"] == int(store.begin(kind)[first + count] - store.begin(kind)[first])
        ref = VF.Filter(18, n)
        ref.reset(LEAVES[kind])
        ref.add(store.build(kind))
        vf.reset(LEAVES[kind], K.stream())
        vf.add_keyframes(kf, kind, stream=K.stream())
        _, _, res = _holds(vf, ref, what=("restated", kind))
        assert res["n_nonfinite"] > 0 and 1000 < res["n_voxels"] < (res["n_accumulated"] if kind == KR.EDGE else res["n_accumulated"] // 2)
        # keyframe by keyframe is the whole: a map grows this way
        vf.reset(LEAVES[kind], K.stream())
        for first in range(0, len(store), 97):
            vf.add_keyframes(kf, kind, first, min(97, len(store) - first), stream=K.stream())
        _holds(vf, ref, what=("in pieces", kind))


@pytest.mark.parametrize("pattern", ("none", "all", "alternate", "random", "every_other_keyframe", "first_of_each", "last_of_each", "one_run",
                                     "bytes_1_2_255"))
def test_add_keyframes_masked_is_add_of_the_masked_build(bits, pattern):
    """the flag patterns of tests/test_keyframes_masked_gpu.py: every source record takes a rank, the flagged ones nothing else"""
    store, kf, vf, n = bits
    for kind in (KR.EDGE, KR.SURFACE):
        flags = KM.bits_patterns(kind)[pattern]
        d = kf.flags(K.stream())[kind]
        d[:len(flags)].copy_(_up(flags, np.uint8))
        K.sync()
        for first, count in KR.bits_ranges(store.begin(kind))[:3]:
            got = _from_store(vf, kf, kind, first, count, True, n)
            want = _from_cloud(vf, kf.build_masked(kind, d, first, count, stream=K.stream()), kind, n)
            _same(got, want, (pattern, kind, first, count), ranks=int(store.begin(kind)[first + count] - store.begin(kind)[first]))
        if pattern == "random":
            ref = VF.Filter(18, n)
            ref.reset(LEAVES[kind])
            ref.add(store.build(kind), keep=flags == 0)
            vf.reset(LEAVES[kind], K.stream())
            vf.add_keyframes(kf, kind, masked=True, stream=K.stream())
            _holds(vf, ref, what=("restated", kind))
        d.zero_()
    K.sync()


def test_add_keyframes_follows_moved_poses_and_refuses_what_it_must(fx, bits):
    from lidar_feature_extraction_amd import binding as B
    store, kf, vf, n = bits
    before = store.poses().copy()
    kf.set_poses(KR.bits_poses(len(store), 77), 0, K.stream())
    for kind in (KR.EDGE, KR.SURFACE):
        moved = _from_store(vf, kf, kind, 0, len(store), False, n)
        _same(moved, _from_cloud(vf, kf.build(kind, stream=K.stream()), kind, n), ("moved", kind))
    kf.set_poses(before, 0, K.stream())
    for kind in (KR.EDGE, KR.SURFACE):
        back = _from_store(vf, kf, kind, 0, len(store), False, n)
        _same(back, _from_cloud(vf, kf.build(kind, stream=K.stream()), kind, n), ("moved back", kind))
        assert back[2].tobytes() != moved[2].tobytes()
    # refusals: a store without flags, keyframes outside the store, a wrong kind, more records than ranks are left
    plain = _device_store(fx, KR.sphere_case()[0])
    vf.reset(0.4, K.stream())
    calls = [(lambda: vf.add_keyframes(plain, "edge", masked=True), B.ERR_INVALID_ARGUMENT),
             (lambda: vf.add_keyframes(kf, "edge", len(store), 1), B.ERR_INVALID_ARGUMENT),
             (lambda: vf.add_keyframes(kf, "edge", 2, len(store) - 1), B.ERR_INVALID_ARGUMENT)]
    small = fx.voxel_filter(8, 10)
    small.reset(0.4, K.stream())
    calls.append((lambda: small.add_keyframes(plain, "surface"), B.ERR_CAPACITY))
    for call, code in calls:
        with pytest.raises(B.LfxError) as e:
            call()
        assert e.value.code == code
    with pytest.raises(ValueError):
        vf.add_keyframes(kf, 2)
    assert vf.info()["n_records"] == 0 and small.info()["n_records"] == 0
    with pytest.raises(B.LfxError) as e:
        plain.save_filtered(vf, "/nonexistent", masked=True)
    assert e.value.code == B.ERR_INVALID_ARGUMENT
    small.close()
    plain.close()


def test_set_poses_on_the_other_stream_waits_for_a_held_add_keyframes(fx, hold):
    """The reader's half of the two-object call: an add_keyframes queued on a held stream B records the store's event too, so
    a set_poses of other poses issued on A while B is still held does not reach the poses before the add has read them."""
    store = KR.sphere_case()[0]
    kf = _device_store(fx, store)
    n = int(store.begin(KR.EDGE)[-1])
    vf = fx.voxel_filter(12, n)
    want = _from_cloud(vf, kf.build(KR.EDGE, stream=K.stream()), KR.EDGE, n)
    vf.reset(LEAVES[KR.EDGE], K.stream())
    K.sync()
    a, b = S.two_streams()
    hold(b)
    vf.add_keyframes(kf, KR.EDGE, stream=b.cuda_stream)
    e = S.event_behind(b)
    hold.still_held(e, "voxel filter: add_keyframes on B, set_poses of its store on A")
    kf.set_poses(KR.bits_poses(len(store), 78), 0, a.cuda_stream)
    got = _emit(vf, n, stream=b.cuda_stream)
    _same(got, want, "a held reader: the emit of the first poses")
    moved = _from_store(vf, kf, KR.EDGE, 0, len(store), False, n)
    assert moved[0] == 0 and moved[2].tobytes() != got[2].tobytes()       # (and the set_poses did land)
    vf.close()
    kf.close()


def test_save_filtered_writes_the_emitted_clouds(fx, bits, tmp_path):
    from lidar_feature_extraction_amd import read_pcd
    store, kf, vf, n = bits
    flags = [KM.bits_patterns(kind)["random"] for kind in (0, 1)]
    for kind in (0, 1):
        kf.flags(K.stream())[kind][:len(flags[kind])].copy_(_up(flags[kind], np.uint8))
    K.sync()
    for masked in (False, True):
        for min_points in (1, 2):
            where = tmp_path / ("m%d_p%d" % (masked, min_points))
            os.makedirs(where)
            assert kf.save_filtered(vf, str(where), LEAVES, min_points, masked, K.stream()) == (True, True)
            for kind, name in ((KR.EDGE, "edge.pcd"), (KR.SURFACE, "surface.pcd")):
                vf.reset(LEAVES[kind], K.stream())
                vf.add_keyframes(kf, kind, masked=masked, stream=K.stream())
                want, res = vf.emit(min_points, stream=K.stream())
                K.sync()
                got = read_pcd(str(where / name))
                assert res["n_written"] == len(got) > 0 and got[:, :3].tobytes() == want.cpu().numpy()[:, :3].tobytes(), (masked, min_points, kind)
    for kind in (0, 1):
        kf.flags(K.stream())[kind].zero_()
    # an empty kind writes no file, and so does a kind of which no voxel survives
    only = KR.Store(2, (40, 1))
    rng = np.random.default_rng(10)
    assert only.add([rng.normal(0, 30, (20, 4)).astype(np.float32)] * 2, [np.zeros((0, 4), np.float32)] * 2, KR.bits_poses(2, 5)) == 0
    okf = _device_store(fx, only)
    os.makedirs(tmp_path / "edge_only")
    assert okf.save_filtered(vf, str(tmp_path / "edge_only"), LEAVES, 1, False, K.stream()) == (True, False)
    assert os.listdir(tmp_path / "edge_only") == ["edge.pcd"]
    os.makedirs(tmp_path / "none")
    assert okf.save_filtered(vf, str(tmp_path / "none"), LEAVES, 50, False, K.stream()) == (False, False)
    assert os.listdir(tmp_path / "none") == []
    okf.close()


def test_save_filtered_goes_down_in_chunks(fx, tmp_path):
    """More voxels than the store's scratch holds records of (2^20): the file is written from more than one window of places,
    and holds what one emit holds.  Device against device."""
    from lidar_feature_extraction_amd import read_pcd
    rng = np.random.default_rng(11)
    sizes = (700000, 0, 600000)
    big = KR.Store(3, (sum(sizes), 1))
    e = [rng.uniform(-200, 200, (k, 4)).astype(np.float32) for k in sizes]
    assert big.add(e, [np.zeros((0, 4), np.float32)] * 3, KR.bits_poses(3, 6)) == 0
    kf = _device_store(fx, big)
    vf = fx.voxel_filter(22, sum(sizes))
    assert kf.save_filtered(vf, str(tmp_path), (0.05, 0.05), 1, False, K.stream()) == (True, False)
    vf.reset(0.05, K.stream())
    vf.add_keyframes(kf, "edge", stream=K.stream())
    want, res = vf.emit(stream=K.stream())
    K.sync()
    assert res["n_written"] > (1 << 20) + 1000 and res["n_table_full"] == 0
    assert read_pcd(str(tmp_path / "edge.pcd"))[:, :3].tobytes() == want.cpu().numpy()[:, :3].tobytes()
    vf.close()
    kf.close()
