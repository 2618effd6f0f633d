"""The flags a keyframe store keeps, the masked submap and the masked save on the device (lfx_keyframes_reserve_flags ..
lfx_keyframes_save_masked, include/lfx.h) against their restatement (tests/keyframes_mask_restatement.py): every cloud, the
guard records behind it, every result record and every flag byte are compared byte for byte -- nothing here has a tolerance.
tests/test_keyframes_masked_expect.py holds the restatement to hand cases and the bits case to the conditions used here.

The count and the scatter of the masked submap work in runs of lfx::kKfRun = 1024 source records counted from the first
record of the WINDOW, lane t of a workgroup on the records 4 t .. 4 t + 3 of its run and a wave on 256 consecutive ones
(csrc/lfx_kernels_keyframes.hpp)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import deskew_cases as K
from tests import keyframes_mask_restatement as KM
from tests import keyframes_restatement as KR
from tests import segment_cases as S
from tests.test_keyframes_gpu import GUARD, _bytes, _device_store, _state, _up

pytestmark = pytest.mark.gpu
FILL = -123.25


@pytest.fixture(scope="module")
def fx():
    f = K.fx_for(16, 64, 3)
    yield f
    f.close()


def _put(kf, kind, flags):
    """the store's flags of `kind` written through flags(): the records' bytes from `flags`"""
    d = kf.flags(K.stream())[kind]
    if len(flags):
        d[:len(flags)].copy_(_up(flags, np.uint8))
    K.sync()


def _masked_guarded(kf, store, flags, kind, center, radius, first, count, capacity, world=None, stream=None):
    """one masked submap into a buffer with GUARD records behind the capacity: cloud, guards and result are the restatement's"""
    import torch
    want, wres = KM.submap_masked(store, flags, kind, center, radius, first, count, capacity, world=world)
    out = torch.full((capacity + GUARD, 4), FILL, dtype=torch.float32, device=K.dev())
    _, res = kf.submap_masked(kind, center, radius, first, len(store) - first if count is None else count, d_out=out.data_ptr(),
                              capacity_points=capacity, stream=K.stream() if stream is None else stream)
    K.sync()
    host = out.cpu().numpy()
    what = (kind, radius, first, count, capacity)
    assert res == wres, (what, res, wres)
    assert host[:len(want)].tobytes() == want.tobytes(), (what, int((host[:len(want)].view(np.uint32) != want.view(np.uint32)).any(axis=1).sum()))
    assert (host[len(want):] == FILL).all(), what
    return res


@pytest.fixture(scope="module")
def bits(fx):
    store = KR.bits_case()[0]
    kf = _device_store(fx, store)
    kf.reserve_flags(K.stream())
    world = [store.build(kind) for kind in (KR.EDGE, KR.SURFACE)]
    yield store, kf, world
    kf.close()


def _selections(store):
    """(centre, radius) by name over bits_poses: all, none, exactly one keyframe, about half"""
    t = store.poses()[:, :, 3]
    sel = {"all": ([0.0, 0.0, 0.0], 1e4), "none": ([1e5, 0.0, 0.0], 1.0), "one": (t[417].tolist(), 0.0), "half": ([0.0, 0.0, 0.0], 92.0)}
    n = {name: int(store.select(c, r).sum()) for name, (c, r) in sel.items()}
    assert n["all"] == len(store) and n["none"] == 0 and n["one"] == 1 and 0.3 * len(store) < n["half"] < 0.7 * len(store), n
    return sel


PATTERNS = ("none", "all", "alternate", "random", "every_other_keyframe", "first_of_each", "last_of_each", "one_run", "bytes_1_2_255")


@pytest.mark.parametrize("pattern", PATTERNS)
def test_submap_masked_bits(bits, pattern):
    store, kf, world = bits
    sel = _selections(store)
    for kind in (KR.EDGE, KR.SURFACE):
        flags = KM.bits_patterns(kind)[pattern]
        _put(kf, kind, flags)
        begin = store.begin(kind).astype(np.int64)
        keep = np.concatenate([[0], np.cumsum(flags == 0)])
        windows = [(0, len(store))] + [w for w in KR.bits_ranges(store.begin(KR.EDGE))[1:3]]
        for first, count in windows:
            for name, (center, radius) in sel.items():
                ids = first + np.nonzero(store.select(center, radius, first, count))[0]
                kept = keep[begin[ids + 1]] - keep[begin[ids]]
                total = int(kept.sum())
                capacities = [total]
                if name in ("all", "half") and first == 0:
                    prefix = np.cumsum(kept)
                    at = [int(prefix[len(ids) * q // 4]) for q in (1, 2, 3)]
                    capacities += [max(total - 1, 0), 0] + [max(p + d, 0) for p in at for d in (-1, 0, 1)]
                for capacity in capacities:
                    res = _masked_guarded(kf, store, flags, kind, center, radius, first, count, capacity, world[kind])
                    assert res["n_selected"] == len(ids)
                    if capacity == total:
                        assert res["n_points"] == total and not res["truncated"]
        assert kf.flags_info(K.stream())["n_flagged"][kind] == int(np.count_nonzero(flags))


def test_zero_flags_give_submaps_bytes_and_the_cloud_is_the_masked_builds_concatenated(bits):
    """Device against device: with no flag set, lfx_keyframes_submap's cloud and record; with flags, the concatenation of
    lfx_keyframes_build_masked(kind, the store's flags, k, 1) over the written keyframes."""
    import torch
    store, kf, world = bits
    sel = _selections(store)
    for kind in (KR.EDGE, KR.SURFACE):
        n = int(store.begin(kind)[-1])
        _put(kf, kind, np.zeros(n, np.uint8))
        for name, (center, radius) in sel.items():
            for first, count, capacity in ((0, len(store), n), (195, 400, n), (0, len(store), n // 3), (0, len(store), 0)):
                plain, pres = kf.submap(kind, center, radius, first, count, capacity_points=capacity, stream=K.stream())
                masked, mres = kf.submap_masked(kind, center, radius, first, count, capacity_points=capacity, stream=K.stream())
                K.sync()
                assert pres == mres and plain.cpu().numpy().tobytes() == masked.cpu().numpy().tobytes(), (kind, name, first, count, capacity)
        flags = KM.bits_patterns(kind)["random"]
        _put(kf, kind, flags)
        d_flags = kf.flags(K.stream())[kind]
        center, radius = sel["half"]
        cloud, res = kf.submap_masked(kind, center, radius, 0, len(store), capacity_points=n // 8, stream=K.stream())
        K.sync()
        assert res["truncated"] and res["n_written_keyframes"] > 5
        written = [int(k) for k in np.nonzero(store.select(center, radius))[0]][:res["n_written_keyframes"]]
        assert written[0] == res["first_id"] and written[-1] == res["last_id"]
        parts = [kf.build_masked(kind, d_flags, k, 1, stream=K.stream()) for k in written]
        K.sync()
        assert torch.cat(parts).cpu().numpy().tobytes() == cloud.cpu().numpy().tobytes()


def test_flag_calls(fx):
    """reserve after adds reads as zeros and is idempotent; set_flags / clear_flags on sub-ranges leave what the restatement
    holds and write nothing outside the range (a sentinel through flags() surrounds it); flags_info counts on the device."""
    import torch
    store = KR.sphere_case()[0]
    kf = _device_store(fx, store)
    info0 = kf.info()
    assert kf.flags_info(K.stream()) == dict(reserved=False, device_bytes=0, n_flagged=(0, 0))
    kf.reserve_flags(K.stream())
    ptrs = [t.data_ptr() for t in kf.flags(K.stream())]
    fi = kf.flags_info(K.stream())
    assert fi["reserved"] and fi["n_flagged"] == (0, 0) and fi["device_bytes"] >= sum(store.max_points) + 16 * store.max_keyframes
    kf.reserve_flags(K.stream())
    assert [t.data_ptr() for t in kf.flags(K.stream())] == ptrs and kf.flags_info(K.stream()) == fi and kf.info() == info0
    for kind in (KR.EDGE, KR.SURFACE):
        d = kf.flags(K.stream())[kind]
        K.sync()
        assert d.dtype == torch.uint8 and d.numel() == store.max_points[kind] and not d.cpu().numpy().any()
    rng = np.random.default_rng(61)
    want = [np.zeros(store.max_points[kind], np.uint8) for kind in (KR.EDGE, KR.SURFACE)]
    for kind in (KR.EDGE, KR.SURFACE):
        n = int(store.begin(kind)[-1])
        src = rng.choice(np.array([0, 1, 2, 255], np.uint8), store.max_points[kind])
        d_src = _up(src, np.uint8)
        for first, count in ((2, 3), (0, 1), (6, 1), (3, 1), (1, 0), (0, len(store))):
            # the sentinel: every byte of the store's array, the range's too; the call rewrites the range and nothing else
            want[kind][:] = 0x5C
            kf.flags(K.stream())[kind].fill_(0x5C)
            K.sync()
            kf.set_flags(kind, d_src, first, count, K.stream())
            KM.set_flags(store, want[kind], kind, src, first, count)
            K.sync()
            assert kf.flags(K.stream())[kind].cpu().numpy().tobytes() == want[kind].tobytes(), (kind, first, count)
        for first, count in ((1, 2), (3, 1), (5, 2)):
            kf.clear_flags(kind, first, count, K.stream())
            KM.clear_flags(store, want[kind], kind, first, count)
            K.sync()
            assert kf.flags(K.stream())[kind].cpu().numpy().tobytes() == want[kind].tobytes(), (kind, first, count)
        assert (want[kind][:n] == 0).any() and (want[kind][:n] != 0).any()
        # (the bytes behind n_points are the store's: zero again before anything counts or masks)
        kf.flags(K.stream())[kind][n:].zero_()
        want[kind][n:] = 0
    K.sync()
    assert kf.flags_info(K.stream())["n_flagged"] == KM.n_flagged(store, want)
    c = KR.sphere_case()[1]
    for kind in (KR.EDGE, KR.SURFACE):
        for capacity in (64, 7, 3, 0):
            _masked_guarded(kf, store, want[kind], kind, c, 7.0, 0, None, capacity)
    kf.close()


def test_hand_flags_on_the_device(fx):
    from tests.test_keyframes_masked_expect import HAND_FLAGS
    store, c, _, _, _ = KR.sphere_case()
    kf = _device_store(fx, store)
    kf.reserve_flags(K.stream())
    kf.set_flags("edge", _up(HAND_FLAGS, np.uint8), 0, len(store), K.stream())
    for capacity, radius, first, count in ((64, 7.0, 0, None), (12, 7.0, 0, None), (11, 7.0, 0, None), (7, 7.0, 0, None), (6, 7.0, 0, None),
                                           (0, 7.0, 0, None), (0, 7.0, 2, 2), (64, 5.0, 0, None), (64, 7.0, 4, 3), (64, 0.5, 0, None), (64, 7.0, 2, 0)):
        _masked_guarded(kf, store, HAND_FLAGS, KR.EDGE, c, radius, first, count, capacity)
    kf.close()


def test_refusals_leave_everything_as_it_was(fx, tmp_path):
    import torch
    from lidar_feature_extraction_amd import binding as B
    store, c, _, _, _ = KR.sphere_case()
    kf = _device_store(fx, store)
    L, ctx, st = fx._L, fx._ctx, C.c_void_p(K.stream())
    out = torch.full((64 + GUARD, 4), FILL, dtype=torch.float32, device=K.dev())
    cc = np.ascontiguousarray(c, np.float64)
    pc = C.c_void_p(cc.ctypes.data)
    r = B.KeyframesSubmapResult()
    w = (C.c_int32 * 2)(5, 5)
    p2 = (C.c_void_p * 2)()
    v0, before = _state(kf)
    clouds = [kf.build(kind).cpu().numpy().tobytes() for kind in (0, 1)]

    def unchanged():
        K.sync()
        v1, after = _state(kf)
        assert v0 == v1 and before == after and (out.cpu().numpy() == FILL).all()
        assert [kf.build(kind).cpu().numpy().tobytes() for kind in (0, 1)] == clouds
        for kind in (KR.EDGE, KR.SURFACE):
            cloud, res = kf.submap(kind, c, 7.0, stream=K.stream())
            K.sync()
            want = store.submap(kind, c, 7.0, 0, None, int(store.begin(kind)[-1]))
            assert res == want[1] and cloud.cpu().numpy().tobytes() == want[0].tobytes()

    def refused(rc, what=None):
        """the call answered LFX_ERR_INVALID_ARGUMENT, and build, submap, the store's bytes and its flags are as they were"""
        assert rc == B.ERR_INVALID_ARGUMENT, what
        unchanged()
        if kf.flags_info(K.stream())["reserved"]:
            assert kf.flags_info(K.stream())["n_flagged"] == (0, 0) and not any(t.cpu().numpy().any() for t in kf.flags(K.stream()))

    # before the reserve: every masked call and flags()
    refused(L.lfx_keyframes_flags(ctx, kf.handle, p2, st))
    refused(L.lfx_keyframes_set_flags(ctx, kf.handle, 0, 0, 1, C.c_void_p(out.data_ptr()), st))
    refused(L.lfx_keyframes_clear_flags(ctx, kf.handle, 0, 0, 1, st))
    refused(L.lfx_keyframes_submap_masked(ctx, kf.handle, 0, pc, 7.0, 0, len(store), C.c_void_p(out.data_ptr()), 64, C.byref(r), st))
    refused(L.lfx_keyframes_save_masked(ctx, kf.handle, os.fsencode(str(tmp_path)), w, st))
    assert os.listdir(tmp_path) == []
    with pytest.raises(B.LfxError) as err:
        kf.submap_masked("edge", c, 7.0, stream=K.stream())
    assert err.value.code == B.ERR_INVALID_ARGUMENT and "reserve_flags" in str(err.value)
    assert kf.flags_info(K.stream()) == dict(reserved=False, device_bytes=0, n_flagged=(0, 0))
    kf.reserve_flags(K.stream())
    src = _up(np.ones(store.max_points[0], np.uint8), np.uint8)
    bad_center = np.array([1.0, np.nan, 3.0])
    inf_center = np.array([np.inf, 2.0, 3.0])
    good = (ctx, kf.handle, 0, pc, 7.0, 0, len(store), C.c_void_p(out.data_ptr()), 64, C.byref(r))
    calls = []
    # NULL ctx, store, centre and result; a bad kind; a window past the store; a radius and a centre that are not finite
    for i, bad in ((0, None), (1, None), (3, None), (9, None), (2, 2), (2, -1), (5, len(store) + 1), (6, len(store) + 1), (4, float("nan")), (4, -1.0),
                   (4, float("inf")), (3, C.c_void_p(bad_center.ctypes.data)), (3, C.c_void_p(inf_center.ctypes.data))):
        a = list(good)
        a[i] = bad
        calls.append(a)
    calls.append([ctx, kf.handle, 0, pc, 7.0, 3, len(store) - 2] + list(good[7:]))
    for a in calls:
        refused(L.lfx_keyframes_submap_masked(*a, st), a[2:7])
    # d_out NULL with records to write -- and without any (nothing selected): LFX_OK
    refused(L.lfx_keyframes_submap_masked(ctx, kf.handle, 0, pc, 7.0, 0, len(store), None, 64, C.byref(r), st))
    assert L.lfx_keyframes_submap_masked(ctx, kf.handle, 0, pc, 0.5, 0, len(store), None, 64, C.byref(r), st) == 0 and r.n_points == 0
    for a in ((None, kf.handle, 0, 0, 1, C.c_void_p(src.data_ptr())), (ctx, None, 0, 0, 1, C.c_void_p(src.data_ptr())), (ctx, kf.handle, 0, 0, 1, None),
              (ctx, kf.handle, 2, 0, 1, C.c_void_p(src.data_ptr())), (ctx, kf.handle, 0, len(store), 1, C.c_void_p(src.data_ptr())),
              (ctx, kf.handle, 0, 2, len(store) - 1, C.c_void_p(src.data_ptr()))):
        refused(L.lfx_keyframes_set_flags(*a, st), a[2:5])
    for a in ((None, kf.handle, 0, 0, 1), (ctx, None, 0, 0, 1), (ctx, kf.handle, 2, 0, 1), (ctx, kf.handle, 0, len(store), 1), (ctx, kf.handle, 1, 2, len(store) - 1)):
        refused(L.lfx_keyframes_clear_flags(*a, st), a[2:5])
    fi = B.KeyframesFlagsInfo()
    refused(L.lfx_keyframes_flags(ctx, kf.handle, None, st))
    refused(L.lfx_keyframes_flags(None, kf.handle, p2, st))
    refused(L.lfx_keyframes_flags_info(ctx, kf.handle, None, st))
    refused(L.lfx_keyframes_flags_info(ctx, None, C.byref(fi), st))
    refused(L.lfx_keyframes_reserve_flags(None, kf.handle, st))
    refused(L.lfx_keyframes_reserve_flags(ctx, None, st))
    refused(L.lfx_keyframes_save_masked(ctx, kf.handle, None, w, st))
    refused(L.lfx_keyframes_save_masked(ctx, kf.handle, os.fsencode(str(tmp_path)), None, st))
    assert os.listdir(tmp_path) == []
    kf.close()


@pytest.fixture(scope="module")
def hold():
    h = S.Hold()
    yield h
    for what, ms in h.issue_ms:
        print("held %.0f ms; issued %.3f ms after the hold was queued: %s" % (S.HOLD_MS, ms, what))


def test_a_masked_submap_is_ordered_behind_the_flags_producer(fx, hold):
    """As test_calls_on_three_streams_are_ordered_one_behind_the_other (tests/test_keyframes_gpu.py): the producer's stream is
    held, an event behind the producer says it has not run, the masked submap goes to another stream and its cloud is the
    one the producer leaves.  (1) set_flags on held A, submap_masked on B.  (2) lfx_visibility_run into the store's flags
    on held A -- a call that waits for its result, so the hold is asserted before it is issued -- then submap_masked on B."""
    import torch
    from tests import visibility_cases as VC
    from tests.test_visibility_gpu import _device_store as _vis_store
    from tests.visibility_restatement import Rule
    store, _ = VC.scene_case()
    rule = Rule(**VC.SCENE)
    kf = _vis_store(fx, store)
    kf.reserve_flags(K.stream())
    vis = fx.visibility(8, 8, **rule.fields())
    a, b = S.two_streams()
    n = [int(store.begin(kind)[-1]) for kind in (0, 1)]
    center, radius = store.poses()[3, :, 3], 1e3
    rng = np.random.default_rng(71)
    drawn = (rng.random(n[0]) < 0.4).astype(np.uint8)
    d_drawn = _up(drawn, np.uint8)
    outs = [torch.full((n[0] + GUARD, 4), FILL, dtype=torch.float32, device=K.dev()) for _ in range(3)]
    scratch = tuple(torch.zeros(max(n[k], 1), dtype=torch.uint8, device=K.dev()) for k in range(2))
    for st in (a, b):                          # warm: nothing below allocates or loads a kernel
        hold._run(1, st)
        kf.set_flags("edge", d_drawn, 0, 1, st.cuda_stream)
        kf.submap_masked("edge", center, radius, d_out=outs[2].data_ptr(), capacity_points=n[0], stream=st.cuda_stream)
        vis.run(kf, 0, len(store), flags=scratch, stream=st.cuda_stream)
    kf.clear_flags("edge", 0, len(store), K.stream())
    K.sync()

    def check(out, res, flags):
        b.synchronize()
        want, wres = KM.submap_masked(store, flags, KR.EDGE, center, radius, 0, None, n[0])
        host = out.cpu().numpy()
        assert res == wres and 0 < wres["n_points"] < int((store.select(center, radius) * np.diff(store.begin(0).astype(np.int64))).sum())
        assert host[:len(want)].tobytes() == want.tobytes() and (host[len(want):] == FILL).all()

    # (1)
    hold(a)
    kf.set_flags("edge", d_drawn, 0, len(store), a.cuda_stream)
    e = S.event_behind(a)
    hold.still_held(e, "keyframes: set_flags on A, submap_masked on B")
    _, res = kf.submap_masked("edge", center, radius, d_out=outs[0].data_ptr(), capacity_points=n[0], stream=b.cuda_stream)
    check(outs[0], res, drawn)
    # (2)
    K.sync()
    voted = rule.run(store)[1]
    assert voted[0].any() and voted[0].tobytes() != drawn.tobytes()
    hold(a)
    e = S.event_behind(a)
    hold.still_held(e, "keyframes: visibility run into the store's flags on A, submap_masked on B")
    vis.run(kf, 0, len(store), flags=kf.flags(a.cuda_stream), stream=a.cuda_stream)
    _, res = kf.submap_masked("edge", center, radius, d_out=outs[1].data_ptr(), capacity_points=n[0], stream=b.cuda_stream)
    check(outs[1], res, voted[0])
    K.sync()
    vis.close()
    kf.close()


def test_visibility_votes_into_the_stores_flags(fx):
    """Visibility.run with the store's flags writes the bytes a run into the caller's buffers writes, and the masked submap
    under them is the restatement's under the restatement's votes."""
    from tests import visibility_cases as VC
    from tests.test_visibility_gpu import _device_store as _vis_store
    from tests.visibility_restatement import Rule
    store, _ = VC.scene_case()
    rule = Rule(**VC.SCENE)
    kf = _vis_store(fx, store)
    kf.reserve_flags(K.stream())
    vis = fx.visibility(8, 4, **rule.fields())
    own, _, res_own = vis.run(kf, 0, len(store), stream=K.stream())
    mine, _, res_store = vis.run(kf, 0, len(store), flags=kf.flags(K.stream()), stream=K.stream())
    K.sync()
    voted = rule.run(store)[1]
    assert res_own == res_store and sum(res_store["n_dynamic"]) > 0
    assert kf.flags_info(K.stream())["n_flagged"] == tuple(res_store["n_dynamic"])
    for kind in (KR.EDGE, KR.SURFACE):
        n = int(store.begin(kind)[-1])
        got = mine[kind].cpu().numpy()
        assert got[:n].tobytes() == own[kind].cpu().numpy()[:n].tobytes() == voted[kind].tobytes() and not got[n:].any()
        for center, radius, capacity in ((store.poses()[3, :, 3], 6.0, n), (store.poses()[0, :, 3], 1e3, n), (store.poses()[0, :, 3], 1e3, n // 2)):
            _masked_guarded(kf, store, voted[kind], kind, center, radius, 0, None, capacity)
    vis.close()
    kf.close()


def test_save_masked_writes_the_masked_builds(fx, tmp_path):
    from lidar_feature_extraction_amd import read_pcd
    store, c, edge, surface, poses = KR.sphere_case()
    kf = _device_store(fx, store)
    kf.reserve_flags(K.stream())
    rng = np.random.default_rng(81)
    flags = [(rng.random(int(store.begin(kind)[-1])) < 0.4).astype(np.uint8) * 3 for kind in (0, 1)]
    for kind in (0, 1):
        _put(kf, kind, flags[kind])
    os.makedirs(tmp_path / "both")
    assert kf.save_masked(str(tmp_path / "both"), K.stream()) == (True, True)
    for kind, name in ((KR.EDGE, "edge.pcd"), (KR.SURFACE, "surface.pcd")):
        got = read_pcd(str(tmp_path / "both" / name))
        want = kf.build_masked(kind, kf.flags(K.stream())[kind]).cpu().numpy()
        assert 0 < len(want) < int(store.begin(kind)[-1])
        assert got[:, :3].tobytes() == want[:, :3].tobytes() == KM.build_masked(store, flags[kind], kind)[:, :3].tobytes()
    # a kind that is fully flagged writes no file
    _put(kf, KR.SURFACE, np.full(int(store.begin(KR.SURFACE)[-1]), 9, np.uint8))
    os.makedirs(tmp_path / "edge_only")
    assert kf.save_masked(str(tmp_path / "edge_only"), K.stream()) == (True, False)
    assert os.listdir(tmp_path / "edge_only") == ["edge.pcd"]
    kf.close()
    # more records than the save's chunk (2^20): the second chunk begins inside the last keyframe; p = 0.3; an empty kind
    sizes = (600000, 0, 500000)
    only = KR.Store(3, (sum(sizes), 1))
    e = [rng.normal(0, 30, (k, 4)).astype(np.float32) for k in sizes]
    assert only.add(e, [np.zeros((0, 4), np.float32)] * 3, poses[:3]) == 0
    kf = _device_store(fx, only)
    kf.reserve_flags(K.stream())
    big = (rng.random(sum(sizes)) < 0.3).astype(np.uint8)
    _put(kf, KR.EDGE, big)
    os.makedirs(tmp_path / "big")
    assert kf.save_masked(str(tmp_path / "big"), K.stream()) == (True, False)
    assert os.listdir(tmp_path / "big") == ["edge.pcd"]
    want = kf.build_masked("edge", kf.flags(K.stream())[0]).cpu().numpy()
    assert len(want) == int((big == 0).sum())
    assert read_pcd(str(tmp_path / "big" / "edge.pcd"))[:, :3].tobytes() == want[:, :3].tobytes() == only.build(KR.EDGE)[big == 0][:, :3].tobytes()
    kf.close()
