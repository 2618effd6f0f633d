"""The visibility votes and the masked build on the device (lfx_visibility_*, lfx_keyframes_build_masked, include/lfx.h)
against their restatement (tests/visibility_restatement.py) over the cases of tests/visibility_cases.py: vote words, flag
bytes, every field of the result and every masked cloud are compared byte for byte -- nothing here has a tolerance.
tests/test_visibility_expect.py holds the cases to what they claim to be."""
import ctypes as C

import numpy as np
import pytest

from tests import deskew_cases as K
from tests import keyframes_restatement as KR
from tests import segment_cases as S
from tests import visibility_cases as VC
from tests.visibility_restatement import Rule, build_masked

pytestmark = pytest.mark.gpu
GUARD = 64                                   # guard records behind a masked build's n_out
FLAG_FILL, VOTE_FILL = 0xAB, 0x5A5A5A5A      # what flags and votes hold before a run: records outside the window keep it


def _up(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype).copy()).to(K.dev())


def _device_store(fx, store):
    """a device store of the restatement's capacities holding its keyframes, added in one call from packed device clouds"""
    from lidar_feature_extraction_amd import Keyframes
    kf = fx.keyframes(store.max_keyframes, store.max_points)
    packed = []
    for kind in range(2):
        counts = np.array([len(c) for c in store.clouds[kind]], np.uint32)
        begins = (np.cumsum(counts) - counts).astype(np.uint32)
        rec = store.records(kind)
        packed.append((_up(rec if len(rec) else np.zeros((1, 4), np.float32)), _up(begins, np.uint32), _up(counts, np.uint32), len(rec)))
    clouds = [Keyframes.clouds(p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), 1, p[3]) for p in packed]
    assert kf.add(clouds[0], clouds[1], store.poses(), K.stream()) == 0
    K.sync()
    return kf


def _fills(store):
    import torch
    n = [int(store.begin(kind)[-1]) for kind in range(2)]
    flags = tuple(torch.full((max(n[k], 1),), FLAG_FILL, dtype=torch.uint8, device=K.dev()) for k in range(2))
    votes = tuple(torch.full((max(n[k], 1),), VOTE_FILL, dtype=torch.int32, device=K.dev()) for k in range(2))
    return n, flags, votes


def _run_and_compare(vis, kf, store, rule, first, count, resident, with_votes=True, stream=None):
    """one device run into prefilled tensors against the restatement run into the same fills: every byte and every field"""
    n, flags, votes = _fills(store)
    got_flags, got_votes, res = vis.run(kf, first, count, votes=votes if with_votes else False, flags=flags, stream=K.stream() if stream is None else stream)
    K.sync()
    want_votes, want_flags, want = rule.run(store, first, count, resident, votes=[np.full(n[k], VOTE_FILL, np.uint32) for k in range(2)],
                                            flags=[np.full(n[k], FLAG_FILL, np.uint8) for k in range(2)])
    for k in range(2):
        f = got_flags[k].cpu().numpy()[:n[k]]
        assert f.tobytes() == want_flags[k].tobytes(), (k, first, count, resident, int((f != want_flags[k]).sum()))
        if with_votes:
            v = got_votes[k].cpu().numpy().view(np.uint32)[:n[k]]
            assert v.tobytes() == want_votes[k].tobytes(), (k, first, count, resident, int((v != want_votes[k]).sum()))
    assert res == want, (res, want)
    return [f.cpu().numpy()[:n[k]] for k, f in enumerate(got_flags)], res


@pytest.fixture(scope="module")
def fx():
    f = K.fx_for(16, 64, 3)
    yield f
    f.close()


@pytest.mark.parametrize("g", VC.hand_groups(), ids=lambda g: g.name)
def test_hand_cases(fx, g):
    store, rule = g.store(), Rule(**g.fields)
    first, count = g.window()
    kf = _device_store(fx, store)
    for resident in (len(store), 1):             # all images at once; one viewer per chunk: a word collects its votes over the chunks
        vis = fx.visibility(len(store), resident, **rule.fields())
        flags, res = _run_and_compare(vis, kf, store, rule, first, count, resident)
        _run_and_compare(vis, kf, store, rule, first, count, resident, with_votes=False)
        vis.close()
    for name, p in g.probes.items():             # ... and the words written beside the probes, once more from the device's flags
        if p["dynamic"] is not None:
            kind, i = g.where(name)
            assert flags[kind][i] == p["dynamic"], name
    kf.close()


@pytest.fixture(scope="module")
def layout(fx):
    store = VC.layout_case()
    kf = _device_store(fx, store)
    yield store, kf
    kf.close()


@pytest.mark.parametrize("window", VC.LAYOUT_WINDOWS)
def test_layout_case_whatever_the_chunks(fx, layout, window):
    store, kf = layout
    rule = Rule(**VC.LAYOUT)
    first, count = window
    seen = []
    for resident in (count, 1, 3):
        vis = fx.visibility(count, resident, **rule.fields())
        flags, res = _run_and_compare(vis, kf, store, rule, first, count, resident)
        _run_and_compare(vis, kf, store, rule, first, count, resident, with_votes=False)    # the object's own words between chunks
        assert res["n_viewer_chunks"] == -(-(res["total_cells"] // 32) // resident)
        seen.append((flags[0].tobytes(), flags[1].tobytes(), {k: v for k, v in res.items() if k != "n_viewer_chunks"}))
        vis.close()
    assert seen[0] == seen[1] == seen[2]


@pytest.fixture(scope="module")
def scene(fx):
    store, classes = VC.scene_case()
    kf = _device_store(fx, store)
    yield store, kf, classes
    kf.close()


@pytest.mark.parametrize("guard", [1, 0])
def test_scene(fx, scene, guard):
    store, kf, classes = scene
    rule = Rule(**dict(VC.SCENE, guard=guard))
    vis = fx.visibility(8, 4, **rule.fields())
    info = vis.info()
    assert info["max_window"] == 8 and info["max_resident_images"] == 4 and info["config"]["n_columns"] == 180
    assert info["device_bytes"] >= 4 * 4 * 16 * 180 + 8 * (2 * 180 + 17) + 4 * 8
    flags, res = _run_and_compare(vis, kf, store, rule, 0, len(store), 4)
    assert res["n_viewer_chunks"] == 2 and res["n_pairs"] == 30 and res["occupied_cells"] > 0.9 * res["total_cells"]
    moving = sum(int(flags[k][classes[k] == VC.MOVING].sum()) for k in range(2))
    print("guard %d: %s; %d records of the moving pillar flagged" % (guard, res, moving))
    vis.close()


def _masked_guarded(kf, store, kind, flags, d_flags, first, count):
    """a masked build into a buffer with GUARD records behind the cloud, and its begins, against the restatement"""
    import torch
    want, want_begin = build_masked(store, kind, flags, first, count)
    n = len(want)
    out = torch.full((n + GUARD, 4), -123.25, dtype=torch.float32, device=K.dev())
    (got, begins) = kf.build_masked(kind, d_flags, first, count, begins=True, d_out=out.data_ptr(), capacity_points=n, stream=K.stream())
    K.sync()
    host = out.cpu().numpy()
    assert got == n, (kind, first, count, got, n)
    assert host[:n].tobytes() == want.tobytes(), (kind, first, count, int((host[:n].view(np.uint32) != want.view(np.uint32)).any(axis=1).sum()))
    assert (host[n:] == -123.25).all(), (kind, first, count)
    assert begins.cpu().numpy().view(np.uint64).tobytes() == want_begin.tobytes(), (kind, first, count)
    return n


def test_build_masked(fx, layout, scene):
    import torch
    from lidar_feature_extraction_amd import binding as B
    for store, kf in (layout, scene[:2]):
        n_kf = len(store)
        for kind in (KR.EDGE, KR.SURFACE):
            total = int(store.begin(kind)[-1])
            rng = np.random.default_rng(77 + kind)
            # the restatement's flags of a whole-store run (bytes 0 / 1), and drawn bytes of any value in long and short runs
            rule = Rule(**(VC.LAYOUT if store is layout[0] else VC.SCENE))
            voted = rule.run(store)[1][kind]
            drawn = (rng.integers(0, 256, total) * (rng.uniform(0, 1, total) < 0.3)).astype(np.uint8)
            drawn[total // 3:total // 3 + 3000] = 7
            drawn[total // 2:total // 2 + 2500] = 0
            ranges = [(0, n_kf), (1, n_kf - 2), (n_kf - 1, 1), (2, 0)]
            if store is layout[0]:
                ranges += KR.bits_ranges(store.begin(KR.EDGE)) + [VC.LAYOUT_WINDOWS[1]]      # (keyframe ranges: the edge counts' shapes)
            for flags in (voted, drawn):
                d_flags = _up(flags if total else np.zeros(1, np.uint8), np.uint8)
                for first, count in ranges:
                    _masked_guarded(kf, store, kind, flags, d_flags, first, count)
            # no flag set: build's bytes; every flag set: nothing
            zeros, ones = np.zeros(total, np.uint8), np.full(total, 255, np.uint8)
            d_zeros, d_ones = _up(zeros, np.uint8), _up(ones, np.uint8)
            assert _masked_guarded(kf, store, kind, zeros, d_zeros, 0, n_kf) == total
            assert kf.build_masked(kind, d_zeros).cpu().numpy().tobytes() == kf.build(kind).cpu().numpy().tobytes() == store.build(kind).tobytes()
            assert _masked_guarded(kf, store, kind, ones, d_ones, 0, n_kf) == 0
            # one record short: refused with the records needed, and nothing written
            need = int((drawn == 0).sum())
            out = torch.full((need + GUARD, 4), -123.25, dtype=torch.float32, device=K.dev())
            n = C.c_uint64(0)
            rc = fx._L.lfx_keyframes_build_masked(fx._ctx, kf.handle, kind, 0, n_kf, C.c_void_p(_up(drawn, np.uint8).data_ptr()), C.c_void_p(out.data_ptr()),
                                                  need - 1, None, C.byref(n), C.c_void_p(K.stream()))
            K.sync()
            assert rc == B.ERR_CAPACITY and n.value == need and (out.cpu().numpy() == -123.25).all()


def test_a_run_sees_the_poses_followed_on_the_other_stream(fx, scene):
    """lfx_keyframes_follow with other poses on held A, then at once a run on B: the run waits for the store's event and votes
    at the new poses.  Its flags and votes are read behind B alone."""
    import torch
    hold = S.Hold()
    store, kf, _ = scene
    rule = Rule(**VC.SCENE)
    moved = KR.Store(store.max_keyframes, store.max_points)
    poses = store.poses().copy()
    poses[:, 0, 3] += np.arange(len(store)) * 0.25               # another trajectory: other votes
    assert moved.add(store.clouds[0], store.clouds[1], poses) == 0
    vis = fx.visibility(8, 8, **rule.fields())
    _run_and_compare(vis, kf, store, rule, 0, len(store), 8)     # warm: nothing below allocates or loads a kernel
    a, b = S.two_streams()
    d_poses = _up(poses.reshape(-1, 12), np.float64)
    K.sync()
    n, flags, votes = _fills(store)
    hold(a)
    kf.follow(d_poses.data_ptr(), 0, len(store), a.cuda_stream)
    e = S.event_behind(a)
    hold.still_held(e, "visibility: follow on A, run on B")
    _, _, res = vis.run(kf, 0, len(store), votes=votes, flags=flags, stream=b.cuda_stream)
    with torch.cuda.stream(b):
        got = [t.to("cpu", non_blocking=False).numpy() for t in flags + votes]
    want_votes, want_flags, want = rule.run(moved, 0, len(store), 8)
    old_votes = rule.run(store, 0, len(store), 8)[0]
    assert res == want
    for k in range(2):
        assert got[k][:n[k]].tobytes() == want_flags[k].tobytes() and got[2 + k].view(np.uint32)[:n[k]].tobytes() == want_votes[k].tobytes()
        assert want_votes[k].tobytes() != old_votes[k].tobytes()
    K.sync()
    kf.set_poses(store.poses(), 0, K.stream())                   # the module's store as it was
    K.sync()
    vis.close()


def _state(kf):
    """every byte the store holds on the device: both kinds' records and begins, every pose"""
    v, i = kf.view(K.stream()), kf.info()
    K.sync()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    blobs = []
    for ptr, nbytes in [(v["points"][q], 16 * i["n_points"][q]) for q in (0, 1)] + [(v["begin"][q], 8 * (i["n_keyframes"] + 1)) for q in (0, 1)] + \
            [(v["poses"], 96 * i["n_keyframes"])]:
        out = np.zeros(int(nbytes), np.uint8)
        assert nbytes == 0 or hip.hipMemcpy(out.ctypes.data, int(ptr), out.nbytes, 2) == 0
        blobs.append(out.tobytes())
    return blobs


def test_refusals_leave_everything_as_it_was(fx, scene):
    from lidar_feature_extraction_amd import binding as B
    store, kf, _ = scene
    L, ctx = fx._L, fx._ctx
    # create: what lfx_visibility_tables refuses, and capacities out of order
    for bad in (dict(n_rows=0), dict(n_rows=129), dict(n_columns=2), dict(n_columns=181), dict(n_columns=4098), dict(elev_step=0.0),
                dict(elev_min=-1.6), dict(elev_min=1.0, elev_step=0.04), dict(min_range=0.0), dict(min_range=5.0, max_range=5.0),
                dict(radius=-1.0), dict(radius=float("inf")), dict(margin_abs=-0.1), dict(margin_rel=float("nan")), dict(guard=3),
                dict(min_through=0), dict(reserved=1)):
        with pytest.raises(B.LfxError) as err:
            fx.visibility(8, 8, **dict(VC.SCENE, **bad))
        assert err.value.code == B.ERR_INVALID_ARGUMENT, bad
    for window, resident in ((0, 0), (4, 0), (4, 5), (B.VISIBILITY_MAX_WINDOW + 1, 1)):
        with pytest.raises(B.LfxError) as err:
            fx.visibility(window, resident, **VC.SCENE)
        assert err.value.code == B.ERR_INVALID_ARGUMENT
    vis = fx.visibility(4, 4, **VC.SCENE)
    before = _state(kf)
    n, flags, votes = _fills(store)
    pf = (C.c_void_p * 2)(flags[0].data_ptr(), flags[1].data_ptr())
    pv = (C.c_void_p * 2)(votes[0].data_ptr(), votes[1].data_ptr())
    half = (C.c_void_p * 2)(flags[0].data_ptr(), None)
    r = B.VisibilityResult()
    st = C.c_void_p(K.stream())
    calls = [(None, vis.handle, kf.handle, 0, 2, pv, pf, C.byref(r)), (ctx, None, kf.handle, 0, 2, pv, pf, C.byref(r)),
             (ctx, vis.handle, None, 0, 2, pv, pf, C.byref(r)), (ctx, vis.handle, kf.handle, 0, 2, None, pf, C.byref(r)),
             (ctx, vis.handle, kf.handle, 0, 2, pv, None, C.byref(r)), (ctx, vis.handle, kf.handle, 0, 2, pv, half, C.byref(r)),
             (ctx, vis.handle, kf.handle, 0, 2, pv, pf, None),
             (ctx, vis.handle, kf.handle, len(store) + 1, 0, pv, pf, C.byref(r)), (ctx, vis.handle, kf.handle, 3, len(store) - 2, pv, pf, C.byref(r)),
             (ctx, vis.handle, kf.handle, 0, 5, pv, pf, C.byref(r))]                   # count > max_window
    for args in calls:
        assert L.lfx_visibility_run(*args, st) == B.ERR_INVALID_ARGUMENT, args[3:5]
    # the masked build's refusals
    n_out = C.c_uint64(0)
    for args in ((ctx, kf.handle, 2, 0, 1, pf[0], None, 0, None, C.byref(n_out)), (ctx, kf.handle, 0, len(store), 1, pf[0], None, 0, None, C.byref(n_out)),
                 (ctx, kf.handle, 0, 0, 1, None, None, 0, None, C.byref(n_out)), (ctx, kf.handle, 0, 0, 1, pf[0], None, 0, None, None)):
        assert L.lfx_keyframes_build_masked(*args, st) == B.ERR_INVALID_ARGUMENT
    K.sync()
    assert _state(kf) == before
    for k in range(2):
        assert (flags[k].cpu().numpy() == FLAG_FILL).all() and (votes[k].cpu().numpy().view(np.uint32) == VOTE_FILL).all()
    # count 0: LFX_OK, the result zero, nothing written
    _, _, res = vis.run(kf, 2, 0, votes=votes, flags=flags, stream=K.stream())
    K.sync()
    assert res == vis.result(B.VisibilityResult()) and (flags[0].cpu().numpy() == FLAG_FILL).all()
    vis.close()
    # only empty keyframes
    empty = KR.Store(3, (1, 1))
    none = [np.zeros((0, 4), np.float32)] * 3
    assert empty.add(none, none, [KR.pose([0, 0, 0], [k, 0, 0]) for k in range(3)]) == 0
    ekf = fx.keyframes(3, 1)
    for k in range(3):
        ekf.add_host(none[0], none[0], empty.pose[k], K.stream())
    vis = fx.visibility(4, 4, **VC.SCENE)
    _, _, res = vis.run(ekf, 0, 3, votes=votes, flags=flags, stream=K.stream())
    assert res == vis.result(B.VisibilityResult())
    got, begins = ekf.build_masked("edge", flags[0], 0, 3, begins=True)
    K.sync()
    assert len(got) == 0 and begins.cpu().numpy().tolist() == [0, 0, 0, 0]
    vis.close()
    ekf.close()
