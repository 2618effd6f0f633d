"""lfx_deskew_batch_trajectory on the device (include/lfx.h, the de-skew section) against the numpy restatement
(tests/trajectory_restatement.py): every time source, knot counts from 2 to 64 within one batch, times on knots and outside
them; the two-knot case against lfx_deskew_batch; what it leaves alone and what it refuses; many calls on two streams; and
that a localiser fed sweeps de-skewed along their trajectories finds the pose a static scan gives."""
import ctypes as C

import numpy as np
import pytest

from tests import deskew_cases as K
from tests import deskew_restatement as R
from tests import trajectory_cases as TC
from tests import trajectory_restatement as T

pytestmark = pytest.mark.gpu

SOURCES = ["index", "f32", "f64", "u32", "f32be", "f64be", "u32be"]
SPAN = {"index": (0.0, 1.0), "f32": (10.0, 0.1), "f64": (1.7e9 + 0.25, 0.1), "u32": (0.5, 0.1)}


def _field(source):
    from lidar_feature_extraction_amd import binding as B
    if source == "index":
        return B.TimeField(B.TIME_FROM_INDEX, 0, 0, 0, 1.0)
    dt, scale = {"f32": (B.FLOAT32, 1.0), "f64": (B.FLOAT64, 1.0), "u32": (B.UINT32, 1e-9)}[source[:3]]
    return B.TimeField(B.TIME_FROM_FIELD, 24, dt, int(source.endswith("be")), scale)


def _time_bytes(source, t):
    """The 8 bytes at offset 24 of every record holding the times t [n] (seconds) for a field source, and the values as
    stored with their scale."""
    n = len(t)
    raw = np.zeros((n, 8), np.uint8)
    be, kind = source.endswith("be"), source[:3]
    if kind == "f32":
        stored, scale = t.astype(np.float32), 1.0
        raw[:, :4] = stored.astype(">f4" if be else "<f4").view(np.uint8).reshape(n, 4)
    elif kind == "f64":
        stored, scale = t.astype(np.float64), 1.0
        raw[:, :8] = stored.astype(">f8" if be else "<f8").view(np.uint8).reshape(n, 8)
    else:
        stored, scale = np.round(t * 1e9).astype(np.uint32), 1e-9
        raw[:, :4] = stored.astype(">u4" if be else "<u4").view(np.uint8).reshape(n, 4)
    return raw, stored, scale


_CLOUDS = {}


def _clouds(rings, cols, n):
    from lidar_feature_extraction_amd import make_sweep
    if (rings, cols, n) not in _CLOUDS:
        _CLOUDS[(rings, cols, n)] = [make_sweep(rings, cols, seed=9100 + s)[0] for s in range(n)]
    return _CLOUDS[(rings, cols, n)]


def _check(gpu, got, clouds, begin, stored, scale, trajectories, what):
    """Every scan's two clouds of `gpu` (K.slices) against the restatement; (coordinates that differ at all, coordinates)."""
    differ, coords = 0, 0
    for s, (ge, gs) in enumerate(gpu):
        idx = np.concatenate([got[s].edge_index, got[s].surface_index]).astype(np.int64)
        pts = np.concatenate([got[s].edge_points, got[s].surface_points])
        t = T.time_from_index(idx, len(clouds[s])) if stored is None else T.time_from_field(stored[begin[s] + idx], scale)
        times, poses, t_ref = trajectories[s]
        a, b = K.compare(np.concatenate([ge, gs]), T.deskew(pts, t, times, poses, t_ref), what + (s,))
        differ, coords = differ + a, coords + b
    return differ, coords


@pytest.mark.parametrize("route", ["organised", "shuffled"])
@pytest.mark.parametrize("rings,cols,n,knots", [(16, 900, 4, (2, 3, 21, 64)), (64, 1800, 2, (21, 21)), (16, 900, 32, (21, 2, 64, 5))],
                         ids=["16x900x4", "64x1800x2", "16x900x32"])
def test_kernel_against_the_restatement(rings, cols, n, knots, route):
    """Every time source (the index; FLOAT32, FLOAT64 and UINT32 fields at byte 24, little- and big-endian), t_ref at the
    first knot, at the last and inside, organised and shuffled scans, out of place, features from download() before the
    call.  16 x 900 x 4 spreads 2, 3, 21 and 64 knots over the scans of one batch (the 3-knot one turns by less than 1e-8
    rad per segment: the small-angle form); a 64 x 1800 scan has more records than one pass of the grid covers; 32 scans
    take the other launch shape.  The fields hold times drawn per record from 2 % before the first knot to 2 % after the
    last; with the FLOAT64 field 200 records per scan sit on knot times exactly.  Per coordinate
    |gpu - ref| <= spacing_f32(ref) + 1e-12, and at most 1e-4 of a case's coordinates may differ from the restatement at all.

    MEASURED SHARE (one MI355X, every one of the 126 cases: 3 shapes x 2 routes x 7 sources x 3 t_ref; 18 483 coordinates
    per 16 x 900 x 4 case, 81 303 per 64 x 1800 x 2 case, 148 068 per 16 x 900 x 32 case): 0 -- no coordinate differs from the
    restatement, the worst share is 0 against the cap of 1e-4 (also in DESIGN.md section 7).  The test prints the share of
    every case."""
    import torch
    rng = np.random.default_rng(31 + n)
    clouds = [c.copy() for c in _clouds(rings, cols, n)]
    if route == "shuffled":
        clouds = [np.ascontiguousarray(c[rng.permutation(len(c))]) for c in clouds]
    fx = K.fx_for(rings, cols, n)
    d, got = K.extract(fx, clouds)
    fx.batch_status(K.stream())
    total = sum(len(c) for c in clouds)
    begin = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    assert sum(len(g.edge_points) + len(g.surface_points) for g in got) > 100 * n
    if rings == 64:
        assert min(len(g.edge_points) + len(g.surface_points) for g in got) > 32 * 256      # (the stride loop runs)
    buffers = K.out_buffers(total)
    worst = 0.0
    for source in SOURCES:
        t0, span = SPAN[source[:3] if source != "index" else "index"]
        shapes = [TC.seeded(rng, knots[s % len(knots)], small=knots[s % len(knots)] == 3, t0=t0, span=span) for s in range(n)]
        stored, scale = None, 1.0
        if source != "index":
            t = np.concatenate([rng.uniform(tm[0] - 0.02 * span, tm[-1] + 0.02 * span, len(c)) for (tm, _), c in zip(shapes, clouds)])
            if source == "f64":
                for s, (tm, _) in enumerate(shapes):
                    hit = begin[s] + rng.choice(len(clouds[s]), 200, replace=False)
                    t[hit] = tm[rng.integers(0, len(tm), 200)]
            raw, stored, scale = _time_bytes(source, t)
            d.view(-1, 32)[:, 24:32] = torch.from_numpy(raw).to(K.dev())
        for where in ("start", "end", "inside"):
            trajectories = [(tm, p, {"start": tm[0], "end": tm[-1], "inside": tm[0] + 0.437 * (tm[-1] - tm[0])}[where]) for tm, p in shapes]
            for b in buffers:
                b.fill_(float("nan"))
            fx.deskew_trajectory(_field(source), trajectories, (buffers[0].data_ptr(), buffers[1].data_ptr()), K.stream())
            differ, coords = _check(K.slices(buffers, clouds, got), got, clouds, begin, stored, scale, trajectories, (route, source, where))
            share = differ / coords
            worst = max(worst, share)
            print("trajectory share %dx%dx%d %s %s %s: %d of %d coordinates differ (%.3g)" % (
                rings, cols, n, route, source, where, differ, coords, share))
            assert share <= 1e-4, (route, source, where, share)
    for s in range(n):        # the context's own clouds were never touched
        again = fx.download(s, K.stream())
        assert again.edge_points.tobytes() == got[s].edge_points.tobytes() and again.surface_points.tobytes() == got[s].surface_points.tobytes()
    print("trajectory worst share %dx%dx%d %s: %.3g" % (rings, cols, n, route, worst))
    fx.close()


def test_two_knots_equal_the_constant_motion_call():
    """lfx_deskew_batch_trajectory with two knots and t_ref = times[0] gives the values of lfx_deskew_batch(TO_START) with
    the motion between the two poses on the same batch, compared as floats: index times and a FLOAT32 field, general and
    small-angle motions, general first poses."""
    import torch
    from lidar_feature_extraction_amd import motion_between
    rings, cols, n = 16, 900, 4
    rng = np.random.default_rng(41)
    clouds = _clouds(rings, cols, n)
    fx = K.fx_for(rings, cols, n)
    d, got = K.extract(fx, clouds)
    total = sum(len(c) for c in clouds)
    a, b = K.out_buffers(total), K.out_buffers(total)
    for source in ("index", "f32"):
        t0, span = SPAN[source]
        pairs = []
        for s in range(n):
            P0 = R.pose(TC.unit(rng) * rng.uniform(0.0, 3.0), rng.uniform(-50, 50, 3))
            w = TC.unit(rng) * (rng.uniform(0.0, 0.3) if s % 2 == 0 else 10.0 ** rng.uniform(-12, -8.5))
            pairs.append((P0, R.compose(P0, R.pose(w, TC.unit(rng) * rng.uniform(0.0, 3.0)))))
        if source != "index":
            raw, _, _ = _time_bytes(source, rng.uniform(t0 - 0.002, t0 + span + 0.002, total))
            d.view(-1, 32)[:, 24:32] = torch.from_numpy(raw).to(K.dev())
        fx.deskew_trajectory(_field(source), [([t0, t0 + span], [p, q], t0) for p, q in pairs], (a[0].data_ptr(), a[1].data_ptr()), K.stream())
        fx.deskew(_field(source), [(t0, t0 + span, motion_between(p, q)) for p, q in pairs], "start", (b[0].data_ptr(), b[1].data_ptr()), K.stream())
        for s, ((ae, asf), (be, bs)) in enumerate(zip(K.slices(a, clouds, got), K.slices(b, clouds, got))):
            assert np.array_equal(ae, be) and np.array_equal(asf, bs), (source, s)
            assert not np.array_equal(ae, got[s].edge_points)
    fx.close()


def test_what_it_leaves_alone_and_what_it_refuses():
    """A NaN time leaves exactly that record unchanged; identity knots give back the input values; an out-of-place call
    leaves the context's clouds alone; in place changes what download() and pack_xyz return; after an in-place call a second
    de-skew is refused from either entry point until the next extraction; every refusal of the header returns
    LFX_ERR_INVALID_ARGUMENT and queues nothing (the outputs keep their NaN fill)."""
    import torch
    from lidar_feature_extraction_amd import binding as B
    from lidar_feature_extraction_amd.extraction import _trajectories
    L = B.load()
    rings, cols, n = 16, 900, 3
    rng = np.random.default_rng(43)
    clouds = _clouds(rings, cols, n)
    fx = K.fx_for(rings, cols, n)
    index, field = _field("index"), _field("f32")
    good = [TC.seeded(rng, k) + (0.3,) for k in (2, 7, 64)]
    with pytest.raises(B.LfxError) as e:        # no batch yet
        fx.deskew_trajectory(index, good)
    assert e.value.code == B.ERR_INVALID_ARGUMENT
    d, got = K.extract(fx, clouds)
    total = sum(len(c) for c in clouds)
    begin = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    buffers = K.out_buffers(total)
    out = (buffers[0].data_ptr(), buffers[1].data_ptr())

    def untouched():
        for s in range(n):
            a = fx.download(s, K.stream())
            assert a.edge_points.tobytes() == got[s].edge_points.tobytes() and a.surface_points.tobytes() == got[s].surface_points.tobytes()

    # identity knots: the input values come back
    still = [(np.array([0.0, 0.4, 1.0]), np.tile(R.IDENTITY, (3, 1, 1)), 0.7)] * n
    fx.deskew_trajectory(index, still, out, K.stream())
    for s, (ge, gs) in enumerate(K.slices(buffers, clouds, got)):
        assert np.array_equal(ge, got[s].edge_points) and np.array_equal(gs, got[s].surface_points), s
    # one edge record and one surface record of scan 1 carry a NaN time
    t = rng.uniform(10.0, 10.1, total)
    stored = t.astype(np.float32)
    hit_e, hit_s = len(got[1].edge_index) // 2, len(got[1].surface_index) // 3
    stored[begin[1] + int(got[1].edge_index[hit_e])] = np.nan
    stored[begin[1] + int(got[1].surface_index[hit_s])] = np.nan
    raw = np.zeros((total, 8), np.uint8)
    raw[:, :4] = stored.view(np.uint8).reshape(total, 4)
    d.view(-1, 32)[:, 24:32] = torch.from_numpy(raw).to(K.dev())
    moving = [TC.seeded(rng, 9, t0=10.0, span=0.1) + (10.1,) for _ in range(n)]
    fx.deskew_trajectory(field, moving, out, K.stream())
    for s, (ge, gs) in enumerate(K.slices(buffers, clouds, got)):
        for gpu, pts, idx, hit in ((ge, got[s].edge_points, got[s].edge_index, hit_e), (gs, got[s].surface_points, got[s].surface_index, hit_s)):
            K.compare(gpu, T.deskew(pts, T.time_from_field(stored[begin[s] + idx.astype(np.int64)], 1.0), *moving[s]), s)
            same = (gpu == pts).all(axis=1)
            if s == 1:
                assert gpu[hit].tobytes() == pts[hit].tobytes() and same.sum() == 1 and same[hit]
            else:
                assert not same.any()
    untouched()

    def refused(time, trajectories, o=out, count=None):
        for b in buffers:
            b.fill_(float("nan"))
        arr, k, _keep = _trajectories(trajectories)
        rc = L.lfx_deskew_batch_trajectory(fx._ctx, C.byref(time), arr, k if count is None else count, o[0] or None, o[1] or None, K.stream())
        assert rc == B.ERR_INVALID_ARGUMENT, rc
        K.sync()
        assert torch.isnan(buffers[0]).all() and torch.isnan(buffers[1]).all()
        untouched()

    def bad(which, value, s=1):
        times, poses, t_ref = (np.array(x, np.float64) for x in good[s])
        if which == "time":
            times[1] = value
        elif which == "pose":
            poses[1, 2, 1] = value
        else:
            t_ref = value
        return [good[k] if k != s else (times, poses, float(t_ref)) for k in range(n)]

    refused(index, good[:-1], count=n - 1)                                                # n_scans not the last batch's
    refused(index, good + good[:1], count=n + 1)

    def refused_call(ctx, time, arr, stream):
        """the same for arguments the binding's conversion cannot form: the return code, nothing queued, the fill still there"""
        for b in buffers:
            b.fill_(float("nan"))
        assert L.lfx_deskew_batch_trajectory(ctx, time, arr, n, out[0], out[1], stream) == B.ERR_INVALID_ARGUMENT
        K.sync()
        assert torch.isnan(buffers[0]).all() and torch.isnan(buffers[1]).all()
        untouched()

    arr, _, _keep = _trajectories(good)
    refused_call(fx._ctx, None, arr, K.stream())                                          # NULL time
    refused_call(fx._ctx, C.byref(index), None, K.stream())                               # NULL trajectories
    refused_call(None, C.byref(index), arr, K.stream())                                   # NULL context
    refused(B.TimeField(2, 24, B.FLOAT32, 0, 1.0), good)                                  # what lfx_deskew_batch refuses about time
    refused(B.TimeField(B.TIME_FROM_FIELD, 24, B.INT32, 0, 1.0), good)
    refused(B.TimeField(B.TIME_FROM_FIELD, 29, B.FLOAT32, 0, 1.0), good)
    for value in (np.nan, np.inf, -np.inf):
        refused(index, bad("time", value))                                                # times not finite
        refused(index, bad("pose", value, 2))                                             # a pose entry not finite
        refused(field, bad("t_ref", value, 0))                                            # t_ref not finite
    refused(index, bad("time", good[1][0][0]))                                            # not strictly ascending
    refused(index, bad("time", good[1][0][2]))
    refused(index, bad("time", good[1][0][3]))
    for k in (0, 1, 65):                                                                  # n_knots outside 2 .. 64
        arr, _, _keep = _trajectories(good)
        arr[2].n_knots = k
        refused_call(fx._ctx, C.byref(index), arr, K.stream())
    for member in ("times", "poses"):                                                     # NULL times / poses
        arr, _, _keep = _trajectories(good)
        setattr(arr[0], member, None)
        refused_call(fx._ctx, C.byref(index), arr, K.stream())
    refused(index, good, o=(out[0], 0))                                                   # exactly one output NULL
    refused(index, good, o=(0, out[1]))
    view = fx.device_view()                                                               # the context's own clouds as outputs
    refused(index, good, o=(view.edge_points, view.surface_points))
    refused(index, good, o=(out[0], view.surface_points))
    # in place: download() and pack_xyz see what the out-of-place call wrote
    fx.deskew_trajectory(index, good, out, K.stream())
    want = K.slices(buffers, clouds, got)
    untouched()
    fx.deskew_trajectory(index, good, None, K.stream())
    e, sf = K.out_buffers(total)
    off = torch.zeros(2 * (n + 1), dtype=torch.int32, device=K.dev())
    fx.pack_xyz(e.data_ptr(), sf.data_ptr(), off.data_ptr(), total, K.stream())
    K.sync()
    e, sf, off = e.cpu().numpy(), sf.cpu().numpy(), off.cpu().numpy()
    for s in range(n):
        a = fx.download(s, K.stream())
        assert a.edge_points.tobytes() == want[s][0].tobytes() and a.surface_points.tobytes() == want[s][1].tobytes()
        assert not np.array_equal(a.edge_points, got[s].edge_points)
        we, ws = want[s][0].copy(), want[s][1].copy()
        we[:, 3], ws[:, 3] = 1.0, 1.0
        assert e[off[s]:off[s + 1]].tobytes() == we.tobytes() and sf[off[n + 1 + s]:off[n + 2 + s]].tobytes() == ws.tobytes()
    # a second de-skew of that batch is refused from either entry point, in place or not, and by both odometry calls
    odo = fx.odometry()
    for call in (lambda: fx.deskew_trajectory(index, good, None, K.stream()), lambda: fx.deskew_trajectory(index, good, out, K.stream()),
                 lambda: fx.deskew(index, [R.IDENTITY] * n, "end", None, K.stream()), lambda: fx.deskew(index, [R.IDENTITY] * n, "end", out, K.stream()),
                 lambda: odo.update_batch_trajectory(index, good, n, K.stream()), lambda: odo.update_batch_deskewed(index, None, 1.0, "end", n, K.stream())):
        with pytest.raises(B.LfxError) as err:
            call()
        assert err.value.code == B.ERR_INVALID_ARGUMENT and "already" in str(err.value)
    for s in range(n):
        assert fx.download(s, K.stream()).edge_points.tobytes() == want[s][0].tobytes()
    # ... and the constant-motion call in place bars the trajectory call as well; a fresh extraction lifts the guard
    d2, got2 = K.extract(fx, clouds)
    fx.deskew(index, [R.pose([0, 0, 0.01], [0.1, 0, 0])] * n, "end", None, K.stream())
    with pytest.raises(B.LfxError) as err:
        fx.deskew_trajectory(index, good, None, K.stream())
    assert err.value.code == B.ERR_INVALID_ARGUMENT and "already" in str(err.value)
    d3, got3 = K.extract(fx, clouds)
    fx.deskew_trajectory(index, good, None, K.stream())
    for s in range(n):
        assert fx.download(s, K.stream()).surface_points.tobytes() == want[s][1].tobytes()
    odo.close()
    fx.close()


def test_many_calls_on_two_streams():
    """20 calls alternating between two streams with growing knot counts (the table blocks are rotated more than twice and
    regrown), each into buffers of its own: every call's output equals the restatement."""
    import torch
    rings, cols, n = 16, 900, 2
    rng = np.random.default_rng(47)
    clouds = _clouds(rings, cols, n)
    fx = K.fx_for(rings, cols, n)
    d, got = K.extract(fx, clouds)
    K.sync()
    total = sum(len(c) for c in clouds)
    begin = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    calls = []
    for i in range(20):
        knots = min(64, 2 + 3 * i + (i // 2))
        trajectories = [TC.seeded(rng, max(2, knots - s)) + (rng.uniform(0.0, 1.0),) for s in range(n)]
        buffers = K.out_buffers(total)
        fx.deskew_trajectory(None, trajectories, (buffers[0].data_ptr(), buffers[1].data_ptr()), streams[i % 2].cuda_stream)
        calls.append((trajectories, buffers))
    K.sync()
    for i, (trajectories, buffers) in enumerate(calls):
        _check(K.slices(buffers, clouds, got), got, clouds, begin, None, 1.0, trajectories, ("call", i))
    fx.close()


def _transformed(pose, records):
    out = np.asarray(records, np.float32).copy()
    out[:, :3] = R.apply(pose, out[:, :3].astype(np.float64)).astype(np.float32)
    return out


def test_trajectory_deskewing_helps_a_localiser():
    """8 sweeps of 32 x 1024 of a sensor entering a turn (tests/trajectory_cases.py: 21 knots per sweep at 15 m/s, a yaw rate
    of 35 deg/s (1 + 2 sin(2 pi t / T)) with a little roll and pitch), each localised with lfx_localize_batch from its true
    end pose moved by (0.2 m, 1 deg) against maps of static scans, in three forms: a static control scan at the end pose, the
    sweep de-skewed along its trajectory (in place, t_ref the last knot), the sweep de-skewed by the constant motion between
    its first and last knot.  Per sweep the trajectory column stays within twice the largest control error (the rule and
    margin of tests/test_deskew_gpu.py); the constant-motion column is printed.

    MEASURED (one MI355X; translation error in metres, control / trajectory / constant motion, sweeps 0 .. 7; also in
    DESIGN.md section 7): 0.0356 / 0.0251 / 0.0553, 0.0251 / 0.0354 / 0.0620, 0.0163 / 0.0181 / 0.0572, 0.0092 / 0.0117 / 0.0617,
    0.0059 / 0.0024 / 0.0533, 0.0067 / 0.0137 / 0.0544, 0.0324 / 0.0139 / 0.0493, 0.0262 / 0.0169 / 0.0128: the largest control
    error is 0.0356 m (bound 0.0712 m), the largest trajectory one 0.0354 m, the largest constant-motion one 0.0620 m."""
    import torch
    from lidar_feature_extraction_amd import make_sweep, make_sweep_trajectory
    rings, cols, n, k, max_iter = 32, 1024, 8, 15, 20
    legs, p = [], R.pose([0.0, 0.0, 0.2], [-7.0, -1.5, 1.8])
    for _ in range(n):
        times, poses = TC.turning(p)
        legs.append((times, poses))
        p = poses[-1]
    ends = [poses[-1] for _, poses in legs]
    rng = np.random.default_rng(21)
    fx = K.fx_for(rings, cols, n)
    map_poses = [R.compose(poses[0], R.pose([0, 0, 0.3 * (i % 3 - 1)], [0.7, 0.4 * (i % 2), 0.0])) for i, (_, poses) in enumerate(legs)]
    d, got = K.extract(fx, [make_sweep(rings, cols, seed=9600 + i, pose0=q)[0] for i, q in enumerate(map_poses)])
    edge_map = np.ascontiguousarray(np.concatenate([_transformed(q, g.edge_points) for q, g in zip(map_poses, got)]))
    surf_map = np.ascontiguousarray(np.concatenate([_transformed(q, g.surface_points) for q, g in zip(map_poses, got)]))
    d_emap, d_smap = torch.from_numpy(edge_map).to(K.dev()), torch.from_numpy(surf_map).to(K.dev())
    emap, smap = fx.make_map(d_emap.data_ptr(), len(edge_map), 1.0, K.stream()), fx.make_map(d_smap.data_ptr(), len(surf_map), 2.0, K.stream())
    start = []
    for q in ends:
        u, v = rng.normal(size=3), rng.normal(size=3)
        start.append(R.compose(q, R.pose(u / np.linalg.norm(u) * np.deg2rad(1.0), v / np.linalg.norm(v) * 0.2)))
    start = np.stack(start)

    def errors(res):
        return np.array([np.linalg.norm(r["pose"][:, 3] - q[:, 3]) for r, q in zip(res, ends)])

    d1, _ = K.extract(fx, [make_sweep(rings, cols, seed=9700 + i, pose0=q)[0] for i, q in enumerate(ends)])
    control = errors(fx.localize_batch(emap, smap, start, k, max_iter, 1.0, K.stream()))
    sweeps = [make_sweep_trajectory(rings, cols, seed=9800 + i, times=times, poses=poses)[0] for i, (times, poses) in enumerate(legs)]
    d2, _ = K.extract(fx, sweeps)
    fx.deskew_trajectory(None, [(times, poses, times[-1]) for times, poses in legs], None, K.stream())
    along = errors(fx.localize_batch(emap, smap, start, k, max_iter, 1.0, K.stream()))
    d3, _ = K.extract(fx, sweeps)
    fx.deskew(None, [TC.constant_motion(poses) for _, poses in legs], "end", None, K.stream())
    flat = errors(fx.localize_batch(emap, smap, start, k, max_iter, 1.0, K.stream()))
    for i in range(n):
        print("trajectory localise sweep %d: control %.4f m, trajectory %.4f m, constant motion %.4f m" % (i, control[i], along[i], flat[i]))
    assert control.max() < 0.1, control          # (the control converges on every pose)
    assert (along <= 2.0 * control.max()).all(), (along, control)
    fx.close()
