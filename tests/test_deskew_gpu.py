"""lfx_deskew_batch on the device (include/lfx.h, the de-skew section) against the numpy restatement
(tests/deskew_restatement.py): every time source on every route, both target frames; what it leaves alone; what it refuses;
and that a localiser fed de-skewed sweeps finds the pose a static scan gives."""
import ctypes as C

import numpy as np
import pytest

from tests import deskew_cases as K
from tests import deskew_restatement as R

pytestmark = pytest.mark.gpu

SOURCES = ["index", "f32", "f64", "u32", "f32be", "f64be", "u32be"]
ROUTES = ["organised", "shuffled", "dropped", "zeros"]


def _time_bytes(source, alpha):
    """The 8 bytes at offset 24 of every record for a time source, its lfx_time_field and (t0, t1), and the stored values."""
    from lidar_feature_extraction_amd import binding as B
    n = len(alpha)
    raw = np.zeros((n, 8), np.uint8)
    if source == "index":
        return raw, B.TimeField(B.TIME_FROM_INDEX, 0, 0, 0, 1.0), (0.0, 0.0), None
    be = source.endswith("be")
    kind = source[:3]
    if kind == "f32":
        t0, t1, scale, dt = 10.0, 10.1, 1.0, B.FLOAT32
        stored = (t0 + alpha * (t1 - t0)).astype(np.float32)
        raw[:, :4] = stored.astype(">f4" if be else "<f4").view(np.uint8).reshape(n, 4)
    elif kind == "f64":
        t0, scale, dt = 1.7e9 + 0.25, 1.0, B.FLOAT64
        t1 = t0 + 0.1
        stored = t0 + alpha * (t1 - t0)
        raw[:, :8] = stored.astype(">f8" if be else "<f8").view(np.uint8).reshape(n, 8)
    else:
        t0, t1, scale, dt = 0.5, 0.6, 1e-9, B.UINT32
        stored = np.round((t0 + alpha * (t1 - t0)) * 1e9).astype(np.uint32)
        raw[:, :4] = stored.astype(">u4" if be else "<u4").view(np.uint8).reshape(n, 4)
    return raw, B.TimeField(B.TIME_FROM_FIELD, 24, dt, int(be), scale), (t0, t1), (stored, scale)


def _routed(clouds, route, rng):
    out = []
    for c in clouds:
        c = c.copy()
        if route == "shuffled":
            c = c[rng.permutation(len(c))]
        elif route == "dropped":
            c = c[rng.uniform(0, 1, len(c)) >= 0.05]
        elif route == "zeros":
            z = rng.uniform(0, 1, len(c)) < 0.05
            c["x"][z], c["y"][z], c["z"][z] = 0.0, 0.0, 0.0
        out.append(np.ascontiguousarray(c))
    return out


_SWEEPS = {}


def _sweeps(rings, cols, n):
    """n sweeps with seeded motions |w| <= 0.2, |v| <= 3 (made once per shape)."""
    from lidar_feature_extraction_amd import make_sweep
    if (rings, cols, n) not in _SWEEPS:
        rng = np.random.default_rng(rings * 1000 + n)
        motions, clouds = [], []
        for s in range(n):
            u, v = rng.normal(size=3), rng.normal(size=3)
            D = R.pose(u / np.linalg.norm(u) * rng.uniform(0, 0.2), v / np.linalg.norm(v) * rng.uniform(0, 3.0))
            motions.append(D)
            clouds.append(make_sweep(rings, cols, seed=9100 + s, motion=D)[0])
        _SWEEPS[(rings, cols, n)] = (clouds, motions)
    return _SWEEPS[(rings, cols, n)]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("rings,cols,n", [(16, 900, 8), (64, 1800, 64)], ids=["16x900x8", "64x1800x64"])
def test_kernel_against_the_restatement(rings, cols, n, route):
    """Every time source (the index; FLOAT32, FLOAT64 and UINT32 fields at byte 24, little- and big-endian; the fields hold
    times drawn per record, so a wrong gather shows) and both target frames, on each route, out of place, features from
    download() before the call.  Per coordinate |gpu - ref| <= spacing_f32(ref) + 1e-12, and at most 1e-4 of a case's
    coordinates may differ from the restatement at all.

    MEASURED SHARE (one MI355X, every one of the 112 cases: 2 shapes x 4 routes x 7 sources x 2 frames; about 34 k coordinates
    per 16 x 900 x 8 case, about 2.6 M per 64 x 1800 x 64 case): 0 -- no coordinate differs from the restatement, where the
    argument above expected about 1e-6 and the cap is 1e-4.  The test prints the share of every case."""
    import torch
    from lidar_feature_extraction_amd import binding as B
    rng = np.random.default_rng(5 + ROUTES.index(route))
    base, motions = _sweeps(rings, cols, n)
    clouds = _routed(base, route, rng)
    kw = dict(drop_zero_points=True, stream_hint=B.STREAM_GRID_WITH_HOLES) if route == "zeros" else {}
    fx = K.fx_for(rings, cols, n, **kw)
    d, got = K.extract(fx, clouds)
    fx.batch_status(K.stream())
    total = sum(len(c) for c in clouds)
    begin = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    assert sum(len(g.edge_points) + len(g.surface_points) for g in got) > 100 * n
    buffers = K.out_buffers(total)
    worst = 0.0
    for source in SOURCES:
        alpha_rec = rng.uniform(-0.02, 1.02, total)
        raw, tf, (t0, t1), stored = _time_bytes(source, alpha_rec)
        d.view(-1, 32)[:, 24:32] = torch.from_numpy(raw).to(K.dev())
        sweeps = [(t0, t1, D) for D in motions]
        for to_end in (True, False):
            for b in buffers:
                b.fill_(float("nan"))
            fx.deskew(tf, sweeps, "end" if to_end else "start", (buffers[0].data_ptr(), buffers[1].data_ptr()), K.stream())
            differ, coords = 0, 0
            for s, (ge, gs) in enumerate(K.slices(buffers, clouds, got)):
                for gpu, pts, idx in ((ge, got[s].edge_points, got[s].edge_index), (gs, got[s].surface_points, got[s].surface_index)):
                    if stored is None:
                        alpha = R.alpha_from_index(idx, len(clouds[s]))
                    else:
                        alpha = R.alpha_from_time(stored[0][begin[s] + idx.astype(np.int64)], stored[1], t0, t1)
                    a, b2 = K.compare(gpu, R.deskew(pts, alpha, motions[s], to_end), (route, source, to_end, s))
                    differ, coords = differ + a, coords + b2
            share = differ / coords
            worst = max(worst, share)
            print("deskew share %dx%dx%d %s %s %s: %d of %d coordinates differ (%.3g)" % (
                rings, cols, n, route, source, "end" if to_end else "start", differ, coords, share))
            assert share <= 1e-4, (route, source, to_end, share)
    # the context's own clouds were never touched
    for s in range(n):
        again = fx.download(s, K.stream())
        assert again.edge_points.tobytes() == got[s].edge_points.tobytes() and again.surface_points.tobytes() == got[s].surface_points.tobytes()
    print("deskew worst share %dx%dx%d %s: %.3g" % (rings, cols, n, route, worst))
    fx.close()


def test_identity_motion_and_a_nan_time():
    """The identity motion gives back the input values; a NaN time leaves exactly that record unchanged; 4th floats equal."""
    import torch
    from lidar_feature_extraction_amd import binding as B, make_sweep
    rings, cols, n = 16, 900, 3
    rng = np.random.default_rng(12)
    clouds = [make_sweep(rings, cols, seed=9300 + s)[0] for s in range(n)]
    fx = K.fx_for(rings, cols, n)
    d, got = K.extract(fx, clouds)
    total = sum(len(c) for c in clouds)
    begin = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    buffers = K.out_buffers(total)
    for to in ("end", "start"):
        for source in ("index", "f32"):
            raw, tf, (t0, t1), _ = _time_bytes(source, rng.uniform(0, 1, total))
            d.view(-1, 32)[:, 24:32] = torch.from_numpy(raw).to(K.dev())
            fx.deskew(tf, [(t0, t1, R.IDENTITY)] * n, to, (buffers[0].data_ptr(), buffers[1].data_ptr()), K.stream())
            for s, (ge, gs) in enumerate(K.slices(buffers, clouds, got)):
                assert np.array_equal(ge, got[s].edge_points) and np.array_equal(gs, got[s].surface_points), (to, source, s)
    # one edge record and one surface record of scan 1 carry a NaN time
    D = R.pose([0.02, -0.01, 0.15], [2.0, -0.5, 0.1])
    alpha_rec = rng.uniform(0, 1, total)
    stored = (10.0 + alpha_rec * 0.1).astype(np.float32)
    hit_e, hit_s = len(got[1].edge_index) // 2, len(got[1].surface_index) // 3
    stored[begin[1] + int(got[1].edge_index[hit_e])] = np.nan
    stored[begin[1] + int(got[1].surface_index[hit_s])] = np.nan
    raw = np.zeros((total, 8), np.uint8)
    raw[:, :4] = stored.view(np.uint8).reshape(total, 4)
    d.view(-1, 32)[:, 24:32] = torch.from_numpy(raw).to(K.dev())
    tf = B.TimeField(B.TIME_FROM_FIELD, 24, B.FLOAT32, 0, 1.0)
    for to_end in (True, False):
        fx.deskew(tf, [(10.0, 10.1, D)] * n, "end" if to_end else "start", (buffers[0].data_ptr(), buffers[1].data_ptr()), K.stream())
        for s, (ge, gs) in enumerate(K.slices(buffers, clouds, got)):
            for gpu, pts, idx, hit in ((ge, got[s].edge_points, got[s].edge_index, hit_e), (gs, got[s].surface_points, got[s].surface_index, hit_s)):
                alpha = R.alpha_from_time(stored[begin[s] + idx.astype(np.int64)], 1.0, 10.0, 10.1)
                K.compare(gpu, R.deskew(pts, alpha, D, to_end), (to_end, s))
                same = (gpu == pts).all(axis=1)
                if s == 1:
                    assert gpu[hit].tobytes() == pts[hit].tobytes()
                    assert same.sum() == 1 and same[hit], (to_end, s, int(same.sum()))
                else:
                    assert not same.any()
    fx.close()


def _packed(fx, n, total, which):
    """pack_xyz / pack_features payloads of the last batch: (edge, surface, offsets) on the host."""
    import torch
    e, s = K.out_buffers(total)
    off = torch.zeros(2 * (n + 1), dtype=torch.int32, device=K.dev())
    getattr(fx, which)(e.data_ptr(), s.data_ptr(), off.data_ptr(), total, K.stream())
    K.sync()
    return e.cpu().numpy(), s.cpu().numpy(), off.cpu().numpy()


def test_in_place_out_of_place_and_refusals():
    """Out of place first, then in place on the same batch: the context's clouds equal the out-of-place buffers byte for
    byte through download(), pack_xyz and pack_features; indices, counts and every per-point output are as before.  Every
    refusal returns LFX_ERR_INVALID_ARGUMENT and leaves the clouds untouched, a second de-skew of the batch among them; a
    fresh extraction lifts the guard."""
    from lidar_feature_extraction_amd import binding as B, make_sweep
    from lidar_feature_extraction_amd.extraction import _sweeps as make_sweeps
    L = B.load()
    rings, cols, n = 16, 900, 4
    rng = np.random.default_rng(14)
    motions = [R.pose(rng.normal(0, 0.05, 3), rng.normal(0, 1.0, 3)) for _ in range(n)]
    clouds = [make_sweep(rings, cols, seed=9400 + s, motion=motions[s])[0] for s in range(n)]
    fx = K.fx_for(rings, cols, n)
    index = B.TimeField(B.TIME_FROM_INDEX, 0, 0, 0, 1.0)
    field = B.TimeField(B.TIME_FROM_FIELD, 24, B.FLOAT32, 0, 1.0)
    sweeps = [(0.0, 0.1, D) for D in motions]
    with pytest.raises(B.LfxError) as e:        # no batch yet
        fx.deskew(index, sweeps)
    assert e.value.code == B.ERR_INVALID_ARGUMENT
    d, got = K.extract(fx, clouds)
    total = sum(len(c) for c in clouds)
    buffers = K.out_buffers(total)
    out = (buffers[0].data_ptr(), buffers[1].data_ptr())
    before_xyz, before_feat = _packed(fx, n, total, "pack_xyz"), _packed(fx, n, total, "pack_features")

    def untouched():
        for s in range(n):
            a = fx.download(s, K.stream())
            assert a.edge_points.tobytes() == got[s].edge_points.tobytes() and a.surface_points.tobytes() == got[s].surface_points.tobytes()

    def refused(time, sw, to="end", o=out, count=None):
        with pytest.raises(B.LfxError) as err:
            if count is None:
                fx.deskew(time, sw, to, o, K.stream())
            else:
                arr, _ = make_sweeps(sw)
                B.check(fx._ctx, L.lfx_deskew_batch(fx._ctx, C.byref(time), arr, count, 1, o[0], o[1], None), L)
        assert err.value.code == B.ERR_INVALID_ARGUMENT, err.value
        untouched()

    bad = lambda i, v: [(0.0, 0.1, np.where(np.arange(12).reshape(3, 4) == i, v, motions[s])) if s == 2 else sweeps[s] for s in range(n)]   # noqa: E731
    refused(index, sweeps[:-1], count=n - 1)                                              # n_scans not the last batch's
    refused(index, sweeps + sweeps[:1], count=n + 1)
    sw_arr = (B.Sweep * n)()
    assert L.lfx_deskew_batch(fx._ctx, None, sw_arr, n, 1, out[0], out[1], None) == B.ERR_INVALID_ARGUMENT      # NULL time
    assert L.lfx_deskew_batch(fx._ctx, C.byref(index), None, n, 1, out[0], out[1], None) == B.ERR_INVALID_ARGUMENT   # NULL sweeps
    assert L.lfx_deskew_batch(None, C.byref(index), sw_arr, n, 1, out[0], out[1], None) == B.ERR_INVALID_ARGUMENT
    untouched()
    refused(B.TimeField(2, 24, B.FLOAT32, 0, 1.0), sweeps)                                # unknown source
    refused(B.TimeField(B.TIME_FROM_FIELD, 24, B.INT32, 0, 1.0), sweeps)                  # unknown datatype
    refused(B.TimeField(B.TIME_FROM_FIELD, 24, B.UINT16, 0, 1.0), sweeps)
    refused(index, sweeps, to=2)                                                          # unknown target
    refused(index, sweeps, to=-1)
    refused(B.TimeField(B.TIME_FROM_FIELD, 29, B.FLOAT32, 0, 1.0), sweeps)                # a field past point_step
    refused(B.TimeField(B.TIME_FROM_FIELD, 25, B.FLOAT64, 0, 1.0), sweeps)
    refused(B.TimeField(B.TIME_FROM_FIELD, 0xFFFFFFFC, B.UINT32, 0, 1e-9), sweeps)
    refused(index, bad(5, np.nan))                                                        # non-finite motion
    refused(field, bad(3, np.inf))
    refused(field, [(np.nan, 0.1, D) for D in motions])                                   # non-finite times
    refused(field, [(0.0, np.inf, D) for D in motions])
    refused(field, [(0.25, 0.25, D) for D in motions])                                    # t1 == t0 with a field
    refused(index, sweeps, o=(out[0], 0))                                                 # exactly one output NULL
    refused(index, sweeps, o=(0, out[1]))
    view = fx.device_view()                                                               # the context's own clouds as outputs
    refused(index, sweeps, o=(view.edge_points, view.surface_points))
    refused(index, sweeps, o=(out[0], view.surface_points))
    # (t1 == t0 is nothing to the index source; out of place may be repeated)
    fx.deskew(index, [(0.25, 0.25, D) for D in motions], "end", out, K.stream())
    fx.deskew(index, sweeps, "end", out, K.stream())
    want = K.slices(buffers, clouds, got)
    for s in range(n):
        K.compare(want[s][0], R.deskew(got[s].edge_points, R.alpha_from_index(got[s].edge_index, len(clouds[s])), motions[s], True), s)
    untouched()
    fx.deskew(index, sweeps, "end", None, K.stream())                                     # in place
    after = [fx.download(s, K.stream()) for s in range(n)]
    for s in range(n):
        assert after[s].edge_points.tobytes() == want[s][0].tobytes() and after[s].surface_points.tobytes() == want[s][1].tobytes()
        assert not np.array_equal(after[s].edge_points, got[s].edge_points)
        for name in ("labels", "curvature", "sorted_index", "ring_id", "ring_count", "ring_offset", "ring_status", "edge_index", "surface_index"):
            assert getattr(after[s], name).tobytes() == getattr(got[s], name).tobytes(), (s, name)
    for which, before in (("pack_xyz", before_xyz), ("pack_features", before_feat)):
        e, sf, off = _packed(fx, n, total, which)
        assert np.array_equal(off, before[2])
        for s in range(n):
            we, ws = want[s][0].copy(), want[s][1].copy()
            if which == "pack_xyz":
                we[:, 3], ws[:, 3] = 1.0, 1.0
            assert e[off[s]:off[s + 1]].tobytes() == we.tobytes(), (which, s)
            assert sf[off[n + 1 + s]:off[n + 2 + s]].tobytes() == ws.tobytes(), (which, s)
    # a second de-skew of that batch, either way, is refused and changes nothing
    for o in (None, out):
        with pytest.raises(B.LfxError) as e:
            fx.deskew(index, sweeps, "end", o, K.stream())
        assert e.value.code == B.ERR_INVALID_ARGUMENT and "already" in str(e.value)
        for s in range(n):
            assert fx.download(s, K.stream()).edge_points.tobytes() == want[s][0].tobytes()
    # a fresh extraction lifts the guard
    d2, got2 = K.extract(fx, clouds)
    for s in range(n):
        assert got2[s].edge_points.tobytes() == got[s].edge_points.tobytes()
    fx.deskew(index, sweeps, "start", None, K.stream())
    for s in range(n):
        a = fx.download(s, K.stream())
        K.compare(a.surface_points, R.deskew(got[s].surface_points, R.alpha_from_index(got[s].surface_index, len(clouds[s])), motions[s], False), s)
    fx.close()


def _transformed(pose, records):
    """records [n, 4] float32 carried by a pose (double, rounded once)."""
    out = np.asarray(records, np.float32).copy()
    out[:, :3] = R.apply(pose, out[:, :3].astype(np.float64)).astype(np.float32)
    return out


def test_deskewing_helps_a_localiser():
    """8 sweeps of 32 x 1024 along an arc at 15 m/s, 35 deg/s of yaw and a little roll and pitch, localised with
    lfx_localize_batch from the true end pose perturbed by (0.2 m, 1 deg) against maps of static scans of the same room
    carried to the world by their true poses.  Control: the same localiser on static scans taken at the sweeps' end poses.
    Per sweep the de-skewed (true motions, in place, to the end) translation error is at most twice the largest control
    error of the eight, and the raw sweep's error is larger than the de-skewed one on every sweep.

    MEASURED (one MI355X; translation error in metres, control / de-skewed / raw, sweeps 0 .. 7; also in DESIGN.md section 7):
    0.0274 / 0.0206 / 0.4692, 0.0280 / 0.0351 / 0.5488, 0.0234 / 0.0271 / 0.6403, 0.0126 / 0.0101 / 0.5616,
    0.0119 / 0.0111 / 0.5087, 0.0118 / 0.0113 / 0.4790, 0.0316 / 0.0214 / 0.6382, 0.0274 / 0.0143 / 0.5340: the largest
    control error is 0.0316 m (bound 0.0632 m), the largest de-skewed one 0.0351 m."""
    import torch
    from lidar_feature_extraction_amd import make_sweep
    rings, cols, n, k, max_iter = 32, 1024, 8, 15, 20
    D = R.pose([0.01, -0.02, 0.06], [1.5, 0.1, -0.05])
    legs = K.arc(R.pose([0.0, 0.0, 0.2], [-7.0, -1.5, 1.8]), D, n)       # (stays 0.8 m clear of every pillar)
    ends = [q for _, q in legs]
    rng = np.random.default_rng(21)
    fx = K.fx_for(rings, cols, n)
    # the maps: static scans at poses between and beside the sweeps' end poses
    map_poses = [R.compose(p, R.pose([0, 0, 0.3 * (i % 3 - 1)], [0.7, 0.4 * (i % 2), 0.0])) for i, (p, _) in enumerate(legs)]
    d, got = K.extract(fx, [make_sweep(rings, cols, seed=9600 + i, pose0=p)[0] for i, p in enumerate(map_poses)])
    edge_map = np.ascontiguousarray(np.concatenate([_transformed(p, g.edge_points) for p, g in zip(map_poses, got)]))
    surf_map = np.ascontiguousarray(np.concatenate([_transformed(p, g.surface_points) for p, g in zip(map_poses, got)]))
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
    d2, _ = K.extract(fx, [make_sweep(rings, cols, seed=9800 + i, pose0=p, motion=D)[0] for i, (p, _) in enumerate(legs)])
    raw = errors(fx.localize_batch(emap, smap, start, k, max_iter, 1.0, K.stream()))
    fx.deskew(None, [D] * n, "end", None, K.stream())
    fixed = errors(fx.localize_batch(emap, smap, start, k, max_iter, 1.0, K.stream()))
    for i in range(n):
        print("deskew localise sweep %d: control %.4f m, de-skewed %.4f m, raw %.4f m" % (i, control[i], fixed[i], raw[i]))
    assert control.max() < 0.1, control          # (the control converges on every pose)
    assert (fixed <= 2.0 * control.max()).all(), (fixed, control)
    assert (raw > fixed).all(), (raw, fixed)
    fx.close()
