"""The general record loader on the device: every layout of tests/layout_cases.py filled from the same canonical clouds,
on the host path and the device path, against the oracle on those clouds; ring ids the reference's uint16 cannot hold;
and both de-skews reading their times from a field that is aligned to nothing."""
import numpy as np
import pytest

from tests import deskew_cases as K
from tests import deskew_restatement as DR
from tests import layout_cases as LC
from tests import trajectory_cases as TC
from tests import trajectory_restatement as T
from tests import wire_cases as W
from tests.parity import assert_filtered_equal, assert_scan_equal

pytestmark = pytest.mark.gpu

from lidar_feature_extraction_amd import FeatureExtraction, make_scan, make_sweep  # noqa: E402
from lidar_feature_extraction_amd import binding as B  # noqa: E402

R, C = 16, 500
ERR_RING_ID = -5
_SCANS = {}


class _Scan:
    """A canonical cloud, the oracle on it (with `zero`: on the cloud without its (0, 0, 0) records) and its payloads."""

    def __init__(self, cloud, zero=None):
        self.cloud, self.zero = cloud, zero
        self.keep = None if zero is None else np.nonzero(~zero)[0]
        kept = cloud if zero is None else np.ascontiguousarray(cloud[self.keep])
        self.want = W.oracle_of(kept)
        self.piece = W.scan_piece(kept, self.want)


def _scans(order):
    """Three scans in driver order or shuffled; the middle one carries ~3 % of (0, 0, 0) records."""
    if order not in _SCANS:
        shuffle = order == "shuffled"
        clouds = [make_scan(R, C, seed=5200 + i, shuffle=shuffle) for i in range(3)]
        zero = np.random.default_rng(52).uniform(0, 1, len(clouds[1])) < 0.03
        for f in ("x", "y", "z"):
            clouds[1][f][zero] = 0.0
        _SCANS[order] = [_Scan(clouds[0]), _Scan(clouds[1], zero), _Scan(clouds[2])]
        assert all(len(s.piece.edge) > 50 and len(s.piece.surface) > 50 for s in _SCANS[order])
    return _SCANS[order]


def _fx(lay, batch=3, **kw):
    return FeatureExtraction(device=0, max_points_per_scan=R * C, max_batch=batch, max_points_per_ring=C, max_rings=R,
                             layout=lay.library_layout(), **kw)


@pytest.mark.parametrize("lay", LC.LAYOUTS, ids=LC.layout_id)
def test_layout_on_the_host_path_and_the_device_path(lay):
    """ExtractFeatures and a device batch of three (the zero filter on, one scan with (0, 0, 0) records) equal the oracle on
    the canonical cloud; download(), pack_xyz and pack_colored of that batch equal the restatement -- colored_scan takes its
    z from the record through the layout's offset and byte order.  Then a scan whose ring ids are 5 r + 2: the host looks
    them up in the records (its own read of the ring field, every type and byte order) and runs the batch again."""
    what = LC.layout_id(lay)
    f = _fx(lay, drop_zero_points=True)
    for order in ("driver", "shuffled"):
        scans = _scans(order)
        for k in (0, 2):
            assert_scan_equal(f.ExtractFeatures(lay.fill(scans[k].cloud)), scans[k].want, "%s %s host scan %d" % (what, order, k))
        d = W.upload([lay.fill(s.cloud) for s in scans])
        f.extract_batch_device(d.data_ptr(), np.array([len(s.cloud) for s in scans], np.uint32), W.stream())
        assert f.scan_routes(3, W.stream()).tolist() == [0, 0, 0], "a layout the general loader reads is bucketed"
        f.batch_status(W.stream())
        for k, s in enumerate(scans):
            got = f.download(k, W.stream())
            if s.zero is None:
                assert_scan_equal(got, s.want, "%s %s device scan %d" % (what, order, k))
            else:
                assert_filtered_equal(got, s.want, s.keep, s.zero, "%s %s device scan %d" % (what, order, k))
        exp = W.batch_expect([s.piece for s in scans])
        W.check_call(f, exp, "pack_xyz", what="%s %s" % (what, order))
        W.check_call(f, exp, "pack_colored", what="%s %s" % (what, order))
    base = _scans("driver")[0].cloud
    strange = base.copy()
    strange["ring"] = 5 * base["ring"] + 2
    got = f.ExtractFeatures(lay.fill(base, 5 * base["ring"].astype(np.int64) + 2))
    want = W.oracle_of(strange)
    assert want["ring_id"].tolist() == [5 * r + 2 for r in range(R)]
    assert_scan_equal(got, want, what + " ring ids 5 r + 2")
    f.close()


@pytest.mark.parametrize("ring_type,bad,be", [(B.INT8, -1, False), (B.INT16, -1, False), (B.INT16, -1, True), (B.INT32, -1, False),
                                              (B.INT32, -1, True), (B.UINT32, 70000, False), (B.UINT32, 70000, True)],
                         ids=lambda v: LC.RING_NAME.get(v, str(v)) if not isinstance(v, bool) else ("be" if v else "le"))
def test_ring_ids_the_reference_cannot_hold(ring_type, bad, be):
    """One record with a ring id of -1 in a signed field, or 70 000 in a UINT32 one: LFX_ERR_RING_ID -- from ExtractFeatures
    with the host's "above 65535" (its sign extension and byte swap find the same id the device refused), from the device
    path through batch_status.  The next batch on that context equals the oracle.  (The payloads of a batch that reported
    an error are unspecified and not looked at.)"""
    lay = LC.RecordLayout("xyzir32", 32, 0, 4, 8, 20, ring_type, be)
    good, other = _scans("driver")[0], _scans("shuffled")[2]
    ids = good.cloud["ring"].astype(np.int64)
    ids[4321] = bad
    f = _fx(lay, batch=2)
    with pytest.raises(B.LfxError) as e:
        f.ExtractFeatures(lay.fill(good.cloud, ids))
    assert e.value.code == ERR_RING_ID and "above 65535" in str(e.value), e.value
    d = W.upload([lay.fill(other.cloud), lay.fill(good.cloud, ids)])
    f.extract_batch_device(d.data_ptr(), np.array([len(other.cloud), len(good.cloud)], np.uint32), W.stream())
    with pytest.raises(B.LfxError) as e:
        f.batch_status(W.stream())
    assert e.value.code == ERR_RING_ID, e.value
    d = W.upload([lay.fill(good.cloud), lay.fill(other.cloud)])
    f.extract_batch_device(d.data_ptr(), np.array([len(good.cloud), len(other.cloud)], np.uint32), W.stream())
    f.batch_status(W.stream())
    assert_scan_equal(f.download(0, W.stream()), good.want, "device path after the error")
    assert_scan_equal(f.download(1, W.stream()), other.want, "device path after the error, second scan")
    assert_scan_equal(f.ExtractFeatures(lay.fill(good.cloud)), good.want, "host path after the error")
    f.close()


@pytest.mark.parametrize("ring_type,be", [(B.INT8, False), (B.INT16, False), (B.INT16, True)],
                         ids=lambda v: LC.RING_NAME.get(v, str(v)) if not isinstance(v, bool) else ("be" if v else "le"))
def test_a_negative_ring_id_is_not_the_unsigned_id_of_its_bits(ring_type, be):
    """A context that was told the sensor's ids (lfx_config.ring_ids), 255 and 65535 among them: a record whose signed ring
    field holds -1 carries those bits, and is still refused -- load_ring extends the sign, so that the id is above every
    uint16, before the table of ids is asked.  Without the table such an id is past max_rings either way and the sign
    extension cannot be seen."""
    lay = LC.RecordLayout("xyzir32", 32, 0, 4, 8, 20, ring_type, be)
    base = _scans("driver")[0].cloud
    sub = np.ascontiguousarray(base[base["ring"] < 14])
    relabelled = sub.copy()
    relabelled["ring"][sub["ring"] == 13] = 100
    want = W.oracle_of(relabelled)
    assert want["ring_id"].tolist() == list(range(13)) + [100]
    ids = relabelled["ring"].astype(np.int64)
    bad = ids.copy()
    bad[4321] = -1
    f = _fx(lay, batch=2, ring_ids=list(range(13)) + [100, 255, 65535])
    n = np.array([len(sub), len(sub)], np.uint32)
    d = W.upload([lay.fill(sub, ids), lay.fill(sub, ids)])
    f.extract_batch_device(d.data_ptr(), n, W.stream())
    f.batch_status(W.stream())
    assert_scan_equal(f.download(1, W.stream()), want, "the ids the context was told")
    d = W.upload([lay.fill(sub, ids), lay.fill(sub, bad)])
    f.extract_batch_device(d.data_ptr(), n, W.stream())
    with pytest.raises(B.LfxError) as e:
        f.batch_status(W.stream())
    assert e.value.code == ERR_RING_ID, e.value
    with pytest.raises(B.LfxError) as e:
        f.ExtractFeatures(lay.fill(sub, bad))
    assert e.value.code == ERR_RING_ID, e.value
    assert_scan_equal(f.ExtractFeatures(lay.fill(sub, ids)), want, "host path after the error")
    f.close()


# ------------------------------------------------------------------------------------------ an unaligned time field
_SWEEPS = None


def _sweeps(rings, cols, n):
    """n sweeps of a moving sensor with seeded motions |w| <= 0.2, |v| <= 3 (made once)."""
    global _SWEEPS
    if _SWEEPS is None:
        rng = np.random.default_rng(5300)
        motions, clouds = [], []
        for s in range(n):
            u, v = rng.normal(size=3), rng.normal(size=3)
            D = DR.pose(u / np.linalg.norm(u) * rng.uniform(0, 0.2), v / np.linalg.norm(v) * rng.uniform(0, 3.0))
            motions.append(D)
            clouds.append(make_sweep(rings, cols, seed=5300 + s, motion=D)[0])
        _SWEEPS = (clouds, motions)
    return _SWEEPS


def _stored_times(time_type, alpha):
    """Times at the fractions alpha of a sweep as a field of that type stores them: (stored values, scale, t0, t1)."""
    if time_type == B.FLOAT32:
        t0, t1 = 10.0, 10.1
        return (t0 + alpha * (t1 - t0)).astype(np.float32), 1.0, t0, t1
    if time_type == B.FLOAT64:
        t0 = 1.7e9 + 0.25
        return t0 + alpha * 0.1, 1.0, t0, t0 + 0.1
    t0, t1 = 0.5, 0.6
    return np.round((t0 + alpha * (t1 - t0)) * 1e9).astype(np.uint32), 1e-9, t0, t1


@pytest.mark.parametrize("be", [False, True], ids=["le", "be"])
def test_deskew_from_an_unaligned_time_field(be):
    """29-byte records x1 y5 z9 ring13 t15: record_time's 4-byte loads (FLOAT32, UINT32) and its 8-byte load (FLOAT64) from
    addresses aligned to nothing, at a step that is no multiple of anything, in both byte orders; lfx_deskew_batch to both
    frames and one lfx_deskew_batch_trajectory call, 16 x 900 x 4, times drawn per record.  The criterion is the de-skew
    tests': per coordinate |gpu - ref| <= spacing_f32(ref) + 1e-12, at most 1e-4 of a case's coordinates different from the
    restatement at all; the share of every case is printed."""
    import torch
    rings, cols, n = 16, 900, 4
    clouds, motions = _sweeps(rings, cols, n)
    rng = np.random.default_rng(53 + int(be))
    geometry = LC.timed29(B.FLOAT32, be)
    fx = FeatureExtraction(device=0, max_points_per_scan=rings * cols, max_batch=n, max_points_per_ring=cols, max_rings=rings,
                           layout=geometry.library_layout())
    total = sum(len(c) for c in clouds)
    begin = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    d = W.upload([geometry.fill(c) for c in clouds])
    records = d[:total * 29].view(-1, 29)
    fx.extract_batch_device(d.data_ptr(), np.array([len(c) for c in clouds], np.uint32), K.stream())
    assert fx.scan_routes(n, K.stream()).tolist() == [0] * n
    fx.batch_status(K.stream())
    got = [fx.download(s, K.stream()) for s in range(n)]
    for s, g in enumerate(got):                        # the features are the records the indices name
        xyz = np.stack([clouds[s]["x"], clouds[s]["y"], clouds[s]["z"]], axis=1)
        assert len(g.edge_index) > 100 and len(g.surface_index) > 100
        assert np.array_equal(g.edge_points[:, :3], xyz[g.edge_index]) and np.array_equal(g.surface_points[:, :3], xyz[g.surface_index])
    buffers = K.out_buffers(total)
    out = (buffers[0].data_ptr(), buffers[1].data_ptr())
    for time_type in (B.FLOAT32, B.UINT32, B.FLOAT64):
        lay = LC.timed29(time_type, be)
        tf = lay.time_field()
        stored, scale, t0, t1 = _stored_times(time_type, rng.uniform(-0.02, 1.02, total))
        raw = lay.put_times(stored)
        records[:, 15:15 + raw.shape[1]] = torch.from_numpy(raw).to(K.dev())
        assert tf.scale == scale
        for to_end in (True, False):
            for b in buffers:
                b.fill_(float("nan"))
            fx.deskew(tf, [(t0, t1, D) for D in motions], "end" if to_end else "start", out, K.stream())
            differ, coords = 0, 0
            for s, (ge, gs) in enumerate(K.slices(buffers, clouds, got)):
                for gpu, pts, idx in ((ge, got[s].edge_points, got[s].edge_index), (gs, got[s].surface_points, got[s].surface_index)):
                    alpha = DR.alpha_from_time(stored[begin[s] + idx.astype(np.int64)], scale, t0, t1)
                    a, b2 = K.compare(gpu, DR.deskew(pts, alpha, motions[s], to_end), (LC.layout_id(lay), to_end, s))
                    differ, coords = differ + a, coords + b2
            share = differ / coords
            print("deskew share %s %s: %d of %d coordinates differ (%.3g)" % (LC.layout_id(lay), "end" if to_end else "start", differ, coords, share))
            assert share <= 1e-4, (LC.layout_id(lay), to_end, share)
    # the FLOAT64 field is still in the records: one trajectory call on them, 2, 3 (small angles), 21 and 64 knots
    knots = (2, 3, 21, 64)
    shapes = [TC.seeded(rng, k, small=k == 3, t0=t0, span=0.1) for k in knots]
    t = np.concatenate([rng.uniform(tm[0] - 0.002, tm[-1] + 0.002, len(c)) for (tm, _), c in zip(shapes, clouds)])
    records[:, 15:23] = torch.from_numpy(lay.put_times(t)).to(K.dev())
    trajectories = [(tm, p, tm[0] + 0.437 * (tm[-1] - tm[0])) for tm, p in shapes]
    for b in buffers:
        b.fill_(float("nan"))
    fx.deskew_trajectory(tf, trajectories, out, K.stream())
    differ, coords = 0, 0
    for s, (ge, gs) in enumerate(K.slices(buffers, clouds, got)):
        idx = np.concatenate([got[s].edge_index, got[s].surface_index]).astype(np.int64)
        pts = np.concatenate([got[s].edge_points, got[s].surface_points])
        times, poses, t_ref = trajectories[s]
        a, b2 = K.compare(np.concatenate([ge, gs]), T.deskew(pts, T.time_from_field(t[begin[s] + idx], 1.0), times, poses, t_ref), ("trajectory", be, s))
        differ, coords = differ + a, coords + b2
    share = differ / coords
    print("trajectory share %s: %d of %d coordinates differ (%.3g)" % (LC.layout_id(lay), differ, coords, share))
    assert share <= 1e-4, ("trajectory", be, share)
    fx.close()
