"""lfx_pack_features_segmented on the device (include/lfx.h, the segmentation section) against the numpy statement of the
filter over the view's arrays (tests/segment_restatement.py filtered_pack): offsets, counts and the records below the
capacity byte for byte -- every mask, capacities around a scan boundary and at the totals, nothing written at or past a
short capacity -- and the filtered clouds through the rolling map with the table as begins and counts."""
import ctypes as C

import numpy as np
import pytest

from tests import deskew_cases as K
from tests import segment_restatement as R

pytestmark = pytest.mark.gpu

RINGS, COLS, BATCH = 16, 900, 3
ALL = 15


@pytest.fixture(scope="module")
def batch():
    """Three scans extracted and segmented once: the context, the classes on the device and on the host, the view's arrays."""
    from lidar_feature_extraction_amd import concat, make_scan
    clouds = [make_scan(RINGS, COLS, seed=700 + s, sensor_pose=(1.5 * s - 3.0, 0.4 * s, 0.3 * s)) for s in range(BATCH)]
    fx = K.fx_for(RINGS, COLS, BATCH)
    d = K.upload_bytes(concat(clouds))
    fx.extract_batch_device(d.data_ptr(), [len(c) for c in clouds], K.stream())
    fx.batch_status(K.stream())
    cfg = R.config(n_rows=RINGS, n_columns=COLS)
    classes, _, _ = fx.segment(cfg, stream=K.stream())
    K.sync()
    host = classes.cpu().numpy()
    assert host.tobytes() == R.segment_batch(cfg, clouds)[0].tobytes()
    begin = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    yield dict(fx=fx, classes=classes, host=host, begin=begin, d=d, clouds=clouds)
    fx.close()


def _features(batch):
    """Per scan (edge records [ne][4], edge_index, surface records, surface_index) as the context's clouds hold them."""
    fx, begin = batch["fx"], batch["begin"]
    v = fx.device_view()
    info = K.d2h(v.scan_info, BATCH, 4).view(np.uint32)
    out = []
    for s in range(BATCH):
        ne, ns = int(info[s][2]), int(info[s][3])
        ep = K.d2h(int(v.edge_points) + 16 * int(begin[s]), ne)
        sp = K.d2h(int(v.surface_points) + 16 * int(begin[s]), ns)
        ei = K.d2h(int(v.edge_index) + 4 * int(begin[s]), ne, 1).view(np.uint32).reshape(-1)
        si = K.d2h(int(v.surface_index) + 4 * int(begin[s]), ns, 1).view(np.uint32).reshape(-1)
        out.append((ep, ei, sp, si))
    return out


def _pack(batch, edge_mask, surface_mask, capacity):
    """(edge buffer, surface buffer -- one record longer than the capacity, filled with a mark --, offsets, counts)"""
    import torch
    from lidar_feature_extraction_amd import binding as B
    fx = batch["fx"]
    mark = 1234.5
    edge = torch.full((capacity + 1, 4), mark, dtype=torch.float32, device=K.dev())
    surface = torch.full((capacity + 1, 4), mark, dtype=torch.float32, device=K.dev())
    offsets = torch.full((2, BATCH + 1), -1, dtype=torch.int32, device=K.dev())
    counts = torch.full((2, BATCH), -1, dtype=torch.int32, device=K.dev())
    B.check(fx._ctx, B.load().lfx_pack_features_segmented(
        fx._ctx, C.c_void_p(batch["classes"].data_ptr()), edge_mask, surface_mask, C.c_void_p(edge.data_ptr()), C.c_void_p(surface.data_ptr()),
        C.c_void_p(offsets.data_ptr()), C.c_void_p(counts.data_ptr()), capacity, C.c_void_p(K.stream())))
    K.sync()
    return edge.cpu().numpy(), surface.cpu().numpy(), offsets.cpu().numpy().view(np.uint32), counts.cpu().numpy().view(np.uint32), mark


def _check(batch, features, edge_mask, surface_mask, capacity):
    we, ws, woff, wcnt = R.filtered_pack(batch["host"], batch["begin"], features, edge_mask, surface_mask)
    e, s, off, cnt, mark = _pack(batch, edge_mask, surface_mask, capacity)
    what = (edge_mask, surface_mask, capacity)
    assert off.tobytes() == woff.tobytes() and cnt.tobytes() == wcnt.tobytes(), (what, off, woff, cnt, wcnt)
    for got, want in ((e, we), (s, ws)):
        n = min(len(want), capacity)
        assert got[:n].tobytes() == want[:n].tobytes(), what
        assert (got[n:] == np.float32(mark)).all(), what               # nothing at or past the capacity, nothing past the total
    return we, ws, woff, wcnt


def test_masks(batch):
    """The default masks, all-pass (lfx_pack_features byte for byte), none, every single class, different masks per cloud."""
    import torch
    from lidar_feature_extraction_amd import binding as B
    features = _features(batch)
    total = int(batch["begin"][-1])
    we, ws, woff, wcnt = _check(batch, features, B.SEG_EDGE_MASK_DEFAULT, B.SEG_SURFACE_MASK_DEFAULT, total)
    all_e, all_s = sum(len(f[1]) for f in features), sum(len(f[3]) for f in features)
    # (the filter bites, and leaves something: edges on clusters only, surfaces on the ground and on clusters)
    assert 0 < len(we) < all_e and 0 < len(ws) < all_s, (len(we), all_e, len(ws), all_s)
    pe, ps, poff, pcnt = _check(batch, features, ALL, ALL, total)
    assert len(pe) == all_e and len(ps) == all_s
    edge = torch.zeros((total, 4), dtype=torch.float32, device=K.dev())
    surface = torch.zeros((total, 4), dtype=torch.float32, device=K.dev())
    offsets = torch.zeros((2, BATCH + 1), dtype=torch.int32, device=K.dev())
    batch["fx"].pack_features(edge.data_ptr(), surface.data_ptr(), offsets.data_ptr(), total, K.stream())
    K.sync()
    assert offsets.cpu().numpy().view(np.uint32).tobytes() == poff.tobytes()
    assert edge.cpu().numpy()[:all_e].tobytes() == pe.tobytes() and surface.cpu().numpy()[:all_s].tobytes() == ps.tobytes()
    ne, ns, noff, ncnt = _check(batch, features, 0, 0, total)
    assert len(ne) == 0 and len(ns) == 0 and not noff.any()
    kept = 0
    for cls in range(4):
        e, _, _, _ = _check(batch, features, 1 << cls, 1 << (3 - cls), total)
        kept += len(e)
    assert kept == all_e                                               # every feature has exactly one class
    # the Python layer: the same tables and records, with and without the counts
    e, s, off, cnt = batch["fx"].pack_features_segmented(batch["classes"], counts=True, stream=K.stream())
    K.sync()
    assert off.cpu().numpy().view(np.uint32).tobytes() == woff.tobytes() and cnt.cpu().numpy().view(np.uint32).tobytes() == wcnt.tobytes()
    assert e.cpu().numpy()[:len(we)].tobytes() == we.tobytes() and s.cpu().numpy()[:len(ws)].tobytes() == ws.tobytes()
    e2, s2, off2 = batch["fx"].pack_features_segmented(batch["classes"], stream=K.stream())
    K.sync()
    assert off2.cpu().numpy().tobytes() == off.cpu().numpy().tobytes() and e2.cpu().numpy()[:len(we)].tobytes() == we.tobytes()


def test_capacities(batch):
    """Around a scan boundary of either cloud, at the totals, one under and one over, and 0: the table is complete, the records
    below the capacity are there and nothing else is written."""
    from lidar_feature_extraction_amd import binding as B
    features = _features(batch)
    _, _, woff, _ = R.filtered_pack(batch["host"], batch["begin"], features, B.SEG_EDGE_MASK_DEFAULT, B.SEG_SURFACE_MASK_DEFAULT)
    caps = {0, 1}
    for k in (0, 1):
        for b in (int(woff[k][1]), int(woff[k][2]), int(woff[k][BATCH])):
            caps |= {max(b - 1, 0), b, b + 1}
    for cap in sorted(caps):
        _check(batch, features, B.SEG_EDGE_MASK_DEFAULT, B.SEG_SURFACE_MASK_DEFAULT, cap)


def test_refusals(batch):
    import torch
    from lidar_feature_extraction_amd import binding as B
    L, fx = B.load(), batch["fx"]
    buf = torch.full((64, 4), 7.0, dtype=torch.float32, device=K.dev())
    tab = torch.full((2, BATCH + 1), 7, dtype=torch.int32, device=K.dev())
    p, t, c = C.c_void_p(buf.data_ptr()), C.c_void_p(tab.data_ptr()), C.c_void_p(batch["classes"].data_ptr())
    null, st = C.c_void_p(0), C.c_void_p(K.stream())
    for args in ((null, 4, 6, p, p, t), (c, 4, 6, null, p, t), (c, 4, 6, p, null, t), (c, 4, 6, p, p, null), (c, 16, 6, p, p, t), (c, 4, 0x80000000, p, p, t)):
        assert L.lfx_pack_features_segmented(fx._ctx, *args, null, 64, st) == B.ERR_INVALID_ARGUMENT, args
    assert L.lfx_pack_features_segmented(null, c, 4, 6, p, p, t, null, 64, st) == B.ERR_INVALID_ARGUMENT
    fresh = K.fx_for(RINGS, COLS, 1)
    assert L.lfx_pack_features_segmented(fresh._ctx, c, 4, 6, p, p, t, null, 64, st) == B.ERR_INVALID_ARGUMENT      # no batch yet
    fresh.close()
    K.sync()
    assert (buf.cpu().numpy() == 7.0).all() and (tab.cpu().numpy() == 7).all()


def test_through_the_rolling_map(batch):
    """The filtered clouds inserted through lfx_rolling_map_insert with the offsets table as d_begin and the counts as d_count
    (stride 1): the map equals the rolling-map restatement fed with the same records."""
    from lidar_feature_extraction_amd import binding as B
    from lidar_feature_extraction_amd.extraction import RollingMap
    from tests.rolling_map_restatement import Store
    fx = batch["fx"]
    features = _features(batch)
    we, ws, woff, wcnt = R.filtered_pack(batch["host"], batch["begin"], features, B.SEG_EDGE_MASK_DEFAULT, B.SEG_SURFACE_MASK_DEFAULT)
    e, s, off, cnt = fx.pack_features_segmented(batch["classes"], counts=True, stream=K.stream())
    dims = (64, 64, 16)
    rm = RollingMap(fx, edge_leaf=0.5, surface_leaf=0.5, edge_dims=dims, surface_dims=dims)
    identity = np.eye(4)[:3]
    poses = [identity] * BATCH
    for k, (kind, buf, want) in enumerate((("edge", e, we), ("surface", s, ws))):
        rm.insert(kind, buf.data_ptr(), off.data_ptr() + 4 * k * (BATCH + 1), cnt.data_ptr() + 4 * k * BATCH, 1, BATCH, max(len(want), 1),
                  np.stack(poses), K.stream())
        K.sync()
        ref = Store(0.5, dims)
        ref.insert([want[int(woff[k][i]):int(woff[k][i + 1])] for i in range(BATCH)], poses)
        lo, hi = ref.window()
        got = rm.extract(kind, lo, hi, K.stream())
        assert got.shape == ref.extract_all().shape and got.tobytes() == ref.extract_all().tobytes(), kind
        assert len(got) > 100, (kind, len(got))
    del rm
