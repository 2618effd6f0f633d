"""lfx_odometry_update_batch_deskewed: scans-only odometry that corrects every scan by its own constant-velocity
prediction.  It must equal the composition a caller can write by hand, bit for bit: per scan the motion between the last two
poses (lfx_motion_between, lfx_motion_scale), lfx_deskew_batch out of place, lfx_odometry_update on that scan's slices.  The
plain update_batch beside it keeps its behaviour (tests/odometry_restatement.py)."""
import numpy as np
import pytest

from tests import deskew_cases as K
from tests import deskew_restatement as R
from tests.odometry_restatement import RecentScans, optimize_scan, downsample

pytestmark = pytest.mark.gpu

RINGS, COLS, N = 32, 1024, 12
MOTION = R.pose([0.002, -0.003, 0.02], [0.3, 0.02, -0.005])       # per sweep: 3 m/s, 11 deg/s of yaw


def _sequence():
    from lidar_feature_extraction_amd import make_sweep
    legs = K.arc(R.pose([0.0, 0.0, 0.2], [-1.0, -1.5, 1.8]), MOTION, N)
    return [make_sweep(RINGS, COLS, seed=9900 + i, pose0=p, motion=MOTION)[0] for i, (p, _) in enumerate(legs)], legs


def _same(a, b):
    return a["pose"].tobytes() == b["pose"].tobytes() and (a["code"], a["iteration"], a["aligned"], a["n_edge_map"], a["n_surface_map"]) == (
        b["code"], b["iteration"], b["aligned"], b["n_edge_map"], b["n_surface_map"]) and (
        a["error"] == b["error"] or (np.isnan(a["error"]) and np.isnan(b["error"])))


def _store(odo):
    v = odo.view()
    return v, K.d2h(v["edge_points"], v["n_edge"]), K.d2h(v["surface_points"], v["n_surface"])


@pytest.mark.parametrize("ratio", [1.0, 0.9])
@pytest.mark.parametrize("to", ["end", "start"])
def test_update_batch_deskewed_equals_the_manual_composition(ratio, to):
    from lidar_feature_extraction_amd import motion_between, motion_scale
    clouds, legs = _sequence()
    fx = K.fx_for(RINGS, COLS, N)
    d, got = K.extract(fx, clouds)
    total = sum(len(c) for c in clouds)
    begin = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    one, manual, plain = fx.odometry(), fx.odometry(), fx.odometry()
    res = one.update_batch_deskewed(None, None, ratio, to, N, K.stream())
    # by hand
    buffers = K.out_buffers(total)
    poses, by_hand = [], []
    for s in range(N):
        D = R.IDENTITY if len(poses) < 2 else motion_between(poses[-2], poses[-1])
        sweeps = [R.IDENTITY] * N
        sweeps[s] = motion_scale(D, ratio)
        fx.deskew(None, sweeps, to, (buffers[0].data_ptr(), buffers[1].data_ptr()), K.stream())
        r = manual.update(buffers[0].data_ptr() + 16 * int(begin[s]), len(got[s].edge_points),
                          buffers[1].data_ptr() + 16 * int(begin[s]), len(got[s].surface_points), K.stream())
        K.sync()
        by_hand.append(r)
        poses.append(r["pose"])
    for s in range(N):
        assert _same(res[s], by_hand[s]), (s, res[s], by_hand[s])
    va, ea, sa = _store(one)
    vb, eb, sb = _store(manual)
    assert ea.tobytes() == eb.tobytes() and sa.tobytes() == sb.tobytes() and len(ea) and len(sa)
    for name in ("n_scans", "n_window_scans", "n_added", "dropped_scans", "n_edge", "n_surface", "n_edge_window", "n_surface_window"):
        assert va[name] == vb[name], name
    assert va["edge_offsets"].tolist() == vb["edge_offsets"].tolist() and va["pose"].tobytes() == vb["pose"].tobytes()
    assert sum(r["aligned"] for r in res) == N - 1
    # the first two scans are de-skewed by the identity: their stored clouds are the raw ones at their poses
    es = RecentScans()
    es.add(res[0]["pose"], got[0].edge_points)
    es.add(res[1]["pose"], got[1].edge_points)
    assert ea[:va["edge_offsets"][2]].tobytes() == es.get_all().tobytes()
    # the batch's own clouds stay raw, and a plain odometry on the same batch is the one tests/test_odometry_gpu.py checks
    for s in range(N):
        a = fx.download(s, K.stream())
        assert a.edge_points.tobytes() == got[s].edge_points.tobytes() and a.surface_points.tobytes() == got[s].surface_points.tobytes()
    pres = plain.update_batch(N, K.stream())
    vp, ep, sp = _store(plain)
    es, ss = RecentScans(), RecentScans()
    for s in range(N):
        es.add(pres[s]["pose"], got[s].edge_points)
        ss.add(pres[s]["pose"], got[s].surface_points)
    assert ep.tobytes() == es.get_all().tobytes() and sp.tobytes() == ss.get_all().tobytes()
    for k in range(1, N):
        lo = max(0, k - 7)
        ew, sw = np.concatenate(es.scans[lo:k]), np.concatenate(ss.scans[lo:k])
        g = pres[k]
        w = optimize_scan(ew, sw, 15, got[k].edge_points, downsample(got[k].surface_points, 1.0), pres[k - 1]["pose"], 20)
        if (g["code"], g["iteration"]) != (w["code"], w["iteration"]):
            assert abs(g["iteration"] - w["iteration"]) <= 1 and np.abs(g["pose"] - w["pose"]).max() < 2e-3, (k, g, w)
        else:
            assert np.abs(g["pose"] - w["pose"]).max() <= 1e-6 * (1 + np.abs(w["pose"]).max()), (k, g["pose"], w["pose"])
    # ... and it feeds the two-pose memory: a de-skewed update after plain ones predicts from their poses
    d3, got3 = K.extract(fx, clouds[:1])
    r = plain.update_batch_deskewed(None, None, ratio, to, 1, K.stream())[0]
    sweeps = [motion_scale(motion_between(pres[-2]["pose"], pres[-1]["pose"]), ratio)]
    b1 = K.out_buffers(len(clouds[0]))
    fx.deskew(None, sweeps, to, (b1[0].data_ptr(), b1[1].data_ptr()), K.stream())
    assert r["aligned"] and np.isfinite(r["pose"]).all()
    v2, e2, s2 = _store(plain)
    want_e = RecentScans()
    want_e.add(r["pose"], K.slices(b1, clouds[:1], got3)[0][0])
    assert e2[v2["edge_offsets"][-2]:].tobytes() == want_e.get_all().tobytes()
    for o in (one, manual, plain):
        o.close()
    fx.close()
