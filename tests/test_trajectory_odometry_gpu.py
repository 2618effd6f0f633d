"""lfx_odometry_update_batch_trajectory: scans-only odometry that corrects every scan along the caller's trajectory of it.
It must equal the composition a caller can write by hand, bit for bit in poses, results and store: lfx_deskew_batch_trajectory
out of place, then lfx_odometry_update on each scan's slices (as tests/test_deskew_odometry_gpu.py does it for the predicting
call).  A batch with a refused trajectory anywhere in it is refused whole: no scan of it is aligned or added."""
import numpy as np
import pytest

from tests import deskew_cases as K
from tests import deskew_restatement as R
from tests import trajectory_cases as TC

pytestmark = pytest.mark.gpu

RINGS, COLS, N = 16, 900, 6


def _sequence():
    from lidar_feature_extraction_amd import make_sweep_trajectory
    legs, p = [], R.pose([0.0, 0.0, 0.2], [-1.0, -1.5, 1.8])
    for i in range(N):
        times, poses = TC.turning(p, knots=(21, 2, 64, 5, 11, 33)[i], speed=3.0, yaw_deg=11.0)
        legs.append((times, poses, times[-1]))
        p = poses[-1]
    return [make_sweep_trajectory(RINGS, COLS, seed=9900 + i, times=t, poses=q)[0] for i, (t, q, _) in enumerate(legs)], legs


def test_update_batch_trajectory_equals_the_manual_composition():
    clouds, legs = _sequence()
    fx = K.fx_for(RINGS, COLS, N)
    d, got = K.extract(fx, clouds)
    total = sum(len(c) for c in clouds)
    begin = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    one, manual = fx.odometry(), fx.odometry()
    res = one.update_batch_trajectory(None, legs, N, K.stream())
    buffers = K.out_buffers(total)
    fx.deskew_trajectory(None, legs, (buffers[0].data_ptr(), buffers[1].data_ptr()), K.stream())
    by_hand = []
    for s in range(N):
        by_hand.append(manual.update(buffers[0].data_ptr() + 16 * int(begin[s]), len(got[s].edge_points),
                                     buffers[1].data_ptr() + 16 * int(begin[s]), len(got[s].surface_points), K.stream()))
        K.sync()
    for s in range(N):
        assert TC.same_result(res[s], by_hand[s]), (s, res[s], by_hand[s])
    va, ea, sa = TC.store(one)
    vb, eb, sb = TC.store(manual)
    assert ea.tobytes() == eb.tobytes() and sa.tobytes() == sb.tobytes() and len(ea) and len(sa)
    for name in ("n_scans", "n_window_scans", "n_added", "dropped_scans", "n_edge", "n_surface", "n_edge_window", "n_surface_window"):
        assert va[name] == vb[name], name
    assert va["edge_offsets"].tolist() == vb["edge_offsets"].tolist() and va["pose"].tobytes() == vb["pose"].tobytes()
    assert sum(r["aligned"] for r in res) == N - 1
    # the de-skewed clouds are not the raw ones, and the batch's own clouds stay raw
    want = K.slices(buffers, clouds, got)
    assert not np.array_equal(want[2][0], got[2].edge_points)
    for s in range(N):
        a = fx.download(s, K.stream())
        assert a.edge_points.tobytes() == got[s].edge_points.tobytes() and a.surface_points.tobytes() == got[s].surface_points.tobytes()
    one.close()
    manual.close()
    fx.close()


def test_a_bad_trajectory_late_in_the_batch_refuses_the_whole_batch():
    """The last scan's trajectory is bad (a time out of order, a NaN pose entry, 65 knots, NULL poses): the call is refused
    before scan 0 is touched -- the store, the pose and the scan count are what they were -- and the same odometry then takes
    the good batch exactly as a fresh one does."""
    import ctypes as C
    from lidar_feature_extraction_amd import binding as B
    from lidar_feature_extraction_amd.extraction import _time_field, _trajectories
    clouds, legs = _sequence()
    fx = K.fx_for(RINGS, COLS, N)
    K.extract(fx, clouds)
    odo, fresh = fx.odometry(), fx.odometry()
    before = TC.store(odo)
    tf = _time_field(None)

    def refused(arr):
        res = (B.OdometryResult * N)()
        rc = odo._L.lfx_odometry_update_batch_trajectory(fx._ctx, odo.handle, C.byref(tf), arr, N, res, C.c_void_p(K.stream()))
        assert rc == B.ERR_INVALID_ARGUMENT, rc
        K.sync()
        after = TC.store(odo)
        for name in ("n_scans", "n_window_scans", "n_added", "dropped_scans", "n_edge", "n_surface"):
            assert after[0][name] == before[0][name] == 0, name
        assert after[0]["pose"].tobytes() == before[0]["pose"].tobytes()

    times, poses, t_ref = legs[-1]
    out_of_order, nan_pose = times.copy(), poses.copy()
    out_of_order[3] = out_of_order[2]
    nan_pose[7, 1, 3] = np.nan
    for last in ((out_of_order, poses, t_ref), (times, nan_pose, t_ref), (times, poses, np.inf)):
        arr, _, _keep = _trajectories(legs[:-1] + [last])
        refused(arr)
    arr, _, _keep = _trajectories(legs)
    arr[N - 1].n_knots = 65
    refused(arr)
    arr, _, _keep = _trajectories(legs)
    arr[N - 1].poses = None
    refused(arr)
    got, want = odo.update_batch_trajectory(None, legs, N, K.stream()), fresh.update_batch_trajectory(None, legs, N, K.stream())
    for s in range(N):
        assert TC.same_result(got[s], want[s]), s
    assert TC.store(odo)[1].tobytes() == TC.store(fresh)[1].tobytes()
    odo.close()
    fresh.close()
    fx.close()
