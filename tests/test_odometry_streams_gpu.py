"""lfx_odometry_* across streams: the event behind an odometry's last queued call (the appended scan, its bounds on their way
to the pinned block) is what the next call waits for before it rebuilds the window maps or rewrites the staged cloud and the
pinned words -- whichever stream either call is on.  Each case feeds one odometry its calls on two streams and a fresh one
the same calls on one stream: the results and the store are equal byte for byte (the arithmetic is the same launches on the
same inputs, so nothing but a missing wait can tell them apart).  The hold is tests/segment_cases.py's, used as
tests/test_keyframes_gpu.py uses it."""
import numpy as np
import pytest

from tests import deskew_cases as K
from tests import segment_cases as S

pytestmark = pytest.mark.gpu

RINGS, COLS, N = 16, 900, 3                   # the smallest scans of tests/test_odometry_gpu.py; three fill a window of two and rebuild it
P0 = np.array([[1.0, 0.0, 0.0, 0.5], [0.0, 1.0, 0.0, -0.25], [0.0, 0.0, 1.0, 0.125]])


@pytest.fixture(scope="module")
def scans():
    """The context, the three scans' clouds on the host (the bits the device holds) and on the device, made once."""
    import torch
    from lidar_feature_extraction_amd import make_sequence
    clouds, _ = make_sequence(N, RINGS, COLS, seed=8400)
    fx = K.fx_for(RINGS, COLS, N)
    d, got = K.extract(fx, clouds)
    host = [(np.ascontiguousarray(g.edge_points, np.float32).reshape(-1, 4), np.ascontiguousarray(g.surface_points, np.float32).reshape(-1, 4))
            for g in got]
    dev = [(torch.from_numpy(e.copy()).to(K.dev()), torch.from_numpy(s.copy()).to(K.dev())) for e, s in host]
    K.sync()
    yield fx, host, dev
    fx.close()


def _state(odo, results):
    """What a run leaves: every result's pose bits, code, iterations and flags, the current pose, the store's offsets and
    records."""
    K.sync()
    v = odo.view()
    return ([(r["pose"].tobytes(), r["code"], r["iteration"], r["aligned"], r["n_edge_map"], r["n_surface_map"]) for r in results],
            odo.pose().tobytes(), v["edge_offsets"].tolist(), v["surface_offsets"].tolist(), (v["n_scans"], v["n_added"]),
            K.d2h(v["edge_points"], v["n_edge"]).tobytes(), K.d2h(v["surface_points"], v["n_surface"]).tobytes())


def _update(odo, dev, s, stream):
    e, sf = dev[s]
    return odo.update(e.data_ptr(), len(e), sf.data_ptr(), len(sf), stream)


def test_held_add_on_a_then_update_on_b(scans):
    """Stream A is held busy and lfx_odometry_add of scan 0 is queued behind the hold; an event behind the add says it has
    not run when lfx_odometry_update of scan 1 is issued on B.  The update rebuilds its window maps from the records and the
    bounds the add leaves, so it has to wait for A: scan 1's pose, then scan 2's (on A again, behind B's append), and the
    store equal those of the same three calls on one stream."""
    fx, host, dev = scans
    hold = S.Hold()
    a, b = S.two_streams()

    def run(st_add, st_update, st_last, held):
        odo = fx.odometry(n_local_scans=2)
        if held:
            hold(a)
        e, sf = dev[0]
        odo.add(P0, e.data_ptr(), len(e), sf.data_ptr(), len(sf), st_add)
        if held:
            hold.still_held(S.event_behind(a), "odometry: add on A, update on B")
        out = [_update(odo, dev, 1, st_update), _update(odo, dev, 2, st_last)]
        state = _state(odo, out)
        odo.close()
        return state

    for st in (a, b):                                                    # (both streams have run the busy kernel before the part that counts)
        hold._run(1, st)
    K.sync()
    want = run(K.stream(), K.stream(), K.stream(), False)
    got = run(a.cuda_stream, b.cuda_stream, a.cuda_stream, True)
    assert [r[3] for r in want[0]] == [True, True] and want[4] == (3, 3)
    assert got == want


def test_update_host_on_alternating_streams(scans):
    """lfx_odometry_update_host of the three scans on A, B, A: each call rewrites the staged cloud and the pinned words
    that the call before it, on the other stream, may still be reading.  Results and store equal those of the same calls on
    one stream."""
    fx, host, dev = scans
    a, b = S.two_streams()

    def run(streams):
        odo = fx.odometry(n_local_scans=2)
        out = [odo.update_host(host[s][0], host[s][1], streams[s]) for s in range(N)]
        state = _state(odo, out)
        odo.close()
        return state

    want = run([K.stream()] * N)
    got = run([a.cuda_stream, b.cuda_stream, a.cuda_stream])
    assert [r[3] for r in want[0]] == [False, True, True] and want[4] == (3, 3)
    assert got == want
