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


# --- the batch calls ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batches():
    """A context for batches of two scans and four scans of the same sensor."""
    from lidar_feature_extraction_amd import make_sequence
    clouds, _ = make_sequence(4, RINGS, COLS, seed=8401)
    fx = K.fx_for(RINGS, COLS, 2)
    yield fx, clouds
    fx.close()


@pytest.mark.parametrize("deskewed", [False, True])
def test_update_batch_on_a_then_b(batches, deskewed):
    """Two batches of two scans through lfx_odometry_update_batch (lfx_odometry_update_batch_deskewed), the first on A, the
    second on B.  The second call rewrites the downsampled clouds, the pinned scan_info and the lengths while the first call's
    last append may still be queued on A; nothing is waited for on the host between the calls (the second extraction is
    ordered behind A by an event -- the context's clouds are the caller's to keep -- and B behind the extraction).  Results
    and store equal those of the same calls on one stream."""
    import torch
    fx, clouds = batches
    a, b = S.two_streams()

    def run(streams):
        odo = fx.odometry(n_local_scans=2)
        cur, out, keep, last = torch.cuda.current_stream(), [], [], None
        for i, st in enumerate(streams):
            if last is not None:
                cur.wait_stream(last)
            keep.append(S.device_batch(fx, clouds[2 * i:2 * i + 2]))
            st.wait_stream(cur)
            out += odo.update_batch_deskewed(None, None, 1.0, "end", 2, st.cuda_stream) if deskewed else odo.update_batch(2, st.cuda_stream)
            last = st
        state = _state(odo, out)
        odo.close()
        return state

    want = run([torch.cuda.current_stream()] * 2)
    got = run([a, b])
    assert [r[3] for r in want[0]] == [False, True, True, True] and want[4] == (4, 4)
    assert got == want


def test_a_refusal_in_the_middle_of_a_batch(batches, tmp_path):
    """An edge store one record too small for scans 0 and 1 together: lfx_odometry_update_batch on A appends scan 0 and
    refuses scan 1 -- LFX_ERR_INVALID_ARGUMENT, "the scan (...) does not fit the odometry's store beside its window" -- with
    scan 0's append queued behind it.  Then, on B, the view, lfx_odometry_save and one more lfx_odometry_update (scan 2's
    surface cloud and as many of its edge records as still fit): the result, the files and the store equal those of the
    same calls on one stream."""
    import torch
    from lidar_feature_extraction_amd import binding as B
    fx, clouds = batches
    a, b = S.two_streams()
    _, (g2,) = K.extract(fx, clouds[2:3])
    e2, s2 = (np.ascontiguousarray(p, np.float32).reshape(-1, 4).copy() for p in (g2.edge_points, g2.surface_points))
    d, got01 = K.extract(fx, clouds[:2])
    ne, ns = [len(g.edge_points) for g in got01], [len(g.surface_points) for g in got01]
    assert ne[1] > 16 and len(e2) > 16
    e2 = e2[:min(len(e2), ne[1] - 1)]
    d_e2, d_s2 = torch.from_numpy(e2).to(K.dev()), torch.from_numpy(s2).to(K.dev())
    K.sync()

    def run(st_batch, st_rest, where):
        odo = fx.odometry(n_local_scans=2, edge_capacity_points=ne[0] + ne[1] - 1)
        with pytest.raises(B.LfxError) as err:
            odo.update_batch(2, st_batch)
        assert err.value.code == -1 and str(err.value) == (
            "lfx error -1: the scan (%d edge, %d surface points) does not fit the odometry's store beside its window" % (ne[1], ns[1]))
        v = odo.view()
        assert (v["n_scans"], v["n_added"], v["n_edge"], v["n_surface"]) == (1, 1, ne[0], ns[0])
        where.mkdir()
        assert odo.save(str(where), st_rest) == (True, True)
        out = [odo.update(d_e2.data_ptr(), len(d_e2), d_s2.data_ptr(), len(d_s2), st_rest)]
        state = _state(odo, out), (where / "edge.pcd").read_bytes(), (where / "surface.pcd").read_bytes()
        odo.close()
        return state

    want = run(K.stream(), K.stream(), tmp_path / "one")
    got = run(a.cuda_stream, b.cuda_stream, tmp_path / "two")
    assert want[0][0][0][3] is True and want[0][4] == (2, 2)
    assert got == want
