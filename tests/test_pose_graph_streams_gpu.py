"""The pose graph across streams and across objects: "Ordered behind every earlier call on this graph, whichever streams they
used" (lfx_pose_graph_optimize) and "the call queues that wait on `stream`" (lfx_pose_graph_view, which is what
Keyframes.follow(graph) goes through), with the held-producer pattern of tests/test_newer_streams_gpu.py (tests/segment_cases.py
Hold): the producer's stream is kept busy, an event E recorded behind the producer has not been reached when the dependent
call is issued on another stream, and the result is, byte for byte, what one stream gives.

Every call that writes the graph first waits ON THE HOST for the graph's previous call (settle: its staging blocks are
about to be rewritten), and so does the upload of the incidence lists in an optimise that follows added nodes or edges.  A
second call on a held stream would therefore wait out the hold before E could be looked at, so each growth case holds ONE
call: add_nodes, add_edges and set_fixed each have a case of their own.  Only set_fixed leaves the lists as they are, so
only there does the optimise on B reach its hipStreamWaitEvent with the producer still held; behind add_nodes and add_edges
it is the host's wait that orders it, and what those two cases pin is that the call itself returned while its stream was
held, and the bytes."""
import numpy as np
import pytest

from tests import deskew_cases as D
from tests import keyframes_restatement as KR
from tests import pose_graph_cases as K
from tests import segment_cases as S
from tests.test_keyframes_gpu import GUARD, _device_store, _up

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    f = D.fx_for(16, 64, 3)
    yield f
    f.close()


@pytest.fixture(scope="module")
def hold():
    h = S.Hold()
    print("a hold: %d units, %.3f ms per %d measured" % (h.amount, h.ms_per_unit, h.unit))
    yield h
    for what, ms in h.issue_ms:
        print("held %.0f ms; issued %.3f ms after the hold was queued: %s" % (S.HOLD_MS, ms, what))


def _graph():
    """24 nodes, a whole chain (edge k is k -> k + 1), loops (2, 15) = edge 23 and (20, 6) = edge 24"""
    return K.graph(24, loops=[(2, 15), (20, 6)], seed=60)


def _one_stream(fx, poses, edges, fixed=()):
    """(poses, result, rho, w) of a fresh graph built and optimised on one stream"""
    pg = fx.pose_graph(24, 25)
    pg.add_nodes(poses, D.stream())
    for k in fixed:
        pg.set_fixed(k, True, D.stream())
    pg.add_edges(edges, D.stream())
    res = pg.optimize(D.stream())
    out = (pg.poses(stream=D.stream()).tobytes(), res) + tuple(x.tobytes() for x in pg.edge_chi2(stream=D.stream()))
    pg.close()
    return out


def _warmed(fx, hold, g, n_nodes, edges):
    """a graph of the first n_nodes nodes and `edges`, optimised once; two streams that have run the busy kernel"""
    pg = fx.pose_graph(24, 25)
    pg.add_nodes(g["poses"][:n_nodes], D.stream())
    pg.add_edges(edges, D.stream())
    pg.optimize(D.stream())
    a, b = S.two_streams()
    for st in (a, b):
        hold._run(1, st)
    D.sync()
    return pg, a, b, pg.poses(stream=D.stream())


def _same_as_one_stream(pg, res, stream, want):
    got = (pg.poses(stream=stream).tobytes(), res) + tuple(x.tobytes() for x in pg.edge_chi2(stream=stream))
    assert got[1] == want[1] and got[0] == want[0] and got[2:] == want[2:]


def test_add_nodes_on_a_held_stream_then_optimize_on_another(fx, hold):
    """22 nodes with their edges, optimised.  Nodes 22 and 23 are added on held A (no edge reaches them yet); optimise on
    B.  The two nodes come back as they were added; everything is a fresh graph's bytes."""
    g = _graph()
    edges = np.concatenate([g["edges"][:21], g["edges"][23:25]])
    pg, a, b, before = _warmed(fx, hold, g, 22, edges)
    hold(a)
    assert pg.add_nodes(g["poses"][22:], a.cuda_stream) == 22
    e = S.event_behind(a)
    hold.still_held(e, "pose graph: add_nodes on A")
    res = pg.optimize(b.cuda_stream)
    start = np.concatenate([before, g["poses"][22:]])
    _same_as_one_stream(pg, res, b.cuda_stream, _one_stream(fx, start, edges))
    assert pg.poses(22, 2, a.cuda_stream).tobytes() == g["poses"][22:].tobytes()
    D.sync()
    pg.close()


def test_add_edges_on_a_held_stream_then_optimize_on_another(fx, hold):
    """All 24 nodes, the chain up to node 21 and loop (2, 15), optimised.  The chain edges into nodes 22 and 23 and the loop
    (20, 6) are added on held A: the incidence lists go up again and ldy grows with the second loop; optimise on B."""
    g = _graph()
    first, second = np.concatenate([g["edges"][:21], g["edges"][23:24]]), np.concatenate([g["edges"][21:23], g["edges"][24:25]])
    pg, a, b, before = _warmed(fx, hold, g, 24, first)
    hold(a)
    pg.add_edges(second, a.cuda_stream)
    e = S.event_behind(a)
    hold.still_held(e, "pose graph: add_edges on A")
    res = pg.optimize(b.cuda_stream)
    assert (res["n_chain"], res["n_loop"]) == (23, 2)
    _same_as_one_stream(pg, res, b.cuda_stream, _one_stream(fx, before, np.concatenate([first, second])))
    D.sync()
    pg.close()


def test_set_fixed_on_a_held_stream_then_optimize_on_another(fx, hold):
    """The whole graph, optimised; other poses written; then node 5 is fixed on held A and optimise is issued on B while A
    has not run.  The lists are current, so optimise waits for nothing on the host: only its hipStreamWaitEvent on the
    graph's event puts the linearisation behind the flag's copy.  A fresh graph with node 5 fixed gives the same bytes, and
    node 5 has not moved (without the wait it is free and moves)."""
    g = _graph()
    pg, a, b, _ = _warmed(fx, hold, g, 24, g["edges"])
    pg.set_poses(g["poses"], 0, D.stream())
    D.sync()
    hold(a)
    pg.set_fixed(5, True, a.cuda_stream)
    e = S.event_behind(a)
    hold.still_held(e, "pose graph: set_fixed on A, optimize on B")
    res = pg.optimize(b.cuda_stream)
    _same_as_one_stream(pg, res, b.cuda_stream, _one_stream(fx, g["poses"], g["edges"], fixed=(5,)))
    assert pg.poses(5, 1, b.cuda_stream).tobytes() == g["poses"][5:6].tobytes()
    D.sync()
    pg.close()


def test_keyframes_follow_a_graph_across_streams(fx, hold):
    """(2) set_poses of the whole graph on held A, follow(graph) on B -- lfx_pose_graph_view queues the graph's wait on B --
    and build on a third stream: the cloud is the one at the poses written on A.  (3) The reverse: follow(device array)
    on held B, then set_poses of the graph on A, then build on the third stream: the build shows the followed poses, the
    graph the set ones.  Every stream has run the busy kernel and a build before the part that counts."""
    import torch
    store, _c, edge, surface, poses = KR.sphere_case()
    n = len(store)
    want = KR.Store(n, store.max_points)
    assert want.add(edge, surface, poses) == 0
    kf = _device_store(fx, want)
    pg = fx.pose_graph(n, 1)
    pg.add_nodes(poses, D.stream())
    a, b = S.two_streams()
    third = torch.cuda.Stream()
    others = [KR.bits_poses(n, seed) for seed in (23, 24, 25)]
    d_other = _up(others[1], np.float64)
    room = int(store.max_points[0])
    outs = [torch.full((room + GUARD, 4), -123.25, dtype=torch.float32, device=D.dev()) for _ in range(3)]
    for st in (a, b, third):
        hold._run(1, st)
        kf.build("edge", d_out=outs[2].data_ptr(), capacity_points=room, stream=st.cuda_stream)
    D.sync()

    def check(out, count, stream):
        stream.synchronize()
        host = out.cpu().numpy()
        cloud = want.build(KR.EDGE)
        assert count == len(cloud) and host[:count].tobytes() == cloud.tobytes() and (host[count:] == -123.25).all()

    # (2)
    hold(a)
    pg.set_poses(others[0], 0, a.cuda_stream)
    e = S.event_behind(a)
    kf.follow(pg, stream=b.cuda_stream)
    hold.still_held(e, "set_poses of the graph on A, keyframes follow(graph) on B, build on a third stream")
    count = kf.build("edge", d_out=outs[0].data_ptr(), capacity_points=room, stream=third.cuda_stream)
    want.set_poses(others[0])
    check(outs[0], count, third)
    assert want.build(KR.EDGE).tobytes() != store.build(KR.EDGE).tobytes()
    # (3)
    D.sync()
    hold(b)
    kf.follow(d_other.data_ptr(), 0, n, b.cuda_stream)
    e = S.event_behind(b)
    pg.set_poses(others[2], 0, a.cuda_stream)
    hold.still_held(e, "keyframes follow(array) on B, set_poses of the graph on A, build on a third stream")
    count = kf.build("edge", d_out=outs[1].data_ptr(), capacity_points=room, stream=third.cuda_stream)
    want.set_poses(others[1])
    check(outs[1], count, third)
    assert pg.poses(stream=a.cuda_stream).tobytes() == others[2].tobytes()
    D.sync()
    assert kf.poses(stream=D.stream()).tobytes() == others[1].tobytes()
    assert kf.build("surface").cpu().numpy().tobytes() == want.build(KR.SURFACE).tobytes()
    kf.close()
    pg.close()
