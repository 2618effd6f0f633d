"""The loop closer on the device (include/lfx.h, the loop closer section) over the drive of tests/loop_closer_cases.py:
extract -> scan_context -> PlaceDb, Keyframes.add_batch at the chained poses, PoseGraph nodes and chain edges.  detect
against the restated gated query; verify and update against the hand composition of the public calls they are defined as,
byte for byte; the acceptance thresholds at equality; what is refused and what is left untouched.

MEASURED on the device (printed by test_update_closes_the_loops): the worst position error of nodes 6-11 is 0.719 m chained
and 0.146 m after update(6, 6)."""
import numpy as np
import pytest

from tests import deskew_cases as K
from tests import loop_closer_cases as LC
from tests import loop_closer_restatement as LR
from tests import scan_context_restatement as SC

pytestmark = pytest.mark.gpu

SCAN = SC.RINGS * SC.COLS
CAPACITY = 5 * SCAN                                                     # a submap holds at most the window's five keyframes


class Drive:
    """The drive's store, index and graph on the device; closers over them by config."""

    def __init__(self, **graph_fields):
        from lidar_feature_extraction_amd import pose_graph_edges
        self.cfg = SC.config()
        self.edges, self.chained = LC.chain()
        self.fx = K.fx_for(SC.RINGS, SC.COLS, LC.N)
        self.d, self.got = K.extract(self.fx, LC.clouds())
        self.fx.batch_status(K.stream())
        desc = self.fx.scan_context(self.cfg, None, K.stream())
        self.db = self.fx.place_db(16, self.cfg)
        self.db.add(desc, LC.N, K.stream())
        self.kf = self.fx.keyframes(16, LC.N * SCAN)
        self.kf.add_batch(self.chained, K.stream())
        self.chain_records = pose_graph_edges([e[0] for e in self.edges], [e[1] for e in self.edges], [e[2] for e in self.edges],
                                              [e[3] for e in self.edges])
        self.graph = self.new_graph(**graph_fields)
        self.made = [self.graph]

    def new_graph(self, **fields):
        g = self.fx.pose_graph(16, 32, **fields)
        g.add_nodes(self.chained, K.stream())
        g.add_edges(self.chain_records, K.stream())
        return g

    def closer(self, graph=None, **config):
        fields = dict(min_gap=LC.MIN_GAP, search_radius=LC.SEARCH_RADIUS, max_distance=LC.MAX_DISTANCE, n_candidates=LC.N_CANDIDATES,
                      submap_capacity=CAPACITY, **LC.SUBMAP)
        fields.update(config)
        lc = self.fx.loop_closer(self.kf, self.db, graph or self.graph, **fields)
        self.made.append(lc)
        return lc

    def state(self, graph=None):
        """every byte the closer may write: the graph's poses, its edge count, the store's poses"""
        g = graph or self.graph
        return g.poses(stream=K.stream()).tobytes(), g.info()["n_edges"], self.kf.poses(stream=K.stream()).tobytes()

    def compose(self, q, cand, leaf=1.0, n_neighbors=15, max_iter=20, cell=1.0):
        """verify of keyframe q against the match dict `cand`, by the four public calls it is defined as."""
        import torch
        fx, kf, st = self.fx, self.kf, K.stream()
        c = cand["entry"]
        pose_c = kf.poses(c, 1, st)[0]
        lo, count = LR.window(c, q, LC.MIN_GAP, LC.SUBMAP["submap_half_window"])
        subs = [kf.submap(kind, pose_c[:, 3], LC.SUBMAP["submap_radius"], lo, count, capacity_points=CAPACITY, stream=st) for kind in ("edge", "surface")]
        maps = [fx.make_map(cloud.data_ptr(), res["n_points"], cell, st) for cloud, res in subs]
        v = kf.view(st)
        begin = [kf._range_points(kind, 0, q) for kind in (0, 1)]
        n = [kf._range_points(kind, q, 1) for kind in (0, 1)]
        words = torch.tensor([0, n[0], n[1], 0, 0, 0, 0, 0], dtype=torch.int32, device=K.dev())
        w = words.data_ptr()
        edge, surface = v["points"][0] + 16 * begin[0], v["points"][1] + 16 * begin[1]
        down = torch.zeros((n[1] + 1, 4), dtype=torch.float32, device=K.dev())
        if leaf > 0.0:
            fx.voxel_downsample(surface, w, w + 8, 1, 1, n[1], leaf, down.data_ptr(), w + 12, w + 16, st)
        K.sync()
        n_down, status = (int(words[3]), int(words[4])) if leaf > 0.0 else (0, 1)      # (no downsample: the cloud as stored)
        scan, count_at, n_scan = (down.data_ptr(), w + 12, n_down) if status == 0 else (surface, w + 8, n[1])
        res, rep = fx.scan_to_map_align(maps[0], maps[1], n_neighbors, max_iter, edge, w, w + 4, 1, n[0], n[0], scan, w, count_at, 1, n_scan, n_scan,
                                        [LR.initial_pose(pose_c, cand["yaw"])], st, report=True)
        for m in maps:
            m.close()
        return dict(pose_c=pose_c, result=res[0], report=rep[0], submap=[s[1] for s in subs])

    def close(self):
        for x in reversed(self.made):
            x.close()
        self.kf.close()
        self.db.close()
        del self.d
        self.fx.close()


def _same(closure, hand, q, c, scale=True):
    """a closure dict equals the hand composition: pose, error, code, the report's bytes, both submaps, the edge"""
    r, h = closure["result"], hand["result"]
    assert closure["query"] == q and closure["candidate"] == c
    assert r["pose"].tobytes() == h["pose"].tobytes() and (r["error"], r["error_scale"], r["iteration"], r["code"]) == (
        h["error"], h["error_scale"], h["iteration"], h["code"]), (q, r, h)
    assert closure["report"]["raw"] == hand["report"]["raw"], q
    assert closure["submap"] == hand["submap"], (closure["submap"], hand["submap"])
    i, j, z, om = LR.edge(c, q, hand["pose_c"], h["pose"], hand["report"]["information"], hand["report"]["sigma2"], scale)
    e = closure["edge"]
    assert (int(e["i"]), int(e["j"]), int(e["flags"])) == (i, j, 1)
    assert e["z"].tobytes() == z.tobytes() and e["information"].tobytes() == om.tobytes(), q
    want = LR.judge({}, h["code"], hand["report"])
    assert closure["reason"] == want and closure["accepted"] == (want == "accepted"), (q, closure["reason"], want)


def _tuples(rows):
    return [[(0xFFFFFFFF if m["entry"] is None else m["entry"], m["shift"], m["distance"], m["yaw"]) for m in row] for row in rows]


def test_detect_equals_the_restated_gated_query():
    d = Drive()
    lc = d.closer()
    desc = d.db.download(stream=K.stream())
    for first, count in ((6, 6), (0, 12), (5, 2), (11, 1)):
        got, n_eligible = lc.detect(first, count, K.stream())
        want, counts = LR.detect(desc, d.chained, first, count, LC.MIN_GAP, LC.SEARCH_RADIUS, LC.MAX_DISTANCE, LC.N_CANDIDATES)
        assert _tuples(got) == want and n_eligible == counts, (first, count, got, want)
    got, _ = lc.detect(6, 6, K.stream())
    assert [row[0]["entry"] for row in got] == [0, 1, 2, 3, 4, 5]
    assert lc.info()["device_bytes"] >= 16 * (2 * CAPACITY + min(CAPACITY, LC.N * SCAN))
    d.close()


def test_verify_equals_the_hand_composition():
    """One revisit whose submap is one keyframe (node 6 against 0) and one whose submap is two (node 8 against 2, with 1)."""
    d = Drive()
    lc = d.closer()
    got, _ = lc.detect(6, 6, K.stream())
    before = d.state()
    for q in (6, 8):
        cand = got[q - 6][0]
        hand = d.compose(q, cand)
        closure = lc.verify(q, cand, K.stream())
        _same(closure, hand, q, cand["entry"])
        assert closure["accepted"] and closure["match"] == cand
    assert d.compose(8, got[2][0])["submap"][0]["n_written_keyframes"] == 2
    assert d.state() == before                                          # (a verification writes nothing)
    # without the scaling the edge carries B H B^T as it is
    plain = d.closer(scale_by_sigma2=0)
    _same(plain.verify(6, got[0][0], K.stream()), d.compose(6, got[0][0]), 6, 0, scale=False)
    # a downsample output smaller than the query's surface cloud: LFX_ERR_CAPACITY -- unless no downsample runs
    from lidar_feature_extraction_amd import binding as B
    with pytest.raises(B.LfxError) as err:
        d.closer(downsample_capacity=10).verify(6, got[0][0], K.stream())
    assert err.value.code == B.ERR_CAPACITY
    stored = d.closer(downsample_capacity=10, surface_leaf=0.0)
    _same(stored.verify(8, got[2][0], K.stream()), d.compose(8, got[2][0], leaf=0.0), 8, 2)
    assert stored.info()["device_bytes"] < lc.info()["device_bytes"]
    assert d.state() == before
    d.close()


def test_update_closes_the_loops():
    from lidar_feature_extraction_amd import binding as B
    d = Drive()
    lc = d.closer()
    got, _ = lc.detect(6, 6, K.stream())
    hands = [d.compose(q, got[q - 6][0]) for q in range(6, 12)]
    closures, result = lc.update(6, 6, K.stream())
    for q, (closure, hand) in enumerate(zip(closures, hands), 6):
        _same(closure, hand, q, q - 6)
    assert result["n_detected"] == 6 and result["n_verified"] == 6 and result["n_accepted"] == 6 and result["followed"]
    assert result["graph"]["code"] in (B.POSE_GRAPH_CONVERGED, B.POSE_GRAPH_MAX_ITERATIONS) and result["graph"]["n_loop"] == 6
    # a second graph given the same edges by hand and optimised
    second = d.new_graph()
    d.made.append(second)
    second.add_edges(np.array([c["edge"] for c in closures], B.POSE_GRAPH_EDGE_DTYPE), K.stream())
    want = second.optimize(K.stream())
    assert want == result["graph"]
    poses = d.graph.poses(stream=K.stream())
    assert poses.tobytes() == second.poses(stream=K.stream()).tobytes()
    assert d.kf.poses(stream=K.stream()).tobytes() == poses.tobytes()
    before, after = LC.worst_error(d.chained), LC.worst_error(poses)
    print("worst position error of nodes 6-11: chained %.3f m, after update %.3f m" % (before, after))
    for c in closures:
        print("node %d against %d: code %d, rms edge %.4f surface %.4f, inliers %d of %d, sigma2 %.3e" % (
            c["query"], c["candidate"], c["result"]["code"], c["report"]["rms_edge"], c["report"]["rms_surface"],
            c["report"]["n_edge_inliers"] + c["report"]["n_surface_inliers"], c["report"]["n_edge"] + c["report"]["n_surface"], c["report"]["sigma2"]))
    assert after < before
    d.close()


def test_acceptance_at_equality_and_rejections_leave_everything_as_it_was():
    d = Drive()
    lc = d.closer()
    got, _ = lc.detect(6, 6, K.stream())
    q, cand = 7, got[1][0]
    rep = d.compose(q, cand)["report"]
    before = d.state()
    for field, reason in (("max_rms_surface", "rms_surface"), ("max_rms_edge", "rms_edge")):
        at = float(rep[reason])
        assert at > 0.0
        assert d.closer(**{field: at}).verify(q, cand, K.stream())["accepted"]
        below = d.closer(**{field: float(np.nextafter(at, 0.0))}).verify(q, cand, K.stream())
        assert not below["accepted"] and below["reason"] == reason
    # max_distance: <= keeps, one float below drops the candidate
    kept, _ = d.closer(max_distance=cand["distance"]).detect(q, 1, K.stream())
    dropped, n_eligible = d.closer(max_distance=float(np.nextafter(cand["distance"], 0.0))).detect(q, 1, K.stream())
    assert kept[0][0] == cand and dropped[0][0]["entry"] is None and dropped[0][0]["distance"] == float("inf") and n_eligible == [1]
    # an update that rejects every closure writes nothing
    closures, result = d.closer(max_rms_surface=0.0).update(6, 6, K.stream())
    assert [c["reason"] for c in closures] == ["rms_surface"] * 6 and not any(c["accepted"] for c in closures)
    assert result == dict(n_detected=6, n_verified=6, n_accepted=0, followed=False, graph=None)
    closures, result = d.closer(max_distance=0.0).update(6, 6, K.stream())
    assert [c["reason"] for c in closures] == ["no_candidate"] * 6 and result["n_detected"] == 0 and result["n_verified"] == 0
    assert d.state() == before
    d.close()


def test_nothing_to_detect_refusals_and_a_full_graph():
    from lidar_feature_extraction_amd import binding as B
    d = Drive()
    before = d.state()
    far = d.closer(min_gap=100)
    got, n_eligible = far.detect(0, 12, K.stream())
    assert all(m["entry"] is None for row in got for m in row) and n_eligible == [0] * 12
    closures, result = far.update(0, 12, K.stream())
    assert result == dict(n_detected=0, n_verified=0, n_accepted=0, followed=False, graph=None) and d.state() == before
    lc = d.closer()
    cand = lc.detect(6, 6, K.stream())[0][0][0]
    d.graph.add_nodes(d.chained[:1], K.stream())                         # (a 13th node: the smallest of the three sizes is still 12)
    before = d.state()
    for call in (lambda: lc.detect(12, 1, K.stream()), lambda: lc.detect(11, 2, K.stream()), lambda: lc.update(11, 2, K.stream()),
                 lambda: lc.update(6, 0, K.stream()), lambda: lc.verify(12, cand, K.stream()), lambda: lc.verify(5, cand, K.stream()),
                 lambda: lc.verify(6, dict(entry=None, yaw=0.0), K.stream()), lambda: d.closer(n_candidates=17),
                 lambda: d.closer(submap_capacity=0), lambda: d.closer(search_radius=-1.0)):
        with pytest.raises(B.LfxError) as err:
            call()
        assert err.value.code == B.ERR_INVALID_ARGUMENT, err.value
    assert d.state() == before
    # a graph with room for two loop edges: LFX_ERR_CAPACITY, the closures filled, the graph untouched
    small = d.new_graph(max_loop_edges=2)
    d.made.append(small)
    tight = d.closer(graph=small)
    before = d.state(small)
    rc, closures, result = tight.update_raw(6, 6, K.stream())
    assert rc == B.ERR_CAPACITY
    assert all(c.accepted and c.query == 6 + s and c.candidate == s for s, c in enumerate(closures))
    assert result.n_verified == 6 and result.followed == 0
    assert d.state(small) == before
    d.close()
