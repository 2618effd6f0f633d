"""lfx::LoopCloser and lfx::PlaceDb / Keyframes / PoseGraph (include/lfx.hpp) in a C++ process of its own: the compiled
examples/close_loop_scans runs the drive of tests/loop_closer_cases.py scan by scan.  Its counts, its closures and the poses
of its graph and its store must be what the Python binding gives for the same calls, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import deskew_cases as K
from tests import loop_closer_cases as LC
from tests import scan_context_restatement as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lidar_feature_extraction_amd", "_lib", "close_loop_scans")
HEAD = np.dtype([("counts", "<u4", 3), ("followed", "<i4"), ("code", "<i4"), ("graph", "<f8", (LC.N, 12)), ("store", "<f8", (LC.N, 12))])
CLOSURE = np.dtype([("query", "<u4"), ("candidate", "<u4"), ("accepted", "<i4"), ("reason", "<i4"), ("pose", "<f8", 12)])


def test_close_loop_scans_example_builds_without_a_gpu():
    assert os.path.exists(EXE), "examples/close_loop_scans is built with the library (csrc/Makefile, CALLERS)"


@pytest.mark.gpu
def test_cpp_loop_closing_matches_the_binding(tmp_path):
    from lidar_feature_extraction_amd import FeatureExtraction, concat, pose_graph_edges
    from lidar_feature_extraction_amd import binding as B
    clouds = LC.clouds()
    edges, chained = LC.chain()
    records = pose_graph_edges([e[0] for e in edges], [e[1] for e in edges], [e[2] for e in edges], [e[3] for e in edges])
    paths = [str(tmp_path / name) for name in ("scans.bin", "poses.bin", "edges.bin", "out.bin")]
    concat(clouds).tofile(paths[0])
    chained.tofile(paths[1])
    records.tofile(paths[2])
    w, radius = LC.SUBMAP["submap_half_window"], LC.SUBMAP["submap_radius"]
    r = subprocess.run([EXE, paths[0], str(LC.N), str(SC.RINGS), str(SC.COLS), paths[1], paths[2], str(LC.MIN_GAP), repr(LC.SEARCH_RADIUS),
                        repr(LC.MAX_DISTANCE), str(w), repr(radius), paths[3]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    raw = open(paths[3], "rb").read()
    head = np.frombuffer(raw[:HEAD.itemsize], HEAD)[0]
    got = np.frombuffer(raw[HEAD.itemsize:], CLOSURE)
    assert len(got) == LC.N - LC.MIN_GAP
    # the same calls through the binding: scan by scan, as the example feeds them
    scan = SC.RINGS * SC.COLS
    fx = FeatureExtraction(device=0, max_points_per_scan=scan, max_batch=1, max_points_per_ring=SC.COLS, max_rings=SC.RINGS)
    db = fx.place_db(LC.N)
    kf = fx.keyframes(LC.N, LC.N * scan)
    for k, c in enumerate(clouds):
        fx.ExtractFeatures(c)
        db.add(fx.scan_context(None, None, K.stream()), 1, K.stream())
        kf.add_batch(chained[k:k + 1], K.stream())
        K.sync()                                 # (the next scan replaces the records the descriptor and the keyframe are made from)
    graph = fx.pose_graph(LC.N, 2 * LC.N)
    graph.add_nodes(chained, K.stream())
    graph.add_edges(records, K.stream())
    lc = fx.loop_closer(kf, db, graph, min_gap=LC.MIN_GAP, search_radius=LC.SEARCH_RADIUS, max_distance=LC.MAX_DISTANCE,
                        submap_capacity=scan * (2 * w + 1), submap_half_window=w, submap_radius=radius)
    closures, result = lc.update(LC.MIN_GAP, LC.N - LC.MIN_GAP, K.stream())
    assert [int(x) for x in head["counts"]] == [result["n_detected"], result["n_verified"], result["n_accepted"]] == [6, 6, 6]
    assert bool(head["followed"]) == result["followed"] and int(head["code"]) == result["graph"]["code"]
    assert head["graph"].tobytes() == graph.poses(stream=K.stream()).tobytes()
    assert head["store"].tobytes() == kf.poses(stream=K.stream()).tobytes() == head["graph"].tobytes()
    for g, c in zip(got, closures):
        assert (int(g["query"]), int(g["candidate"]), bool(g["accepted"]), lc.REASONS[g["reason"]]) == (c["query"], c["candidate"], c["accepted"], c["reason"])
        assert g["pose"].tobytes() == c["result"]["pose"].tobytes()
    assert "loop closer: 6 of 6 keyframes have a candidate, 6 verified, 6 accepted" in r.stdout, r.stdout
    assert LC.worst_error(head["graph"]) < LC.worst_error(chained)
    assert result["graph"]["code"] in (B.POSE_GRAPH_CONVERGED, B.POSE_GRAPH_MAX_ITERATIONS)
    lc.close()
    graph.close()
    kf.close()
    db.close()
    fx.close()
