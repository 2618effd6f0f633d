"""lfx::PoseGraph's priors (include/lfx.hpp) in a C++ process of its own: the compiled examples/anchor_loop chains a drifting
two-lap circle from a first pose whose heading is off, gives every 16th node a position fix with a lever arm, releases the
first node, optimises and prints the worst position error and the heading error at node 0 before and after.  The same
graph through the Python binding must give the same poses, bit for bit, and the printed figures must be the ones computed
here from its file, character for character."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import deskew_cases as D
from tests import pose_graph_cases as K
from tests import pose_graph_prior_cases as PK
from tests import pose_graph_prior_restatement as Q
from tests import pose_graph_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lidar_feature_extraction_amd", "_lib", "anchor_loop")


def test_anchor_loop_example_builds_without_a_gpu():
    assert os.path.exists(EXE), "examples/anchor_loop is built with the library (csrc/Makefile, CALLERS)"


def _heading_error(poses, truth_yaw):
    d = np.arctan2(poses[0, 1, 0], poses[0, 0, 0]) - truth_yaw
    return float(np.arctan2(np.sin(d), np.cos(d)))


@pytest.mark.gpu
def test_cpp_priors_match_the_binding(tmp_path):
    n, P = 128, 8
    dst = str(tmp_path / "graph.bin")
    r = subprocess.run([EXE, str(n), dst], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    raw = open(dst, "rb").read()
    assert np.frombuffer(raw, "<u4", 2).tolist() == [n, P]
    at = 8
    start = np.frombuffer(raw, "<f8", 12 * n, at).reshape(n, 3, 4)
    at += 96 * n
    edges = np.frombuffer(raw, K.EDGE, n - 1, at)
    at += 400 * (n - 1)
    priors = np.frombuffer(raw, PK.PRIOR, P, at)
    at += 416 * P
    cpp = np.frombuffer(raw, "<f8", 12 * n, at).reshape(n, 3, 4)
    assert at + 96 * n == len(raw)
    assert (priors["flags"] == (Q.PRIOR_POSITION | Q.PRIOR_ROBUST)).all() and priors["node"].tolist() == list(range(0, n, 16))
    assert np.allclose(priors["lever"], PK.LEVER) and (edges["j"] == edges["i"] + 1).all()
    fx = D.fx_for(16, 900, 1)
    pg = fx.pose_graph(n, len(edges), max_iter=20)
    pg.add_nodes(start, D.stream())
    pg.add_edges(edges, D.stream())
    pg.reserve_priors(P)
    pg.add_priors(priors, D.stream())
    pg.release_first(True, D.stream())
    res = pg.optimize(D.stream())
    got = pg.poses(stream=D.stream())
    info, pinfo = pg.info(), pg.prior_info()
    assert got.tobytes() == cpp.tobytes()
    ang = 4.0 * np.pi * np.arange(n) / n
    truth = np.zeros((n, 3, 4))
    truth[:, 0, 3], truth[:, 1, 3] = 20.0 * np.cos(ang), 20.0 * np.sin(ang)
    before, after = K.worst_error(start, truth), K.worst_error(got, truth)
    hb, ha = _heading_error(start, np.pi / 2.0), _heading_error(got, np.pi / 2.0)
    # the figures the binding gives, formatted as the example formats them: the same characters
    lines = r.stdout.splitlines()
    assert lines[0] == "pose graph: %d nodes, %d chain and %d loop edges, %d priors, %d bytes on the device" % (n, n - 1, 0, P, info["device_bytes"])
    assert lines[1] == "optimised: code %d after %d iterations, chi2 %.6e -> %.6e (the priors' share %.6e), last step %.3e" % (
        res["code"], res["iterations"], res["chi2_initial"], res["chi2_final"], pinfo["chi2"], res["max_step"])
    m = re.fullmatch(r"worst position error: ([0-9.]+) m before, ([0-9.]+) m after", lines[2])
    assert m and abs(float(m.group(1)) - before) <= 1e-6 and abs(float(m.group(2)) - after) <= 1e-6
    m = re.fullmatch(r"heading error at node 0: (-?[0-9.]+) rad before, (-?[0-9.]+) rad after", lines[3])
    assert m and abs(float(m.group(1)) - hb) <= 1e-6 and abs(float(m.group(2)) - ha) <= 1e-6
    print("binding: worst position error %.6f -> %.6f m, heading error at node 0 %.6f -> %.6f rad" % (before, after, hb, ha))
    assert res["code"] == R.CONVERGED and after < before and abs(ha) < abs(hb) and abs(hb - 0.03) < 1e-9
    # ... and the restatement agrees with both
    want, wres, _, _ = Q.optimize(start, edges, priors, (), True, max_iter=20)
    diff = float(np.abs(got - want).max())
    print("device - restatement %.3e (64 f = %.2e); iterations %d (%d)" % (diff, 64 * K.floors()[0], res["iterations"], wres["iterations"]))
    assert diff <= 64 * K.floors()[0] and abs(wres["iterations"] - res["iterations"]) <= 1
    pg.close()
    fx.close()
