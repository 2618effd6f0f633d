"""lfx::GridMatcher (include/lfx.hpp) in a C++ process of its own: the compiled examples/localize_grid reads scans and poses
from files, renders the occupancy grid, makes the score field, reduces one scan through a grid of 1 x 1 cells, searches for
it from a centre that is off and hands the lifted pose to lfx::Localizer.  The best it writes is the Python binding's for the
same calls, and the pose found is the restatement's candidate of that index."""
import os
import subprocess

import numpy as np
import pytest

from tests import deskew_cases as K
from tests import grid_match_cases as GC
from tests import grid_match_restatement as G
from tests import occupancy_cases as OC
from tests import segment_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lidar_feature_extraction_amd", "_lib", "localize_grid")
N, QUERY = 4, 2
GRID = dict(n_beams=90, width=150, height=110, resolution=0.25, origin_x=-18.5, origin_y=-13.25)
OFF = (3, -2, 2)
THETA_STEP = 0.01


def test_localize_grid_example_builds_without_a_gpu():
    assert os.path.exists(EXE), "examples/localize_grid is built with the library (csrc/Makefile, CALLERS)"


@pytest.mark.gpu
def test_the_example_finds_what_the_binding_finds(tmp_path):
    from lidar_feature_extraction_amd import DistanceField, GridMatcher, OccupancyGrid, concat
    scans = S.scans33()[:N]
    poses = OC.tilted_poses(N, seed=41)
    concat(scans).tofile(tmp_path / "scans.bin")
    with open(tmp_path / "poses.txt", "w") as f:
        for q in poses:
            f.write(" ".join("%.17g" % v for v in q.reshape(12)) + "\n")
    out = tmp_path / "out.bin"
    args = [str(tmp_path / "scans.bin"), str(S.RINGS), str(S.COLS), str(N), str(tmp_path / "poses.txt"), str(QUERY), str(GRID["n_beams"]), str(GRID["width"]),
            str(GRID["height"]), "%.9g" % GRID["resolution"], "%.17g" % GRID["origin_x"], "%.17g" % GRID["origin_y"], str(OFF[0]), str(OFF[1]), str(OFF[2]),
            "%.17g" % THETA_STEP, str(out)]
    r = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    raw = open(out, "rb").read()
    best = np.frombuffer(raw[:16], np.uint32)
    centre, found, initial, refined = (np.frombuffer(raw[16 + 8 * a:16 + 8 * b], np.float64) for a, b in ((0, 3), (3, 6), (6, 18), (18, 30)))
    # the same calls through the Python binding
    fx = K.fx_for(S.RINGS, S.COLS, N)
    g = OccupancyGrid(fx, GRID["width"], GRID["height"], GRID["resolution"], (GRID["origin_x"], GRID["origin_y"]), N, n_beams=GRID["n_beams"])
    d = S.device_batch(fx, scans)
    g.add_batch(poses, stream=K.stream())
    g.render(stream=K.stream())
    df = DistanceField(fx, GRID["width"], GRID["height"])
    df.from_occupancy(g, stream=K.stream())
    m = GridMatcher(fx, GRID["width"], GRID["height"], GRID["resolution"], (GRID["origin_x"], GRID["origin_y"]), max_scans=1, max_beams=GRID["n_beams"])
    m.set_field(df, stream=K.stream())
    level = poses[QUERY].copy()
    level[:, 3] = 0.0
    r1 = OccupancyGrid(fx, 1, 1, GRID["resolution"], (GRID["origin_x"], GRID["origin_y"]), 1, n_beams=GRID["n_beams"])
    r1.truncate(0)
    r1.add_batch(np.stack([level] * N), select=[int(k == QUERY) for k in range(N)], stream=K.stream())
    m.set_scans_occupancy(r1, 0, 1, stream=K.stream())
    res = float(np.float32(GRID["resolution"]))
    want_centre = np.array([poses[QUERY][0, 3] + OFF[0] * res, poses[QUERY][1, 3] + OFF[1] * res, OFF[2] * THETA_STEP])
    GC.same_bytes(centre, want_centre, "centre")
    window = G.search_config(half_x=abs(OFF[0]) + 2, half_y=abs(OFF[1]) + 2, half_theta=abs(OFF[2]) + 1, step_cells=1, theta_step=THETA_STEP)
    got, _, _ = m.search([want_centre], window, stream=K.stream())
    K.sync()
    GC.same_bytes(best, GC.as_u32(got)[0], "the example's best against the binding's")
    assert best[0] > 0 and best[3] > 20 and best[2] > 0
    GC.same_bytes(found, G.candidate(window, GRID["resolution"], want_centre, int(best[1])), "the pose found")
    GC.same_bytes(initial.reshape(3, 4), G.pose3(found, poses[QUERY][:, :3], poses[QUERY][2, 3]), "the lifted pose")
    assert refined.shape == (12,) and "update " in r.stdout                    # (the alignment ran from the lifted pose; how it ends is the scene's)
    for o in (m, r1, df, g):
        o.close()
    fx.close()
    del d
