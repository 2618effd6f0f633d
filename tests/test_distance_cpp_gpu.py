"""lfx::DistanceField (include/lfx.hpp) in a C++ process of its own: the compiled examples/costmap reads scans and two sets
of poses from files, renders the occupancy grid, takes its distance field from the counts and writes the emitted grid and the
costmap; moves the poses and does it again.  Each costmap is the restatement's (tests/distance_restatement.py) of the grid
written next to it, and the printed stats are its stats."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import distance_restatement as D
from tests import occupancy_cases as OC
from tests import segment_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lidar_feature_extraction_amd", "_lib", "costmap")
N = 4
GRID = dict(n_beams=90, width=150, height=110, resolution=0.25, origin_x=-18.5, origin_y=-13.25)
MAX_CELLS = 9


def test_costmap_example_builds_without_a_gpu():
    assert os.path.exists(EXE), "examples/costmap is built with the library (csrc/Makefile, CALLERS)"


@pytest.mark.gpu
def test_the_written_costmaps_are_the_restatements(tmp_path):
    from lidar_feature_extraction_amd import concat, distance_cost_table
    scans = S.scans33()[:N]
    poses, moved = OC.tilted_poses(N, seed=41), OC.tilted_poses(N, seed=42)
    concat(scans).tofile(tmp_path / "scans.bin")
    for name, p in (("poses.txt", poses), ("moved.txt", moved)):
        with open(tmp_path / name, "w") as f:
            for q in p:
                f.write(" ".join("%.17g" % v for v in q.reshape(12)) + "\n")
    out = tmp_path / "out"
    args = [str(tmp_path / "scans.bin"), str(S.RINGS), str(S.COLS), str(N), str(tmp_path / "poses.txt"), str(tmp_path / "moved.txt"), str(out),
            str(GRID["n_beams"]), str(GRID["width"]), str(GRID["height"]), "%.9g" % GRID["resolution"], "%.17g" % GRID["origin_x"], "%.17g" % GRID["origin_y"],
            str(MAX_CELLS)]
    r = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    printed = re.findall(r"(first|second) transform: (\d+) obstacle cells, (\d+) unknown cells, (\d+) far cells, max d2 (\d+)", r.stdout)
    assert [p[0] for p in printed] == ["first", "second"], r.stdout
    w, h = GRID["width"], GRID["height"]
    cfg, cost = D.config(max_cells=MAX_CELLS), D.cost_config()
    lut = distance_cost_table(cost, GRID["resolution"])
    assert D.cost_cells(cost, GRID["resolution"]) == 3 <= MAX_CELLS
    grids = []
    for k, which in enumerate(("first", "second")):
        G = np.fromfile(out / which / "grid.bin", np.int8).reshape(h, w)
        grids.append(G)
        cl, d2 = D.classes(G, cfg), D.d2_separable(G, cfg)
        st = D.stats(G, cfg, d2)
        assert tuple(int(v) for v in printed[k][1:]) == (st["n_obstacle"], st["n_unknown"], st["n_far"], st["max_d2"]), (which, printed[k], st)
        assert st["n_obstacle"] > 20 and st["n_unknown"] > 100 and 0 < st["max_d2"] <= MAX_CELLS ** 2 and st["n_far"] > 0
        want = D.costmap(cl, d2, lut, cost)
        assert len(np.unique(want)) > 4 and (want == 254).any() and (want == 255).any() and (want == 0).any()
        head = b"P5\n%d %d\n255\n" % (w, h)
        assert open(out / which / "costmap.pgm", "rb").read() == head + want[::-1].tobytes(), which
    assert grids[0].tobytes() != grids[1].tobytes()
