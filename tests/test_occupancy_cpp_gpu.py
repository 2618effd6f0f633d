"""lfx::OccupancyGrid (include/lfx.hpp) in a C++ process of its own: the compiled examples/occupancy_map reads scans and two
sets of poses from files, adds every scan, renders and saves the grid, moves the poses, renders and saves again.  Both pairs
of files are the restatement's bytes (tests/occupancy_restatement.py) and the printed counters its counters."""
import os
import re
import subprocess

import pytest

from tests import occupancy_cases as OC
from tests import occupancy_restatement as O
from tests import segment_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lidar_feature_extraction_amd", "_lib", "occupancy_map")
N = 4
GRID = dict(n_beams=90, width=150, height=110, resolution=0.25, origin_x=-18.5, origin_y=-13.25)


def test_occupancy_map_example_builds_without_a_gpu():
    assert os.path.exists(EXE), "examples/occupancy_map is built with the library (csrc/Makefile, CALLERS)"


@pytest.mark.gpu
def test_the_saved_maps_are_the_restatements(tmp_path):
    from lidar_feature_extraction_amd import concat
    scans = S.scans33()[:N]
    poses, moved = OC.tilted_poses(N, seed=41), OC.tilted_poses(N, seed=42)
    concat(scans).tofile(tmp_path / "scans.bin")
    for name, p in (("poses.txt", poses), ("moved.txt", moved)):
        with open(tmp_path / name, "w") as f:
            for q in p:
                f.write(" ".join("%.17g" % v for v in q.reshape(12)) + "\n")
    out = tmp_path / "out"
    args = [str(tmp_path / "scans.bin"), str(S.RINGS), str(S.COLS), str(N), str(tmp_path / "poses.txt"), str(tmp_path / "moved.txt"), str(out),
            str(GRID["n_beams"]), str(GRID["width"]), str(GRID["height"]), "%.9g" % GRID["resolution"], "%.17g" % GRID["origin_x"], "%.17g" % GRID["origin_y"]]
    r = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    cfg = O.config(max_scans=N, **GRID)
    ref = O.Grid(cfg)
    ref.add_scans(scans, poses)
    printed = re.findall(r"(first|second) render: (\d+) hit beams, (\d+) clear beams, (\d+) skipped, (\d+) occupied votes, (\d+) free votes, (\d+) outside", r.stdout)
    assert [p[0] for p in printed] == ["first", "second"], r.stdout
    grids = []
    for k, (which, at) in enumerate((("first", poses), ("second", moved))):
        ref.set_poses(at)
        ref.clear()
        ref.render()
        assert tuple(int(v) for v in printed[k][1:]) == tuple(ref.counters[n] for n in O.COUNTERS), (which, printed[k], ref.counters)
        assert ref.counters["n_window_miss"] == 0 and ref.counters["n_occupied_votes"] > 100 and ref.counters["n_free_votes"] > 1000
        grid = ref.emit()
        grids.append(grid)
        assert open(out / which / "map.pgm", "rb").read() == O.pgm_bytes(grid), which
        assert open(out / which / "map.yaml", "rb").read() == O.yaml_bytes(GRID["resolution"], GRID["origin_x"], GRID["origin_y"]), which
        assert len(set(O.pgm_bytes(grid)[-150 * 110:])) == 3                      # (free, occupied and unknown are all there)
    assert grids[0].tobytes() != grids[1].tobytes()
