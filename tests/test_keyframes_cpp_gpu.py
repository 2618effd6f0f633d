"""lfx::Keyframes (include/lfx.hpp) in a C++ process of its own: the compiled examples/repose_map puts a small cloud per
keyframe of close_loop's drifted two-lap circle into a store, builds the map before and after the graph is optimised and the
store has followed it, cuts a submap around the lap-closing keyframe and localises that keyframe's cloud against it.

The thresholds: the map's error after `follow` is smaller than before; the graph's figures are the ones examples/close_loop
prints for the same circle; the localisation succeeds and lands within E2E_BOUND (0.06 m, tests/test_mapping_gpu.py's bound
for localisation) of where the submap has that place -- the corrected pose of the first-lap keyframe that stands at the same
spot.  The scene is the example's own (walls, ground, poles: every direction is held by a plane or a line), not a scan through
the extraction: the example has no scans."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "lidar_feature_extraction_amd", "_lib")
EXE, CLOSE_LOOP = os.path.join(LIB, "repose_map"), os.path.join(LIB, "close_loop")
E2E_BOUND = 0.06                              # tests/test_mapping_gpu.py: E2E_BOUND


def test_repose_map_example_builds_without_a_gpu():
    assert os.path.exists(EXE), "examples/repose_map is built with the library (csrc/Makefile, CALLERS)"


@pytest.mark.gpu
def test_the_map_follows_the_graph_and_the_loop_is_measured(tmp_path):
    from lidar_feature_extraction_amd import read_pcd
    n, loops = 128, 4
    r = subprocess.run([EXE, str(n), str(loops), str(tmp_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    ref = subprocess.run([CLOSE_LOOP, str(n), str(loops)], capture_output=True, text=True, timeout=120)
    assert ref.returncode == 0, (ref.stdout, ref.stderr)
    # the graph is close_loop's: the same figures, character for character
    for pattern in (r"optimised: code .*", r"worst position error: .*"):
        assert re.search(pattern, r.stdout).group(0) == re.search(pattern, ref.stdout).group(0)
    before = re.search(r"map point error before: worst ([0-9.]+) m, mean ([0-9.]+) m", r.stdout)
    after = re.search(r"map point error after: worst ([0-9.]+) m, mean ([0-9.]+) m", r.stdout)
    assert before and after, r.stdout
    assert float(after.group(1)) < float(before.group(1)) and float(after.group(2)) < float(before.group(2))
    m = re.search(r"localised keyframe (\d+) against it: code (\d+) .* ([0-9.]+) m from keyframe (\d+) before, ([0-9.]+) m after", r.stdout)
    assert m, r.stdout
    assert (int(m.group(1)), int(m.group(4))) == (n - 1, n // 2 - 1) and int(m.group(2)) <= 2          # LFX_ALIGN_SUCCESS
    assert float(m.group(5)) < E2E_BOUND
    s = re.search(r"submap around keyframe \d+: keyframes (\d+) \.\. (\d+), (\d+) edge and (\d+) surface records", r.stdout)
    assert s and int(s.group(2)) < n // 2 and int(s.group(3)) > 0 and int(s.group(4)) > 0
    # the saved map is the corrected one: as many records as the store holds
    k = re.search(r"keyframe store: (\d+) keyframes, (\d+) edge and (\d+) surface records", r.stdout)
    assert int(k.group(1)) == n
    assert len(read_pcd(str(tmp_path / "edge.pcd"))) == int(k.group(2)) and len(read_pcd(str(tmp_path / "surface.pcd"))) == int(k.group(3))
