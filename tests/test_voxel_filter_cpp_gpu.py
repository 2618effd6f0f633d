"""lfx::VoxelFilter and lfx::Keyframes::SaveFiltered (include/lfx.hpp) in a C++ process of its own: the compiled
examples/filter_map reads the scene of tests/visibility_cases.py from PCD files, votes into the store's own flags, writes
the map of each kind without the flagged records and thinned to its voxel grid, and builds an lfx::Localizer from the two
files.  The files are the restatements' clouds (visibility, masked build, voxel filter) byte for byte, and the printed figures
their results."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import visibility_cases as VC
from tests import voxel_filter_restatement as VF
from tests.visibility_restatement import Rule, build_masked

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lidar_feature_extraction_amd", "_lib", "filter_map")
LEAVES = (0.2, 0.4)
E2E_BOUND = 0.06                              # tests/test_mapping_gpu.py: E2E_BOUND, its bound for a localisation


def test_filter_map_example_builds_without_a_gpu():
    assert os.path.exists(EXE), "examples/filter_map is built with the library (csrc/Makefile, CALLERS)"


@pytest.mark.gpu
@pytest.mark.parametrize("min_points", (1, 2))
def test_the_filtered_map_is_the_restatements(tmp_path, min_points):
    from lidar_feature_extraction_amd import read_pcd, write_pcd
    store, _ = VC.scene_case()
    rule = Rule(**VC.SCENE)
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    out.mkdir()
    with open(src / "poses.txt", "w") as f:
        for p in store.poses():
            f.write(" ".join("%.17g" % v for v in p.reshape(12)) + "\n")
    for k in range(len(store)):
        for kind, name in ((0, "edge"), (1, "surface")):
            write_pcd(str(src / ("%s_%d.pcd" % (name, k))), store.clouds[kind][k])
    c = rule.cfg
    args = ["%.9g" % LEAVES[0], "%.9g" % LEAVES[1], str(min_points), str(int(c.n_rows)), str(int(c.n_columns)), "%.9g" % c.elev_min,
            "%.9g" % c.elev_step, str(int(c.guard))]
    r = subprocess.run([EXE, str(src), str(out)] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    _, flags, res = rule.run(store)
    m = re.search(r"visibility: (\d+) edge and (\d+) surface records dynamic", r.stdout)
    assert m and tuple(int(v) for v in m.groups()) == tuple(res["n_dynamic"]) and min(res["n_dynamic"]) > 0
    for kind, name in ((0, "edge"), (1, "surface")):
        kept = build_masked(store, kind, flags[kind])[0]
        want, _, wres = VF.filtered(kept, LEAVES[kind], min_points)
        got = read_pcd(str(out / (name + ".pcd")))
        assert 0 < len(want) < len(kept)
        assert np.ascontiguousarray(got[:, :3]).tobytes() == np.ascontiguousarray(want[:, :3]).tobytes(), name
        m = re.search(r"%s: (\d+) records, (\d+) accumulated, (\d+) voxels, (\d+) written" % name, r.stdout)
        assert m and tuple(int(v) for v in m.groups()) == (res["n_records"][kind], wres["n_accumulated"], wres["n_voxels"], wres["n_written"])
    m = re.search(r"localised keyframe (\d+) against the filtered map: (success|no success), code (-?\d+), ([0-9.]+) m from its pose", r.stdout)
    assert m and int(m.group(1)) == len(store) // 2, r.stdout
    # the keyframe's own clouds against a map that holds them thinned, from the keyframe's own pose: it stays where it is
    assert m.group(2) == "success" and float(m.group(4)) < E2E_BOUND, r.stdout
