"""lfx::Visibility and lfx::Keyframes::BuildMasked (include/lfx.hpp) in a C++ process of its own: the compiled
examples/clean_map reads the scene of tests/visibility_cases.py from PCD files, votes, and writes the map of each kind without
the records flagged DYNAMIC.  Its two files are the restatement's masked clouds, byte for byte, and its printed figures the
restatement's result."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import visibility_cases as VC
from tests.visibility_restatement import Rule, build_masked

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lidar_feature_extraction_amd", "_lib", "clean_map")


def test_clean_map_example_builds_without_a_gpu():
    assert os.path.exists(EXE), "examples/clean_map is built with the library (csrc/Makefile, CALLERS)"


@pytest.mark.gpu
def test_the_cleaned_map_is_the_restatements(tmp_path):
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
            assert (store.clouds[kind][k][:, 3] == 1.0).all()          # what a PCD file of x y z reads back as
            write_pcd(str(src / ("%s_%d.pcd" % (name, k))), store.clouds[kind][k])
    c = rule.cfg
    args = [str(int(c.n_rows)), str(int(c.n_columns)), "%.9g" % c.elev_min, "%.9g" % c.elev_step, str(int(c.guard))]
    r = subprocess.run([EXE, str(src), str(out)] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    _, flags, res = rule.run(store)
    m = re.search(r"visibility: (\d+) pairs in (\d+) chunk\(s\), images (\d+) of (\d+) cells occupied", r.stdout)
    assert m and tuple(int(v) for v in m.groups()) == (res["n_pairs"], 1, res["occupied_cells"], res["total_cells"])
    for kind, name in ((0, "edge"), (1, "surface")):
        m = re.search(r"%s: (\d+) records, (\d+) voted on, (\d+) dynamic" % name, r.stdout)
        assert m and tuple(int(v) for v in m.groups()) == (res["n_records"][kind], res["n_voted"][kind], res["n_dynamic"][kind])
        want = build_masked(store, kind, flags[kind])[0]
        got = read_pcd(str(out / (name + ".pcd")))
        assert res["n_dynamic"][kind] > 0 and len(want) == res["n_records"][kind] - res["n_dynamic"][kind]
        assert np.ascontiguousarray(got[:, :3]).tobytes() == np.ascontiguousarray(want[:, :3]).tobytes()
