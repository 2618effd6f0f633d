"""lfx::Keyframes::ReserveFlags / Flags / FlagsInfo / SubmapMasked (include/lfx.hpp) in a C++ process of its own: the compiled
examples/clean_closer reads the scene of tests/visibility_cases.py from PCD files, lets lfx::Visibility vote into the store's
own flags and writes the masked submap around one keyframe.  Its printed result records and checksums are the Python
binding's over the same files."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import deskew_cases as K
from tests import visibility_cases as VC
from tests.visibility_restatement import Rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lidar_feature_extraction_amd", "_lib", "clean_closer")


def fnv1a(data):
    h = 14695981039346656037
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_clean_closer_example_builds_without_a_gpu():
    assert os.path.exists(EXE), "examples/clean_closer is built with the library (csrc/Makefile, CALLERS)"
    assert fnv1a(b"") == 0xCBF29CE484222325 and fnv1a(b"a") == 0xAF63DC4C8601EC8C          # the published test vectors


@pytest.mark.gpu
def test_the_masked_submap_is_the_bindings(tmp_path):
    from lidar_feature_extraction_amd import write_pcd
    store, _ = VC.scene_case()
    rule = Rule(**VC.SCENE)
    src = tmp_path / "in"
    src.mkdir()
    with open(src / "poses.txt", "w") as f:
        for p in store.poses():
            f.write(" ".join("%.17g" % v for v in p.reshape(12)) + "\n")
    for k in range(len(store)):
        for kind, name in ((0, "edge"), (1, "surface")):
            assert (store.clouds[kind][k][:, 3] == 1.0).all()          # what a PCD file of x y z reads back as
            write_pcd(str(src / ("%s_%d.pcd" % (name, k))), store.clouds[kind][k])
    c = rule.cfg
    center_id, radius = 2, 0.75                                        # (the keyframes are 0.5 m apart: 1, 2 and 3)
    args = [str(center_id), "%.17g" % radius, str(int(c.n_rows)), str(int(c.n_columns)), "%.9g" % c.elev_min, "%.9g" % c.elev_step, str(int(c.guard))]
    r = subprocess.run([EXE, str(src)] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    # the same through the Python binding
    fx = K.fx_for(16, 64, 1)
    kf = fx.keyframes(len(store), tuple(int(store.begin(kind)[-1]) for kind in (0, 1)))
    for k in range(len(store)):
        kf.add_host(store.clouds[0][k], store.clouds[1][k], store.pose[k], K.stream())
    kf.reserve_flags(K.stream())
    vis = fx.visibility(len(store), len(store), **rule.fields())
    _, _, res = vis.run(kf, flags=kf.flags(K.stream()), stream=K.stream())
    n = kf.info()["n_points"]
    m = re.search(r"flags: (\d+) of (\d+) edge and (\d+) of (\d+) surface records", r.stdout)
    assert m and tuple(int(v) for v in m.groups()) == (res["n_dynamic"][0], n[0], res["n_dynamic"][1], n[1]) and res["n_dynamic"][0] > 0
    selected = int(store.select(store.poses()[center_id, :, 3], radius).sum())
    assert 0 < selected < len(store)
    for kind, name in ((0, "edge"), (1, "surface")):
        cloud, s = kf.submap_masked(kind, store.poses()[center_id, :, 3], radius, stream=K.stream())
        K.sync()
        m = re.search(r"%s: selected (\d+) written (\d+) points (\d+) first (\d+) last (\d+) truncated (\d) checksum ([0-9a-f]{16})" % name, r.stdout)
        assert m, r.stdout
        assert tuple(int(v) for v in m.groups()[:6]) == (s["n_selected"], s["n_written_keyframes"], s["n_points"], s["first_id"], s["last_id"], int(s["truncated"]))
        assert s["n_selected"] == selected and s["n_points"] > 0
        assert int(m.group(7), 16) == fnv1a(cloud.cpu().numpy().tobytes())
    vis.close()
    kf.close()
    fx.close()
