"""lfx::RollingMap (include/lfx.hpp) in a C++ process of its own: the compiled examples/rolling_map_scans feeds a moving
sequence scan by scan to an lfx::Odometry and hands its poses to an lfx::RollingMap.  Both trajectories must equal what the
Python binding gives on the same sequence, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lidar_feature_extraction_amd", "_lib", "rolling_map_scans")
REC = np.dtype([("pose", "<f8", 12), ("error", "<f8"), ("scale", "<f8"), ("iteration", "<i4"), ("code", "<i4"), ("aligned", "<i4")])


def test_rolling_map_example_builds_without_a_gpu():
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()
    assert os.access(EXE, os.X_OK)


@pytest.mark.gpu
def test_cpp_rolling_map_matches_the_binding(tmp_path):
    from lidar_feature_extraction_amd import FeatureExtraction, concat, make_sequence
    rings, cols, n = 16, 900, 6
    clouds, truth = make_sequence(n, rings, cols, seed=8800)
    src, dst = str(tmp_path / "scans.bin"), str(tmp_path / "poses.bin")
    concat(clouds).tofile(src)
    r = subprocess.run([EXE, src, str(rings), str(cols), str(n), dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(dst, REC)
    assert len(got) == 2 * n
    odometry, mapped = got[0::2], got[1::2]
    fx = FeatureExtraction(device=0, max_points_per_scan=rings * cols, max_batch=1, max_points_per_ring=cols, max_rings=rings)
    odo, rm = fx.odometry(), fx.rolling_map()
    for s in range(n):
        fx.ExtractFeatures(clouds[s])
        o = odo.update_batch(1)[0]
        m = rm.update_batch(o["pose"][None], 1)[0]
        for g, w in ((odometry[s], o), (mapped[s], m)):
            assert g["pose"].tobytes() == w["pose"].tobytes(), (s, g, w)
            assert (int(g["iteration"]), int(g["code"]), bool(g["aligned"])) == (w["iteration"], w["code"], w["aligned"]), (s, g, w)
        line = r.stdout.splitlines()[s]
        p = rm.pose()[:, 3]
        assert line.startswith("scan %d: " % s) and "map t = (%.4f, %.4f, %.4f)" % tuple(p) in line, line
    assert not mapped[0]["aligned"] and all(mapped["aligned"][1:])
    assert "rolling map: %d scans" % n in r.stdout
    odo.close()
    rm.close()
    fx.close()
