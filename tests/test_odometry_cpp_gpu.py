"""lfx::Odometry (include/lfx.hpp) in a C++ process of its own: the compiled examples/odometry_scans feeds a moving sequence
scan by scan to one odometry through Update() (the extraction's device clouds) and to another through Update(host clouds),
as the reference's OdometrySubscriber would receive them.  Both must give what the Python binding gives, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lidar_feature_extraction_amd", "_lib", "odometry_scans")
REC = np.dtype([("pose", "<f8", 12), ("error", "<f8"), ("scale", "<f8"), ("iteration", "<i4"), ("code", "<i4"), ("aligned", "<i4")])


@pytest.mark.gpu
def test_cpp_odometry_matches_the_binding(tmp_path):
    from lidar_feature_extraction_amd import FeatureExtraction, concat, make_sequence
    rings, cols, n = 16, 900, 6
    clouds, truth = make_sequence(n, rings, cols, seed=8800)
    src, dst = str(tmp_path / "scans.bin"), str(tmp_path / "poses.bin")
    concat(clouds).tofile(src)
    r = subprocess.run([EXE, src, str(rings), str(cols), str(n), dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(dst, REC)
    assert len(got) == 2 * n
    device, host = got[0::2], got[1::2]
    fx = FeatureExtraction(device=0, max_points_per_scan=rings * cols, max_batch=1, max_points_per_ring=cols, max_rings=rings)
    odo = fx.odometry()
    for s in range(n):
        fx.ExtractFeatures(clouds[s])
        w = odo.update_batch(1)[0]
        for g in (device[s], host[s]):
            assert g["pose"].tobytes() == w["pose"].tobytes(), (s, g, w)
            assert (int(g["iteration"]), int(g["code"]), bool(g["aligned"])) == (w["iteration"], w["code"], w["aligned"]), (s, g, w)
    assert not device[0]["aligned"] and all(device["aligned"][1:])
    assert np.abs(device[-1]["pose"].reshape(3, 4)[:, 3] - truth[-1][:, 3]).max() < 0.06
    assert "odometry: %d scans" % n in r.stdout
    odo.close()
    fx.close()
