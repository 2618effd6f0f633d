"""lfx::FeatureExtraction / lfx::Odometry::UpdateBatchDeskewed (include/lfx.hpp) in a C++ process of its own: the compiled
examples/deskew_scans feeds sweeps of a moving sensor scan by scan to a plain odometry and to a de-skewing one.  Both must
give what the Python binding gives, bit for bit, and the example prints both trajectories."""
import os
import subprocess

import numpy as np
import pytest

from tests import deskew_cases as K
from tests import deskew_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lidar_feature_extraction_amd", "_lib", "deskew_scans")
REC = np.dtype([("pose", "<f8", 12), ("error", "<f8"), ("scale", "<f8"), ("iteration", "<i4"), ("code", "<i4"), ("aligned", "<i4")])


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", [1.0, 0.9])
def test_cpp_deskewed_odometry_matches_the_binding(tmp_path, ratio):
    from lidar_feature_extraction_amd import FeatureExtraction, concat, make_sweep
    rings, cols, n = 16, 900, 6
    motion = R.pose([0.002, -0.003, 0.02], [0.3, 0.02, -0.005])
    legs = K.arc(R.pose([0.0, 0.0, 0.2], [-1.0, -1.5, 1.8]), motion, n)
    clouds = [make_sweep(rings, cols, seed=9950 + i, pose0=p, motion=motion)[0] for i, (p, _) in enumerate(legs)]
    src, dst = str(tmp_path / "scans.bin"), str(tmp_path / "poses.bin")
    concat(clouds).tofile(src)
    r = subprocess.run([EXE, src, str(rings), str(cols), str(n), dst, repr(ratio)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(dst, REC)
    assert len(got) == 2 * n
    plain, deskewed = got[0::2], got[1::2]
    fx = FeatureExtraction(device=0, max_points_per_scan=rings * cols, max_batch=1, max_points_per_ring=cols, max_rings=rings)
    a, b = fx.odometry(), fx.odometry()
    lines = r.stdout.splitlines()
    for s in range(n):
        fx.ExtractFeatures(clouds[s])
        wa = a.update_batch(1)[0]
        wb = b.update_batch_deskewed(None, None, ratio, "end", 1)[0]
        for g, w in ((plain[s], wa), (deskewed[s], wb)):
            assert g["pose"].tobytes() == w["pose"].tobytes(), (s, g, w)
            assert (int(g["iteration"]), int(g["code"]), bool(g["aligned"])) == (w["iteration"], w["code"], w["aligned"]), (s, g, w)
        want = "%4u   %9.4f %9.4f %9.4f   %9.4f %9.4f %9.4f" % ((s,) + tuple(wa["pose"][:, 3]) + tuple(wb["pose"][:, 3]))
        assert want in lines, (want, r.stdout)
    assert not deskewed[0]["aligned"] and all(deskewed["aligned"][1:])
    # from the third scan on the prediction is a motion: the two odometries no longer see the same clouds
    assert deskewed[-1]["pose"].tobytes() != plain[-1]["pose"].tobytes()
    assert "deskew: %d scans" % n in r.stdout
    a.close()
    b.close()
    fx.close()
