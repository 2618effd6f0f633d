"""lfx::FeatureExtraction::ScanContext, lfx::PlaceDb and lfx::Localizer (include/lfx.hpp) in a C++ process of its own: the
compiled examples/relocalize_scan indexes the prototype's six keyframes, recognises a revisit and localises it from the
proposed pose.  The match and the pose must be what the Python binding gives, bit for bit."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import deskew_cases as K
from tests import scan_context_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lidar_feature_extraction_amd", "_lib", "relocalize_scan")
REC = np.dtype([("entry", "<u4"), ("shift", "<u4"), ("distance", "<f8"), ("yaw", "<f8"), ("pose", "<f8", 12), ("error", "<f8"),
                ("scale", "<f8"), ("iteration", "<i4"), ("code", "<i4")])


def test_relocalize_example_builds_without_a_gpu():
    assert os.path.exists(EXE), "examples/relocalize_scan is built with the library (csrc/Makefile, CALLERS)"


@pytest.mark.gpu
@pytest.mark.parametrize("visit", [5, 14], ids=["place1-37deg", "place3--128deg"])
def test_cpp_relocalisation_matches_the_binding(tmp_path, visit):
    from lidar_feature_extraction_amd import FeatureExtraction, concat
    keys = R.keyframes()
    cloud, place, yaw = R.revisits()[visit]
    src, scan, dst = str(tmp_path / "keyframes.bin"), str(tmp_path / "scan.bin"), str(tmp_path / "out.bin")
    concat(keys).tofile(src)
    cloud.tofile(scan)
    r = subprocess.run([EXE, src, str(len(keys)), scan, str(R.RINGS), str(R.COLS), dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(dst, REC)
    assert len(got) == 1
    got = got[0]
    fx = FeatureExtraction(device=0, max_points_per_scan=R.RINGS * R.COLS, max_batch=1, max_points_per_ring=R.COLS, max_rings=R.RINGS)
    db = fx.place_db(len(keys))
    features = []
    for c in keys:
        features.append(fx.ExtractFeatures(c))
        db.add(fx.scan_context(None, None, K.stream()), 1, K.stream())
        K.sync()                                 # (the next scan replaces the records the descriptor is made from)
    fx.ExtractFeatures(cloud)
    m = db.query(fx.scan_context(None, None, K.stream()), 1, 1, stream=K.stream())[0][0]
    assert (int(got["entry"]), int(got["shift"]), float(got["distance"]), float(got["yaw"])) == (m["entry"], m["shift"], m["distance"], m["yaw"])
    assert m["entry"] == place and R.yaw_error(m["yaw"], yaw) <= 2.0 * np.pi / 60
    f = features[place]
    emap, smap = fx.make_map_from_host(f.edge_points, 1.0, K.stream()), fx.make_map_from_host(f.surface_points, 1.0, K.stream())
    c, s = math.cos(m["yaw"]), math.sin(m["yaw"])
    want = fx.localize_batch(emap, smap, np.array([[c, -s, 0.0, 0.0, s, c, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]]), 15, 20, 1.0, K.stream())[0]
    assert got["pose"].tobytes() == want["pose"].tobytes(), (got["pose"], want["pose"])
    assert (int(got["iteration"]), int(got["code"])) == (want["iteration"], want["code"])
    assert got["error"] == want["error"] and got["scale"] == want["error_scale"]
    assert "recognised keyframe %d of %d: shift %d" % (place, len(keys), m["shift"]) in r.stdout, r.stdout
    assert np.linalg.norm(want["pose"][:, 3] - np.array([R.REVISIT_OFFSET[0], R.REVISIT_OFFSET[1], 0.0])) < 0.3
    emap.close()
    smap.close()
    db.close()
    fx.close()
