"""lfx::Mapper, lfx::Odometry and the file-built lfx::Localizer (include/lfx.hpp) in a C++ process of its own: the compiled
examples/build_map drives a sequence through extraction and odometry, maps the odometry poses with two mappers, saves
them, builds a localizer from the files and localizes every scan.  Files byte for byte and poses bit for bit equal what
the Python binding gives for the same steps."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "lidar_feature_extraction_amd", "_lib", "build_map")
REC = np.dtype([("odometry", "<f8", 12), ("pose", "<f8", 12), ("error", "<f8"), ("iteration", "<i4"), ("code", "<i4"),
                ("edge", "<i4"), ("surface", "<i4")])


@pytest.mark.gpu
def test_cpp_build_map_matches_the_binding(tmp_path):
    from lidar_feature_extraction_amd import FeatureExtraction, Mapper, ScanMap, concat, make_sequence
    rings, cols, n = 16, 900, 10
    clouds, _ = make_sequence(n, rings, cols, seed=9400, step=0.3, yaw_step_deg=1.0)
    src, out = str(tmp_path / "scans.bin"), str(tmp_path / "poses.bin")
    cdir, pdir = tmp_path / "cpp", tmp_path / "py"
    cdir.mkdir()
    pdir.mkdir()
    concat(clouds).tofile(src)
    r = subprocess.run([EXE, src, str(rings), str(cols), str(n), str(cdir), out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out, REC)
    assert len(got) == n
    fx = FeatureExtraction(device=0, max_points_per_scan=rings * cols, max_batch=1, max_points_per_ring=cols, max_rings=rings)
    odo = fx.odometry()
    em, sm = Mapper(fx), Mapper(fx)
    poses = []
    for s in range(n):
        fx.ExtractFeatures(clouds[s])
        poses.append(odo.update_batch(1)[0]["pose"])
        assert int(em.add_batch("edge", poses[-1])[0]) == got["edge"][s]
        assert int(sm.add_batch("surface", poses[-1])[0]) == got["surface"][s]
        assert got["odometry"][s].tobytes() == poses[-1].tobytes()
    assert em.save(str(pdir / "edge.pcd")) and sm.save(str(pdir / "surface.pcd"))
    for name in ("edge.pcd", "surface.pcd"):
        assert open(cdir / name, "rb").read() == open(pdir / name, "rb").read(), name
    emap, smap = ScanMap.from_pcd(fx, str(pdir / "edge.pcd")), ScanMap.from_pcd(fx, str(pdir / "surface.pcd"))
    for s in range(n):
        fx.ExtractFeatures(clouds[s])
        w = fx.localize_batch(emap, smap, poses[s], max_iter=40)[0]
        assert got["pose"][s].tobytes() == w["pose"].tobytes(), s
        assert (int(got["iteration"][s]), int(got["code"][s])) == (w["iteration"], w["code"]), s
    assert list(got["edge"]).count(0) >= 2
    assert "build_map: %d scans" % n in r.stdout
    emap.close(); smap.close(); em.close(); sm.close(); odo.close(); fx.close()
