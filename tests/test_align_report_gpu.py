"""lfx_align_report on the device (lfx_*_report, lfx_odometry_reports) against tests/report_restatement.py.  The ground truth
is numpy fed with the rows that the EXISTING lfx_scan_to_map_residuals / lfx_edge_residuals produce at result.pose for the
same clouds and maps: the reduction, the weights, the projection, the eigen-solve and the covariance are all recomputed
outside the code under test.

Bounds (none of them from what the device gives): counts equal; the scalar sums to 1e-9 relative and H to 1e-9 in the
Frobenius norm -- both sides see the same rows, what is left is the order of ~10^4 additions (n * 2^-53 ~ 1e-12) and fused
against unfused products, while a real fault (a wrong weight, a row left out) shows in the third digit; eigenvalues to
1e-12 * the largest against numpy on the device's own H (the Jacobi stop is 2^-50 ~ 1e-15); the covariance to
1e3 * 2^-53 * cond(H) * |C|; and beside these, bit for bit, eigenvalues, eigenvectors, covariance and rank against the float64
restatement of the device's algorithm (tests/align_report_reference.py; the report's edges: tests/test_align_report_edges_gpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.align_report_reference import mismatches
from tests.report_restatement import FLOOR, covariance_from, restate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, MAX_ITER = 15, 20
IDENT = np.ascontiguousarray(np.hstack([np.eye(3), np.zeros((3, 1))]))


def _rotation(axis_angle):
    th = np.asarray(axis_angle, np.float64)
    k = np.linalg.norm(th)
    if k == 0:
        return np.eye(3)
    u = th / k
    Kx = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + np.sin(k) * Kx + (1 - np.cos(k)) * Kx @ Kx


def _pose(axis_angle, t):
    return np.ascontiguousarray(np.hstack([_rotation(axis_angle), np.asarray(t, np.float64).reshape(3, 1)]))


def _scene(rings, cols, seeds):
    from lidar_feature_extraction_amd import make_scan
    from oracle import binding as OB
    clouds = [make_scan(rings, cols, seed=s) for s in seeds]
    return clouds, [OB.extract(c, canonical_ties=False) for c in clouds]


def _dev():
    import torch
    return torch.device("cuda", 0)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _up(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype).copy()).to(_dev())


def _same_results(a, b):
    return a["pose"].tobytes() == b["pose"].tobytes() and (a["code"], a["iteration"]) == (b["code"], b["iteration"]) and \
        np.float64(a["error"]).tobytes() == np.float64(b["error"]).tobytes() and \
        np.float64(a["error_scale"]).tobytes() == np.float64(b["error_scale"]).tobytes()


def _rows_of_clouds(fx, emap, smap, pose, edge, surface):
    """The rows of one scan -- edge cloud and (already downsampled) surface cloud, [n][4] float32 on the host -- at `pose`,
    through lfx_scan_to_map_residuals."""
    import torch
    dev = _dev()
    out = []
    for kind, m, pts, width in ((0, emap, edge, 3), (1, smap, surface, 1)):
        n = len(pts)
        d_p = _up(np.vstack([pts, np.zeros((1, 4), np.float32)]))
        d_b, d_n = _up([0], np.int32), _up([n], np.int32)
        d_r = torch.zeros((n + 1, width), dtype=torch.float64, device=dev)
        d_j = torch.zeros((n + 1, 7 * width), dtype=torch.float64, device=dev)
        if n:
            fx.scan_to_map_residuals(kind, m, pose, K, d_p.data_ptr(), d_b.data_ptr(), d_n.data_ptr(), 1, 1, n, d_r.data_ptr(),
                                     d_j.data_ptr(), _stream())
        torch.cuda.synchronize()
        out += [d_r.cpu().numpy()[:n], d_j.cpu().numpy()[:n]]
    return out


def _check(rep, want, what, inliers=True):
    """One device report against the restatement of the same rows; prints each figure before it asserts."""
    assert rep["valid"], what
    H, Hw = rep["information"], want["information"]
    rel = lambda a, b: abs(a - b) / max(abs(b), 1e-300)   # noqa: E731
    figures = dict(
        error=rel(rep["error"], want["error"]), error_scale=rel(rep["error_scale"], want["error_scale"]),
        sigma2=rel(rep["sigma2"], want["sigma2"]), rms_edge=rel(rep["rms_edge"], want["rms_edge"]) if want["n_edge"] else 0.0,
        rms_surface=rel(rep["rms_surface"], want["rms_surface"]) if want["n_surface"] else 0.0,
        information=np.linalg.norm(H - Hw) / np.linalg.norm(Hw))
    lam = rep["eigenvalues"]
    lam_np = np.linalg.eigvalsh(H)
    figures["eigenvalues"] = np.abs(lam - lam_np).max() / lam[5]
    vec = rep["eigenvectors"]
    figures["eigenvectors"] = max(np.linalg.norm(H @ vec[k] - lam[k] * vec[k]) for k in range(6)) / lam[5]
    figures["orthonormal"] = np.abs(vec @ vec.T - np.eye(6)).max()
    _, _, cov_np, rank_np = covariance_from(H, rep["sigma2"])
    cond = lam_np[5] / max(lam_np[0], FLOOR * lam_np[5])
    cov_bound = 1e3 * 2.0 ** -53 * cond * np.linalg.norm(cov_np)
    figures["covariance / bound"] = np.linalg.norm(rep["covariance"] - cov_np) / cov_bound
    d_bound = 1e-9 * np.linalg.norm(want["D"])
    figures["min_eigenvalue_d / bound"] = abs(rep["min_eigenvalue_d"] - want["min_eigenvalue_d"]) / d_bound
    print(what, {k: float("%.3g" % v) for k, v in figures.items()}, "rank", rep["rank"], "degenerate", rep["degenerate"],
          "inliers", rep["n_edge_inliers"], rep["n_surface_inliers"], "of", rep["n_edge"], rep["n_surface"])
    assert (rep["n_edge"], rep["n_surface"], rep["n_surface_no_plane"]) == (want["n_edge"], want["n_surface"], want["n_surface_no_plane"]), what
    if inliers:
        assert not want["near_threshold"], what + ": an input with a residual at the Huber threshold (choose another seed)"
        assert (rep["n_edge_inliers"], rep["n_surface_inliers"]) == (want["n_edge_inliers"], want["n_surface_inliers"]), what
    for k in ("error", "error_scale", "sigma2", "rms_edge", "rms_surface", "information"):
        assert figures[k] <= 1e-9, (what, k, figures[k])
    assert figures["eigenvalues"] <= 1e-12 and figures["eigenvectors"] <= 1e-12 and figures["orthonormal"] <= 1e-12, (what, figures)
    assert np.all(np.diff(lam) >= 0), what
    for k in range(6):
        assert vec[k][np.argmax(np.abs(vec[k]))] > 0, (what, k)
    assert figures["covariance / bound"] <= 1.0, (what, figures)
    # and, stricter: eigenvalues, eigenvectors, covariance and rank are the bytes of the float64 restatement of the device's
    # algorithm on the record's own information and sigma2 (tests/align_report_reference.py)
    assert not mismatches(rep), (what, mismatches(rep))
    assert rep["covariance"].tobytes() == np.ascontiguousarray(rep["covariance"].T).tobytes(), what
    assert rep["information"].tobytes() == np.ascontiguousarray(rep["information"].T).tobytes(), what
    assert rep["rank"] == int((lam > FLOOR * lam[5]).sum()) == rank_np, what
    assert figures["min_eigenvalue_d / bound"] <= 1.0, (what, figures)
    assert abs(want["min_eigenvalue_d"] - 0.1) > d_bound, what + ": D's smallest eigenvalue sits on the threshold (choose another input)"
    assert rep["degenerate"] == (want["min_eigenvalue_d"] < 0.1), what


@pytest.mark.parametrize("cell", [1.0, 0.0])
@pytest.mark.parametrize("batch", [1, 4])
@pytest.mark.parametrize("rings,cols", [(16, 900), (64, 1800)])
def test_reports_of_a_batch_against_the_restatement(rings, cols, batch, cell):
    """lfx_localize_batch_report straight after extraction, maps from other scans of the scene, every scan from its own moved
    pose; both search routes.  Results: the plain call's bytes, before and after; reports: the same bytes twice, and the
    restatement's numbers from the rows lfx_edge_residuals / lfx_scan_to_map_residuals give at result.pose."""
    import torch
    from lidar_feature_extraction_amd import FeatureExtraction, concat
    rng = np.random.default_rng(31)
    clouds, _ = _scene(rings, cols, [7500 + s for s in range(batch)])
    _, maps = _scene(rings, cols, [7590, 7591, 7592])
    edge_map = np.ascontiguousarray(np.concatenate([m["edge_points"] for m in maps]), np.float32)
    surf_map = np.ascontiguousarray(np.concatenate([m["surface_points"] for m in maps]), np.float32)
    dev, stream = _dev(), _stream()
    fx = FeatureExtraction(device=0, max_points_per_scan=rings * cols, max_batch=batch, max_points_per_ring=cols, max_rings=rings)
    d = torch.from_numpy(concat(clouds).view(np.uint8).copy()).to(dev)
    fx.extract_batch_device(d.data_ptr(), [len(c) for c in clouds], stream)
    d_emap, d_smap = _up(edge_map), _up(surf_map)
    poses = np.stack([_pose(rng.normal(0, 0.004, 3), rng.normal(0, 0.03, 3)) for _ in range(batch)])
    emap, smap = fx.make_map(d_emap.data_ptr(), len(edge_map), cell, stream), fx.make_map(d_smap.data_ptr(), len(surf_map), cell, stream)
    before = fx.localize_batch(emap, smap, poses, K, MAX_ITER, 1.0, stream)
    res, reps = fx.localize_batch(emap, smap, poses, K, MAX_ITER, 1.0, stream, report=True)
    after = fx.localize_batch(emap, smap, poses, K, MAX_ITER, 1.0, stream)
    res2, reps2 = fx.localize_batch(emap, smap, poses, K, MAX_ITER, 1.0, stream, report=True)
    for s in range(batch):
        assert _same_results(res[s], before[s]) and _same_results(after[s], before[s]) and _same_results(res2[s], before[s]), s
        assert reps[s]["raw"] == reps2[s]["raw"], s
    # the rows at the returned poses, from the entry points that were there before
    total = sum(len(c) for c in clouds)
    view = fx.device_view()
    d_down = torch.zeros((total, 4), dtype=torch.float32, device=dev)
    d_dn, d_ds = torch.zeros(batch, dtype=torch.int32, device=dev), torch.zeros(batch, dtype=torch.int32, device=dev)
    fx.downsample_surface(1.0, d_down.data_ptr(), d_dn.data_ptr(), d_ds.data_ptr(), stream)
    d_res, d_jac = torch.zeros((total, 3), dtype=torch.float64, device=dev), torch.zeros((total, 21), dtype=torch.float64, device=dev)
    d_sres, d_sjac = torch.zeros(total, dtype=torch.float64, device=dev), torch.zeros((total, 7), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    dn = d_dn.cpu().numpy()
    begin = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    for s in range(batch):
        assert res[s]["code"] <= 3, (s, res[s])
        pose = res[s]["pose"]
        fx.edge_residuals(emap, pose, K, d_res.data_ptr(), d_jac.data_ptr(), stream)
        fx.scan_to_map_residuals(1, smap, pose, K, d_down.data_ptr(), view.scan_begin, d_dn.data_ptr(), 1, batch, rings * cols,
                                 d_sres.data_ptr(), d_sjac.data_ptr(), stream)
        torch.cuda.synchronize()
        ne = len(fx.download(s, stream).edge_points)
        b = int(begin[s])
        want = restate(pose, d_res[b:b + ne].cpu().numpy(), d_jac[b:b + ne].cpu().numpy(), d_sres[b:b + int(dn[s])].cpu().numpy(),
                       d_sjac[b:b + int(dn[s])].cpu().numpy())
        assert ne > 50 and dn[s] > 50
        _check(reps[s], want, "%d x %d, batch %d, cell %g, scan %d" % (rings, cols, batch, cell, s))
    fx.close()


def test_report_calls_in_a_row_leave_nothing_behind():
    """A report call between plain calls, with another batch size and far fewer iterations, changes nothing a later call
    gives (the launches' sizes, the iterations queued ahead and the scratch are all carried from call to call); and a scan's
    report does not depend on its neighbours in the batch: the same bytes alone and among four."""
    import torch
    from lidar_feature_extraction_amd import FeatureExtraction, concat, make_scan
    rng = np.random.default_rng(77)
    rings, cols = 32, 1024
    dev, stream = _dev(), _stream()
    _, maps = _scene(rings, cols, [7590, 7591, 7592])
    edge_map = np.ascontiguousarray(np.concatenate([m["edge_points"] for m in maps]), np.float32)
    surf_map = np.ascontiguousarray(np.concatenate([m["surface_points"] for m in maps]), np.float32)
    d_emap, d_smap = _up(edge_map), _up(surf_map)
    full = [make_scan(rings, cols, seed=7600 + s) for s in range(4)]
    small = full[0][:4 * cols].copy()
    poses = np.stack([_pose(rng.normal(0, 0.004, 3), rng.normal(0, 0.03, 3)) for _ in range(4)])
    fx = FeatureExtraction(device=0, max_points_per_scan=rings * cols, max_batch=4, max_points_per_ring=cols, max_rings=rings)
    emap, smap = fx.make_map(d_emap.data_ptr(), len(edge_map), 1.0, stream), fx.make_map(d_smap.data_ptr(), len(surf_map), 2.0, stream)

    def run(clouds, p, max_iter=20, report=False):
        d = torch.from_numpy(concat(clouds).view(np.uint8).copy()).to(dev)
        fx.extract_batch_device(d.data_ptr(), [len(c) for c in clouds], stream)
        return fx.localize_batch(emap, smap, p, K, max_iter, 1.0, stream, report=report)

    fresh = run([full[3]], poses[3:4])[0]
    assert fresh["iteration"] >= 2
    res4, rep4 = run(full, poses, report=True)
    run([small], poses[:1], max_iter=2, report=True)            # leaves short guesses behind
    again = run([full[3]], poses[3:4])[0]
    assert _same_results(fresh, again), (fresh, again)
    res1, rep1 = run([full[3]], poses[3:4], report=True)
    assert _same_results(res1[0], fresh) and _same_results(res4[3], fresh)
    assert rep1[0]["valid"] and rep1[0]["raw"] == rep4[3]["raw"]
    fx.close()


def _corridor(end_wall):
    """Walls y = +-3, floor z = -1.8 (not through the origin: such a plane has no X w = -1 form), x from -20 to 20; the map on
    a lattice of 0.2 m, the scan on another (0.25 m, shifted) and kept 0.75 m away from the corners so that the 15 nearest
    map points of every scan point lie in ONE plane; edge points on the two wall-floor lines.  Nothing constrains x unless
    there is an end wall at x = 20.  The scan's three kinds of residuals -- floor (0 at the start pose), walls (0.1 m), edge
    lines -- are 40 %, 47 % and 13 % of its rows: none is a majority, so the median and the MAD of the errors are the walls'
    and the robust scale is of their size (with more than half of the rows at exactly 0 the scale would be 0 and every other
    row would get a weight of 1e-7: exact coordinates have no noise to set a scale from)."""
    def plane(fixed_axis, value, u, v):
        g = np.stack(np.meshgrid(u, v, indexing="ij"), -1).reshape(-1, 2)
        p = np.zeros((len(g), 4), np.float32)
        free = [a for a in range(3) if a != fixed_axis]
        p[:, free[0]], p[:, free[1]], p[:, fixed_axis] = g[:, 0], g[:, 1], value
        return p
    xm, xs = np.arange(-20, 20.001, 0.2), np.arange(-19.43, 19.5, 0.25)
    smap = [plane(1, 3.0, xm, np.arange(-1.8, 1.201, 0.2)), plane(1, -3.0, xm, np.arange(-1.8, 1.201, 0.2)),
            plane(2, -1.8, xm, np.arange(-3, 3.001, 0.2))]
    sscan = [plane(1, 3.0, xs, np.arange(-1.03, 0.7, 0.25)), plane(1, -3.0, xs, np.arange(-1.03, 0.7, 0.25)),
             plane(2, -1.8, xs, np.arange(-1.46, 1.5, 0.25))]
    if end_wall:
        smap.append(plane(0, 20.0, np.arange(-3, 3.001, 0.2), np.arange(-1.8, 1.201, 0.2)))
        sscan.append(plane(0, 20.0, np.arange(-2.21, 2.25, 0.25), np.arange(-1.03, 0.7, 0.25)))

    def lines(x):
        p = np.zeros((2 * len(x), 4), np.float32)
        p[:, 0], p[:, 1], p[:, 2] = np.concatenate([x, x]), np.repeat([3.0, -3.0], len(x)), -1.8
        return p
    return lines(xm), np.concatenate(smap), lines(np.arange(-19.43, 19.5, 0.125)), np.concatenate(sscan)


def test_a_corridor_is_reported_as_one():
    """Nothing in a straight corridor says where along it the scan is: the update is refused (IsDegenerate), the stop code
    is LFX_ALIGN_CONVERGED all the same -- and the report says rank 5, degenerate, the unconstrained direction is the
    translation along x, and its standard deviation (the floor's) is orders above the one across.  With an end wall: rank 6."""
    from lidar_feature_extraction_amd import FeatureExtraction, covariance_ros
    fx = FeatureExtraction(device=0, max_points_per_scan=1024, max_batch=1)
    start = _pose([0, 0, 0], [0, 0.1, 0])
    for end_wall in (False, True):
        edge_map, surf_map, edge, surf = _corridor(end_wall)
        emap, smap = fx.make_map_from_host(edge_map, 1.0), fx.make_map_from_host(surf_map, 1.0)
        # (leaf 0.1, under the scan's spacing: every voxel holds one point.  A 1 m voxel at a corner would average wall and
        # floor points into a centroid in mid-air, whose neighbourhood spans both planes)
        res, rep = fx.localize_host(emap, smap, edge, surf, start, K, MAX_ITER, 0.1, report=True)
        plain = fx.localize_host(emap, smap, edge, surf, start, K, MAX_ITER, 0.1)
        assert _same_results(res, plain)
        assert rep["n_surface"] == len(surf)
        assert rep["valid"] and rep["n_surface_no_plane"] == 0 and rep["n_edge"] == len(edge), rep
        std = np.sqrt(np.diag(covariance_ros(res["pose"], rep["covariance"])))
        print("corridor, end wall", end_wall, "code", res["code"], "iteration", res["iteration"], "eigenvalues", rep["eigenvalues"],
              "std (x y z rx ry rz)", std, "min eigenvalue of D", rep["min_eigenvalue_d"])
        if end_wall:
            assert rep["rank"] == 6, rep["eigenvalues"]
            continue
        assert res["code"] == 0 and res["pose"].tobytes() == start.tobytes()      # the refused update reads as converged
        assert rep["rank"] == 5 and rep["degenerate"], rep["eigenvalues"]
        assert abs(rep["eigenvectors"][0][3]) >= 0.999, rep["eigenvectors"][0]
        assert std[0] >= 100.0 * std[1], std
        # by construction: sqrt(lambda_y / (1e-9 lambda_max)); the y direction is an eigenvector of its own up to the coupling
        # with the roll, so this is an order of magnitude, printed above and not asserted beyond the issue's 10^2
        emap.close()
        smap.close()
    fx.close()


def _all_zero(rep):
    return not rep["valid"] and rep["raw"] == bytes(len(rep["raw"]))


def test_nothing_to_report():
    """Empty clouds (LFX_ALIGN_EMPTY_INPUT) and a scan whose surface rows are all zero rows (LFX_ALIGN_NO_PLANE, a map plane
    through the origin): valid 0, every byte of the record 0, results as the plain call gives them."""
    from lidar_feature_extraction_amd import FeatureExtraction
    rng = np.random.default_rng(51)
    fx = FeatureExtraction(device=0, max_points_per_scan=1024, max_batch=1)
    plane = np.zeros((4000, 4), np.float32)
    plane[:, :2] = rng.uniform(-20, 20, (4000, 2))
    scan_surface = np.zeros((300, 4), np.float32)
    scan_surface[:, :2] = rng.uniform(-15, 15, (300, 2))
    scan_surface[:, 2] = 0.05
    none = np.zeros((0, 4), np.float32)
    emap, smap = fx.make_map_from_host(plane, 1.0), fx.make_map_from_host(plane, 1.0)
    for surface, leaf, code, max_iter in ((scan_surface, 1000.0, 5, 7), (none, 1.0, 4, 20)):
        res, rep = fx.localize_host(emap, smap, none, surface, IDENT, K, max_iter, leaf, report=True)
        plain = fx.localize_host(emap, smap, none, surface, IDENT, K, max_iter, leaf)
        assert (res["code"], res["iteration"], res["success"]) == (code, 0, False) and _same_results(res, plain), res
        assert _all_zero(rep), rep
    # and a scan with a report right after: the record is filled again
    plane[:, 2] = -2.0
    scan_surface[:, 2] = -1.95
    emap2, smap2 = fx.make_map_from_host(plane, 1.0), fx.make_map_from_host(plane, 1.0)
    res, rep = fx.localize_host(emap2, smap2, none, scan_surface, IDENT, K, 20, 0.5, report=True)
    assert res["code"] == 0 and rep["valid"] and rep["degenerate"] and rep["rank"] == 3 and rep["n_edge"] == 0, rep
    fx.close()


def test_odometry_reports():
    """Six scans of a moving sensor through one update_batch with reports on: six records, the first not valid (the scan was
    not aligned) and all zero, the others the restatement's on the window rebuilt from the store; poses and store are the
    bytes of a run with reports off."""
    import torch
    from lidar_feature_extraction_amd import FeatureExtraction, concat, make_sequence
    rings, cols, n = 16, 900, 6
    clouds, _ = make_sequence(n, rings, cols)
    dev, stream = _dev(), _stream()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def d2h(ptr, count):
        out = np.zeros((int(count), 4), np.float32)
        torch.cuda.synchronize()
        if count:
            assert hip.hipMemcpy(out.ctypes.data, int(ptr), out.nbytes, 2) == 0
        return out

    runs = {}
    for on in (False, True):
        fx = FeatureExtraction(device=0, max_points_per_scan=rings * cols, max_batch=n, max_points_per_ring=cols, max_rings=rings)
        odo = fx.odometry(reports=True) if on else fx.odometry()
        d = torch.from_numpy(concat(clouds).view(np.uint8).copy()).to(dev)
        fx.extract_batch_device(d.data_ptr(), [len(c) for c in clouds], stream)
        res = odo.update_batch(n, stream)
        view = odo.view()
        runs[on] = (res, d2h(view["edge_points"], view["n_edge"]), d2h(view["surface_points"], view["n_surface"]), view)
        if not on:
            assert odo.reports() == []
            odo.close()
            fx.close()
    (res0, edge0, surf0, _), (res, edge, surf, view) = runs[False], runs[True]
    for a, b in zip(res0, res):
        assert _same_results(a, b) and a["aligned"] == b["aligned"]
    assert edge0.tobytes() == edge.tobytes() and surf0.tobytes() == surf.tobytes()
    reps = odo.reports()
    assert len(reps) == n and _all_zero(reps[0]) and res[0]["code"] == 6
    eo, so = view["edge_offsets"], view["surface_offsets"]
    for k in range(1, n):
        assert res[k]["aligned"] and res[k]["code"] <= 3
        lo = max(0, k - 7)
        ew, sw = edge[eo[lo]:eo[k]], surf[so[lo]:so[k]]
        emap, smap = fx.make_map_from_host(ew, 1.0), fx.make_map_from_host(sw, 1.0)
        scan = fx.download(k, stream)
        down = _downsample_on_device(fx, scan.surface_points)
        want = restate(res[k]["pose"], *_rows_of_clouds(fx, emap, smap, res[k]["pose"], np.ascontiguousarray(scan.edge_points, np.float32), down))
        _check(reps[k], want, "odometry, scan %d" % k)
        emap.close()
        smap.close()
    # a single update: one record, of that scan
    scan = fx.download(n - 1, stream)
    one = odo.update_host(scan.edge_points, scan.surface_points)
    assert one["aligned"] and len(odo.reports()) == 1 and odo.reports()[0]["valid"]
    odo.set_reports(False)
    assert odo.reports() == []
    odo.close()
    fx.close()


def _downsample_on_device(fx, points):
    """Downsample(points, 1.0) by lfx_voxel_downsample (the entry point that was there before), back on the host."""
    import torch
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    n = len(pts)
    d_p, d_b, d_n = _up(np.vstack([pts, np.zeros((1, 4), np.float32)])), _up([0], np.int32), _up([n], np.int32)
    d_out = torch.zeros((n + 1, 4), dtype=torch.float32, device=_dev())
    d_on, d_os = torch.zeros(1, dtype=torch.int32, device=_dev()), torch.zeros(1, dtype=torch.int32, device=_dev())
    fx.voxel_downsample(d_p.data_ptr(), d_b.data_ptr(), d_n.data_ptr(), 1, 1, n, 1.0, d_out.data_ptr(), d_on.data_ptr(), d_os.data_ptr(),
                        _stream())
    torch.cuda.synchronize()
    assert int(d_os.cpu()[0]) == 0
    return np.ascontiguousarray(d_out.cpu().numpy()[:int(d_on.cpu()[0])])


LOCALIZE = os.path.join(ROOT, "lidar_feature_extraction_amd", "_lib", "localize_scan")


def test_the_cpp_header_gives_the_python_call_s_report(tmp_path):
    """include/lfx.hpp through a compiled caller (examples/localize_scan --report: lfx::Localizer::Update with a report,
    lfx::CovarianceRos): one scan, the report printed with 17 digits, the numbers of the Python call.  Without the flag the
    example prints what it printed before."""
    from lidar_feature_extraction_amd import FeatureExtraction, covariance_ros, make_scan
    rings, cols = 16, 900
    cloud = make_scan(rings, cols, seed=7700)
    _, maps = _scene(rings, cols, [7790, 7791])
    edge_map = np.ascontiguousarray(np.concatenate([m["edge_points"] for m in maps]), np.float32)
    surf_map = np.ascontiguousarray(np.concatenate([m["surface_points"] for m in maps]), np.float32)
    paths = [str(tmp_path / n) for n in ("edge_map.bin", "surface_map.bin", "scan.bin", "poses.bin")]
    edge_map.tofile(paths[0])
    surf_map.tofile(paths[1])
    cloud.tofile(paths[2])
    base = [LOCALIZE, paths[0], paths[1], paths[2], str(rings), str(cols), paths[3], "host"]
    r = subprocess.run(base + ["--report"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    with_report = open(paths[3], "rb").read()
    plain = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "report" not in plain.stdout and open(paths[3], "rb").read() == with_report
    assert [ln for ln in r.stdout.split("\n") if not ln.startswith("report:")] == plain.stdout.split("\n")
    line = [ln for ln in r.stdout.split("\n") if ln.startswith("report: std")]
    assert len(line) == 1, r.stdout
    w = line[0].split()
    std = np.array([float(x) for x in w[2:8]])
    assert w[8] == "rank" and w[10] == "degenerate" and w[12] == "inliers"
    fx = FeatureExtraction(device=0, max_points_per_scan=rings * cols, max_batch=1, max_points_per_ring=cols, max_rings=rings)
    fx.ExtractFeatures(cloud)
    emap, smap = fx.make_map_from_host(edge_map, 1.0), fx.make_map_from_host(surf_map, 1.0)
    initial = np.array([[1, 0, 0, 0.02], [0, 1, 0, -0.015], [0, 0, 1, 0.01]], np.float64)
    res, reps = fx.localize_batch(emap, smap, initial[None], K, MAX_ITER, 1.0, report=True)
    rep = reps[0]
    assert rep["valid"]
    assert np.frombuffer(with_report[:96], np.float64).tobytes() == res[0]["pose"].tobytes()
    want = np.sqrt(np.diag(covariance_ros(res[0]["pose"], rep["covariance"])))
    assert std.tobytes() == want.tobytes(), (std, want)
    assert (int(w[9]), int(w[11])) == (rep["rank"], int(rep["degenerate"]))
    assert float(w[13]) == rep["n_edge_inliers"] / rep["n_edge"] and float(w[14]) == rep["n_surface_inliers"] / rep["n_surface"]
    fx.close()
