"""Test-side restatement of the reference's odometry (no GPU): RecentScans (recent_scans.hpp:56-88), EdgeSurfaceMap
(edge_surface_map.hpp:38-76), Odometry (odometry.hpp:43-71) and TransformPointCloud (pcl_utils.hpp:76-83 ->
pcl::transformPointCloud with an Affine3d: PCL's generic Transformer<double>, every coordinate ((r0*x + r1*y) + r2*z) + t in
double rounded once to float, the other fields copied).  tests/test_odometry_reference.py pins it with the reference's own
vectors (tests/golden/odometry_vectors.json); tests/test_odometry_gpu.py holds the device to it.  The full CPU chain --
extract -> Downsample -> Optimizer::Run against the window -- is composed from the oracle's entry points."""
import ctypes as C

import numpy as np

PD, PF = C.POINTER(C.c_double), C.POINTER(C.c_float)


def transform(pose, cloud):
    """pcl::transformPointCloud(cloud, out, Affine3d(pose)): records of 4 floats, the 4th copied."""
    P = np.asarray(pose, np.float64).reshape(3, 4)
    c = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)
    x, y, z = (c[:, a].astype(np.float64) for a in range(3))
    out = c.copy()
    for r in range(3):
        out[:, r] = (((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3]).astype(np.float32)
    return out


class RecentScans:
    def __init__(self):
        self.scans = []

    def add(self, pose, scan):
        self.scans.append(transform(pose, scan))

    def is_empty(self):
        return len(self.scans) == 0

    def get_recent(self, n):
        recent = self.scans[len(self.scans) - min(n, len(self.scans)):]
        return np.concatenate(recent) if recent else np.zeros((0, 4), np.float32)    # MergeClouds: oldest first

    def get_all(self):
        return self.get_recent(len(self.scans))


class EdgeSurfaceMap:
    def __init__(self, n_local_scans):
        self.n = n_local_scans
        self.edge, self.surface = RecentScans(), RecentScans()

    def is_empty(self):
        return self.edge.is_empty() and self.surface.is_empty()

    def add(self, pose, scan):
        self.edge.add(pose, scan[0])
        self.surface.add(pose, scan[1])

    def get_recent(self):
        return self.edge.get_recent(self.n), self.surface.get_recent(self.n)


class Odometry:
    """Odometry<PoseUpdaterClass, MapClass, ScanType>: updater(recent_map) is a callable (scan, pose) -> pose."""

    def __init__(self, updater, map_, initial_pose=None):
        self.updater, self.map = updater, map_
        self.pose = np.eye(4)[:3].copy() if initial_pose is None else np.asarray(initial_pose, np.float64).reshape(3, 4).copy()

    def update(self, scan):
        if self.map.is_empty():
            self.map.add(self.pose, scan)
            return
        update = self.updater(self.map.get_recent())
        self.pose = update(scan, self.pose)
        self.map.add(self.pose, scan)


def downsample(points, leaf):
    """Downsample (downsample.hpp:37-51) by the oracle; a cloud PCL hands back unfiltered comes back as it is."""
    from oracle import binding as OB
    pts = np.ascontiguousarray(points, np.float32)
    out, n_out = np.zeros_like(pts), C.c_int(0)
    rc = OB.lib().orc_voxel_downsample(OB.ptr(pts, PF), len(pts), C.c_float(leaf), OB.ptr(out, PF), C.byref(n_out))
    return pts.copy() if rc else np.ascontiguousarray(out[:n_out.value])


def optimize_scan(edge_map, surf_map, k, edge, surf_down, pose, max_iter):
    """Optimizer<LOAMOptimizationProblem>::Run by the oracle (as tests/test_align_gpu.py calls it)."""
    from oracle import binding as OB
    edge_map, surf_map, edge, surf_down = (np.ascontiguousarray(a, np.float32) for a in (edge_map, surf_map, edge, surf_down))
    pose = np.ascontiguousarray(pose, np.float64)
    out, err, scale, it, code = np.zeros(12), C.c_double(), C.c_double(), C.c_int(), C.c_int()
    ok = OB.lib().orc_loc_optimize_scan(OB.ptr(edge_map, PF), len(edge_map), OB.ptr(surf_map, PF), len(surf_map), k,
                                        OB.ptr(edge, PF), len(edge), OB.ptr(surf_down, PF), len(surf_down), OB.ptr(pose, PD),
                                        max_iter, OB.ptr(out, PD), C.byref(err), C.byref(scale), C.byref(it), C.byref(code))
    return dict(pose=out.reshape(3, 4), error=err.value, error_scale=scale.value, iteration=it.value, code=code.value, success=bool(ok))


def oracle_chain(clouds, n_local_scans=7, k=15, max_iter=20, leaf=1.0):
    """The whole chain on the CPU: extract every scan, then Odometry with the problem Localizer::Update runs (window maps
    under k points: not aligned, as the library defines it).  Returns the poses after every scan."""
    from oracle import binding as OB

    def updater(recent):
        def run(scan, pose):
            if len(recent[0]) < k or len(recent[1]) < k:
                return pose
            return optimize_scan(recent[0], recent[1], k, scan[0], downsample(scan[1], leaf), pose, max_iter)["pose"]
        return run
    odo = Odometry(updater, EdgeSurfaceMap(n_local_scans))
    poses = []
    for cloud in clouds:
        f = OB.extract(cloud, canonical_ties=False)
        odo.update((f["edge_points"], f["surface_points"]))
        poses.append(odo.pose.copy())
    return np.stack(poses)


def trajectory_error(poses, truth):
    """Largest translation error (m) and largest rotation error (rad) over a trajectory."""
    dt = max(float(np.linalg.norm(p[:, 3] - t[:, 3])) for p, t in zip(poses, truth))
    dr = 0.0
    for p, t in zip(poses, truth):
        R = p[:, :3] @ t[:, :3].T
        dr = max(dr, float(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))))
    return dt, dr
