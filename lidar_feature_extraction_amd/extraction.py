"""Host-side mirror of the reference's extraction node for tests, the bench and Python users.

The reference operator is the body of FeatureExtraction::Callback
(/root/reference/extraction/app/feature_extraction.cpp:114-157); its construction reads the
nine HyperParameters (hyper_parameter.hpp:32-65).  `FeatureExtraction` here keeps those names:
construct with HyperParameters, call ExtractFeatures(cloud) per scan.  Everything runs in the
HIP library through the C ABI (binding.py); nothing is computed in Python.
"""
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import binding as B
from .synth import POINT_DTYPE

LABEL_NAMES = ["Default", "Edge", "EdgeNeighbor", "Surface", "SurfaceNeighbor", "OutOfRange",
               "Occluded", "ParallelBeam"]          # point_label.hpp:32-42
RING_STATUS_NAMES = {0: "ok", 1: "sparse", 2: "too_few_for_convolution", 3: "too_few_for_blocks",
                     4: "block_too_small", 5: "zero_norm_pair", 7: "too_large"}


@dataclass
class HyperParameters:
    """hyper_parameter.hpp:35-43 (code defaults)."""
    padding: int = 5
    neighbor_degree_threshold: float = 2.0
    distance_diff_threshold: float = 0.3
    parallel_beam_min_range_ratio: float = 0.02
    edge_threshold: float = 0.05
    surface_threshold: float = 0.05
    min_range: float = 0.1
    max_range: float = 100.0
    n_blocks: int = 6

    @staticmethod
    def launch_yaml():
        """lidar_feature_launch/config/lidar_feature_extraction.param.yaml:3-10"""
        return HyperParameters(padding=2, neighbor_degree_threshold=3.0, edge_threshold=50.0, max_range=1000.0)

    def to_c(self):
        return B.Params(self.padding, self.neighbor_degree_threshold, self.distance_diff_threshold,
                        self.parallel_beam_min_range_ratio, self.edge_threshold, self.surface_threshold,
                        self.min_range, self.max_range, self.n_blocks)


@dataclass
class ScanFeatures:
    labels: np.ndarray          # u8 [n], original point order
    curvature: np.ndarray       # f64 [n], original point order
    sorted_index: np.ndarray    # u32 [n], rings ascending / angle ascending
    ring_id: np.ndarray
    ring_count: np.ndarray
    ring_offset: np.ndarray
    ring_status: np.ndarray
    edge_points: np.ndarray     # f32 [n_edge,4]: x y z (float)curvature
    edge_index: np.ndarray      # u32 [n_edge] original indices
    surface_points: np.ndarray
    surface_index: np.ndarray

    @property
    def edge_xyz(self):
        """what the node publishes on scan_edge (ToPointXYZ, feature_extraction.cpp:163)"""
        return self.edge_points[:, :3]

    @property
    def surface_xyz(self):
        return self.surface_points[:, :3]


def _np(ptr, n, dtype, shape=None):
    if n == 0 or not ptr:                  # (a NULL pointer: that output was not asked for, lfx_config.outputs)
        return np.zeros((0,) + tuple(shape[1:]) if shape else 0, dtype)
    a = np.ctypeslib.as_array(ptr, shape=(n,) if shape is None else shape).astype(dtype, copy=True)
    return a


def _result(r):
    ne, ns, n, nr = r.n_edge, r.n_surface, r.n_points, r.n_rings
    return ScanFeatures(
        labels=_np(r.labels, n, np.uint8), curvature=_np(r.curvature, n, np.float64),
        sorted_index=_np(r.sorted_index, r.n_sorted, np.uint32),
        ring_id=_np(r.ring_id, nr, np.uint16), ring_count=_np(r.ring_count, nr, np.uint32),
        ring_offset=_np(r.ring_offset, nr, np.uint32), ring_status=_np(r.ring_status, nr, np.uint8),
        edge_points=_np(r.edge_points, ne, np.float32, (ne, 4)) if ne else np.zeros((0, 4), np.float32),
        edge_index=_np(r.edge_index, ne, np.uint32),
        surface_points=_np(r.surface_points, ns, np.float32, (ns, 4)) if ns else np.zeros((0, 4), np.float32),
        surface_index=_np(r.surface_index, ns, np.uint32))


class FeatureExtraction:
    """One context = one GPU = one calling thread (feature_extraction.cpp:65-87,185)."""

    def __init__(self, params=None, device=0, max_points_per_scan=262144, max_batch=1,
                 max_points_per_ring=0, max_rings=0, drop_zero_points=False, layout=None, outputs=0, stream_hint=0, test_hooks=None,
                 ring_ids=None):
        # max_points_per_ring: 0 = B.MAX_RING_POINTS; up to B.MAX_LONG_RING_POINTS (and max_points_per_scan).  Above
        # B.MAX_RING_POINTS longer rings run in the long-ring kernel (HBM workspace); the ring-major arrays then take
        # max_batch * max_rings * capacity * 45 bytes: give max_rings (0 reserves 256 rings)
        # test_hooks: the context comes from the test-hooks build of the library (B.HOOKS_LIB_PATH), the only one whose
        # lfx_create reads the LFX_DEBUG_* switches (tests and tools/ only).  None: that build exactly when such a switch is
        # set in the environment -- the shipped library would not see it
        if test_hooks is None:
            test_hooks = any(k.startswith("LFX_DEBUG_") for k in os.environ)
        self._L = B.load(bool(test_hooks))
        self.params = params or HyperParameters()
        self._ctx = C.c_void_p()
        # layout: (point_step, off_x, off_y, off_z, off_ring[, ring_datatype, big_endian]) of the records or a
        # B.Layout (layout_from_fields), None = PointXYZIR
        if layout is None:
            lay = B.Layout(0, 0, 0, 0, 0, 0, 0)
        elif isinstance(layout, B.Layout):
            lay = layout
        else:
            lay = B.Layout(*(tuple(layout) + (0, 0))[:7])
        self._step = lay.point_step or 32
        # outputs: B.OUT_* mask of what ExtractFeatures / extract_batch bring back (0 = everything); the two clouds always do
        # stream_hint: B.STREAM_* (what the caller knows about the order its driver publishes in; spares the first batch a slower route)
        # ring_ids: the sensor's ring ids where they are not 0 .. max_rings-1 (lfx_config.ring_ids); None: the host entry points
        # look them up in a scan that carries another id
        ids = None if ring_ids is None else (C.c_uint16 * len(ring_ids))(*[int(r) for r in ring_ids])
        cfg = B.Config(C.sizeof(B.Config), max_points_per_scan, max_batch, max_points_per_ring, max_rings, int(bool(drop_zero_points)), lay,
                       int(outputs), int(stream_hint), ids, 0 if ids is None else len(ring_ids))
        self._pinned = []
        cp = self.params.to_c()
        rc = self._L.lfx_create(C.byref(self._ctx), device, C.byref(cp), C.byref(cfg))
        if rc != 0:
            self._ctx = C.c_void_p()
            raise B.LfxError(rc, (self._L.lfx_last_error(None) or b"").decode())
        self.max_batch = max_batch
        self.max_points_per_scan = max_points_per_scan
        self.device = device

    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            for ptr in getattr(self, "_pinned", []):
                self._L.lfx_host_free(self._ctx, ptr)
            self._pinned = []
            self._L.lfx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- the operator ------------------------------------------------------------------
    def ExtractFeatures(self, cloud):
        """cloud: POINT_DTYPE array (PointXYZIR records).  Returns ScanFeatures."""
        return self.extract_batch([cloud])[0]

    def extract_batch(self, clouds):
        clouds = [np.ascontiguousarray(c) for c in clouds]
        for c in clouds:
            if c.dtype.itemsize != self._step:
                raise TypeError("clouds must be arrays of %d-byte records (POINT_DTYPE for PointXYZIR)" % self._step)
        nb = len(clouds)
        ptrs = (C.c_void_p * nb)(*[c.ctypes.data for c in clouds])
        ns = (C.c_size_t * nb)(*[len(c) for c in clouds])
        res = (B.ScanResult * nb)()
        B.check(self._ctx, self._L.lfx_extract_batch(self._ctx, ptrs, ns, nb, res), self._L)
        return [_result(res[i]) for i in range(nb)]

    def submit(self, cloud):
        """lfx_extract_submit: queue one scan (upload, kernels, download) and return its ticket at once; at most two
        tickets may be outstanding.  A pinned `cloud` (pinned_like) must stay untouched until wait(ticket) returns."""
        cloud = np.ascontiguousarray(cloud)
        if cloud.dtype.itemsize != self._step:
            raise TypeError("clouds must be arrays of %d-byte records (POINT_DTYPE for PointXYZIR)" % self._step)
        t = C.c_uint64(0)
        B.check(self._ctx, self._L.lfx_extract_submit(self._ctx, C.c_void_p(cloud.ctypes.data), len(cloud), C.byref(t)), self._L)
        return int(t.value)

    def wait(self, ticket, raw=False):
        """lfx_extract_wait: the ScanFeatures of that ticket (raw=True: the ctypes result, nothing copied)."""
        res = B.ScanResult()
        B.check(self._ctx, self._L.lfx_extract_wait(self._ctx, C.c_uint64(int(ticket)), C.byref(res)), self._L)
        return res if raw else _result(res)

    def pinned_like(self, cloud):
        """A copy of `cloud` in pinned host memory (lfx_host_alloc): lfx_extract reads such a buffer by DMA instead of
        staging it.  Owned by this object (freed by close())."""
        cloud = np.ascontiguousarray(cloud)
        ptr = C.c_void_p()
        B.check(self._ctx, self._L.lfx_host_alloc(self._ctx, max(cloud.nbytes, 1), C.byref(ptr)), self._L)
        self._pinned.append(ptr)
        buf = (C.c_uint8 * cloud.nbytes).from_address(ptr.value)
        out = np.frombuffer(buf, dtype=cloud.dtype, count=len(cloud))
        out[...] = cloud
        return out

    def voxel_downsample(self, d_points, d_begin, d_count, count_stride, n_clouds, total_points, leaf, d_out, d_out_count,
                         d_status, stream=0):
        """lfx_voxel_downsample: Downsample (pcl::VoxelGrid, downsample.hpp:37-51) of device clouds; all pointers are device addresses."""
        B.check(self._ctx, self._L.lfx_voxel_downsample(
            self._ctx, C.c_void_p(int(d_points)), C.c_void_p(int(d_begin)), C.c_void_p(int(d_count)), int(count_stride),
            int(n_clouds), int(total_points), float(leaf), C.c_void_p(int(d_out)), C.c_void_p(int(d_out_count)),
            C.c_void_p(int(d_status)), C.c_void_p(int(stream))))

    def downsample_surface(self, leaf, d_out, d_out_count, d_status, stream=0):
        """lfx_downsample_surface: the surface clouds of the last device batch, as the localizer downsamples them (surface.hpp:111)."""
        B.check(self._ctx, self._L.lfx_downsample_surface(
            self._ctx, float(leaf), C.c_void_p(int(d_out)), C.c_void_p(int(d_out_count)), C.c_void_p(int(d_status)),
            C.c_void_p(int(stream))))

    def make_map(self, d_points, n_points, cell_size=1.0, stream=0):
        """lfx_map_create: the map a scan is matched against (KDTreeEigen, kdtree.hpp:50-71); cell_size 0 = no grid."""
        return ScanMap(self, d_points, n_points, cell_size, stream)

    def make_map_from_host(self, points, cell_size=1.0, stream=0):
        """lfx_map_create_host: points [n][4] float32 on the host."""
        return ScanMap(self, 0, 0, cell_size, stream, host_points=points)

    def scan_to_map_residuals(self, kind, scan_map, pose, n_neighbors, d_points, d_begin, d_count, count_stride, n_clouds,
                              max_points_per_cloud, d_residual, d_jacobian, stream=0):
        """lfx_scan_to_map_residuals: kind 0 = edge rows (edge.hpp:86-124), 1 = surface rows (surface.hpp:116-139);
        pose: 3 x 4 [R | t] (point_to_map); device addresses otherwise."""
        pm = np.ascontiguousarray(pose, np.float64).reshape(12)
        B.check(self._ctx, self._L.lfx_scan_to_map_residuals(
            self._ctx, int(kind), scan_map.handle, pm.ctypes.data_as(C.POINTER(C.c_double)), int(n_neighbors),
            C.c_void_p(int(d_points)), C.c_void_p(int(d_begin)), C.c_void_p(int(d_count)), int(count_stride), int(n_clouds),
            int(max_points_per_cloud), C.c_void_p(int(d_residual)), C.c_void_p(int(d_jacobian)), C.c_void_p(int(stream))))

    def edge_residuals(self, scan_map, pose, n_neighbors, d_residual, d_jacobian, stream=0):
        """lfx_edge_residuals: the edge clouds of the last device batch against an edge map."""
        pm = np.ascontiguousarray(pose, np.float64).reshape(12)
        B.check(self._ctx, self._L.lfx_edge_residuals(
            self._ctx, scan_map.handle, pm.ctypes.data_as(C.POINTER(C.c_double)), int(n_neighbors),
            C.c_void_p(int(d_residual)), C.c_void_p(int(d_jacobian)), C.c_void_p(int(stream))))

    def _align_results(self, res):
        out = []
        for r in res:
            out.append(dict(pose=np.array(r.pose[:], np.float64).reshape(3, 4), error=r.error, error_scale=r.error_scale,
                            iteration=r.iteration, code=r.code, success=r.code <= 2,
                            message=self._L.lfx_align_message(r.code).decode()))
        return out

    @staticmethod
    def _align_reports(reps):
        """lfx_align_report records as dicts: 6 x 6 matrices as arrays, the rest as numbers; `raw` keeps the record's bytes."""
        out = []
        for r in reps:
            d = dict(information=np.array(r.information[:], np.float64).reshape(6, 6), eigenvalues=np.array(r.eigenvalues[:], np.float64),
                     eigenvectors=np.array(r.eigenvectors[:], np.float64).reshape(6, 6),
                     covariance=np.array(r.covariance[:], np.float64).reshape(6, 6), raw=bytes(r))
            for k in ("sigma2", "min_eigenvalue_d", "error", "error_scale", "rms_edge", "rms_surface", "n_edge", "n_surface",
                      "n_edge_inliers", "n_surface_inliers", "n_surface_no_plane", "rank"):
                d[k] = getattr(r, k)
            d["degenerate"] = bool(r.degenerate)
            d["valid"] = bool(r.valid)
            out.append(d)
        return out

    def scan_to_map_align(self, edge_map, surface_map, n_neighbors, max_iter, d_edge_points,
                          d_edge_begin, d_edge_count, edge_count_stride, max_edge, total_edge, d_surface_points, d_surface_begin,
                          d_surface_count, surface_count_stride, max_surface, total_surface, initial_poses, stream=0, report=False):
        """lfx_scan_to_map_align: Optimizer<LOAMOptimizationProblem>::Run (optimizer.hpp:79-123) per scan; initial_poses
        [n][3][4]; returns one dict per scan (pose, error, error_scale, iteration, code, success, message).  report=True:
        lfx_scan_to_map_align_report, returns (results, reports)."""
        poses = np.ascontiguousarray(initial_poses, np.float64).reshape(-1, 12)
        res = (B.AlignResult * len(poses))()
        v = lambda a: C.c_void_p(int(a))   # noqa: E731
        args = [self._ctx, edge_map.handle, surface_map.handle, int(n_neighbors), int(max_iter),
                v(d_edge_points), v(d_edge_begin), v(d_edge_count), int(edge_count_stride), int(max_edge), int(total_edge),
                v(d_surface_points), v(d_surface_begin), v(d_surface_count), int(surface_count_stride), int(max_surface),
                int(total_surface), len(poses), poses.ctypes.data_as(C.POINTER(C.c_double)), res]
        if report:
            reps = (B.AlignReport * len(poses))()
            B.check(self._ctx, self._L.lfx_scan_to_map_align_report(*args, reps, v(stream)))
            return self._align_results(res), self._align_reports(reps)
        B.check(self._ctx, self._L.lfx_scan_to_map_align(*args, v(stream)))
        return self._align_results(res)

    def align_point_pairs(self, d_source, d_target, d_begin, d_count, max_points, total_points, max_iter, initial_poses, stream=0):
        """lfx_align_point_pairs: the same optimizer on AlignmentProblem (alignment.cpp:33-78)."""
        poses = np.ascontiguousarray(initial_poses, np.float64).reshape(-1, 12)
        res = (B.AlignResult * len(poses))()
        v = lambda a: C.c_void_p(int(a))   # noqa: E731
        B.check(self._ctx, self._L.lfx_align_point_pairs(
            self._ctx, v(d_source), v(d_target), v(d_begin), v(d_count), int(max_points), int(total_points), len(poses),
            int(max_iter), poses.ctypes.data_as(C.POINTER(C.c_double)), res, v(stream)))
        return self._align_results(res)

    def localize_batch(self, edge_map, surface_map, initial_poses, n_neighbors=15, max_iter=20, surface_leaf=1.0, stream=0,
                       report=False):
        """lfx_localize_batch: Localizer::Update (localizer.hpp:71-80) for every scan of the last device batch.  report=True:
        lfx_localize_batch_report, returns (results, reports)."""
        poses = np.ascontiguousarray(initial_poses, np.float64).reshape(-1, 12)
        res = (B.AlignResult * len(poses))()
        if report:
            reps = (B.AlignReport * len(poses))()
            B.check(self._ctx, self._L.lfx_localize_batch_report(
                self._ctx, edge_map.handle, surface_map.handle, int(n_neighbors), int(max_iter), float(surface_leaf), len(poses),
                poses.ctypes.data_as(C.POINTER(C.c_double)), res, reps, C.c_void_p(int(stream))))
            return self._align_results(res), self._align_reports(reps)
        B.check(self._ctx, self._L.lfx_localize_batch(
            self._ctx, edge_map.handle, surface_map.handle, int(n_neighbors), int(max_iter), float(surface_leaf), len(poses),
            poses.ctypes.data_as(C.POINTER(C.c_double)), res, C.c_void_p(int(stream))))
        return self._align_results(res)

    def localize_host(self, edge_map, surface_map, edge_points, surface_points, initial_pose, n_neighbors=15, max_iter=20,
                      surface_leaf=1.0, stream=0, report=False):
        """lfx_localize_host: Localizer::Update for one scan whose clouds ([n][4] float32) are on the host.  report=True:
        lfx_localize_host_report, returns (result, report)."""
        e = np.ascontiguousarray(edge_points, np.float32).reshape(-1, 4)
        sf = np.ascontiguousarray(surface_points, np.float32).reshape(-1, 4)
        pose = np.ascontiguousarray(initial_pose, np.float64).reshape(12)
        res = (B.AlignResult * 1)()
        if report:
            reps = (B.AlignReport * 1)()
            B.check(self._ctx, self._L.lfx_localize_host_report(
                self._ctx, edge_map.handle, surface_map.handle, int(n_neighbors), int(max_iter), float(surface_leaf),
                C.c_void_p(e.ctypes.data), len(e), C.c_void_p(sf.ctypes.data), len(sf), pose.ctypes.data_as(C.POINTER(C.c_double)),
                res, reps, C.c_void_p(int(stream))))
            return self._align_results(res)[0], self._align_reports(reps)[0]
        B.check(self._ctx, self._L.lfx_localize_host(
            self._ctx, edge_map.handle, surface_map.handle, int(n_neighbors), int(max_iter), float(surface_leaf),
            C.c_void_p(e.ctypes.data), len(e), C.c_void_p(sf.ctypes.data), len(sf), pose.ctypes.data_as(C.POINTER(C.c_double)), res,
            C.c_void_p(int(stream))))
        return self._align_results(res)[0]

    def odometry(self, **config):
        """lfx_odometry_create: Odometry over EdgeSurfaceMap (odometry.hpp:52-63) on this context's device.  Keywords: the
        fields of lfx_odometry_config (n_local_scans=7, n_neighbors=15, max_iter=20, surface_leaf=1.0, edge_cell=1.0,
        surface_cell=1.0, edge_capacity_points, surface_capacity_points, initial_pose: 3 x 4)."""
        return Odometry(self, **config)

    def mapper(self, **config):
        """lfx_mapper_create: MapBuilder (map.hpp:95-153) with its map on this context's device.  Keywords: the fields of
        lfx_mapper_config (translation_threshold=1.0, rotation_threshold=0.1, initial_capacity_points=2^20,
        max_points=2^32 - 1)."""
        return Mapper(self, **config)

    def rolling_map(self, **config):
        """lfx_rolling_map_create: a rolling voxel map on this context's device.  Keywords: the fields of
        lfx_rolling_map_config (edge_leaf=0.2, surface_leaf=0.4, edge_dims=(512, 512, 128), surface_dims=(256, 256, 64),
        match_half_extent=(50, 50, 12.8), n_neighbors=15, max_iter=20, scan_surface_leaf=1.0, edge_cell=1.0, surface_cell=1.0,
        initial_pose: 3 x 4)."""
        return RollingMap(self, **config)

    def set_ring_ids(self, ring_ids):
        """lfx_set_ring_ids: the sensor's ring ids for the device path (None: back to 0 .. max_rings-1)."""
        if ring_ids is None:
            B.check(self._ctx, self._L.lfx_set_ring_ids(self._ctx, None, 0), self._L)
            return
        ids = (C.c_uint16 * len(ring_ids))(*[int(r) for r in ring_ids])
        B.check(self._ctx, self._L.lfx_set_ring_ids(self._ctx, ids, len(ring_ids)), self._L)

    def scan_routes(self, n_scans, stream=0):
        """lfx_scan_routes: per scan of the last batch 1 = read in place, 2 = in place through ring transforms, 3 = in place as a
        grid with (0, 0, 0) records the zero filter dropped, 0 = bucketed."""
        out = np.zeros(n_scans, np.uint8)
        B.check(self._ctx, self._L.lfx_scan_routes(self._ctx, C.c_void_p(int(stream)), C.c_void_p(out.ctypes.data)), self._L)
        return out

    def batch_status(self, stream=0):
        """lfx_batch_status: raises LfxError if a scan of the last device batch carries an error bit."""
        bad = C.c_uint32(0)
        B.check(self._ctx, self._L.lfx_batch_status(self._ctx, C.c_void_p(int(stream)), C.byref(bad)), self._L)

    def extract_batch_device(self, d_points, n_points, stream=0):
        """d_points: device address of the scans' records back to back; asynchronous on `stream`."""
        n = np.ascontiguousarray(n_points, dtype=np.uint32)
        B.check(self._ctx, self._L.lfx_extract_batch_device(
            self._ctx, C.c_void_p(int(d_points)), n.ctypes.data_as(C.POINTER(C.c_uint32)), len(n),
            C.c_void_p(int(stream))))

    def device_view(self):
        v = B.DeviceView()
        B.check(self._ctx, self._L.lfx_device_results(self._ctx, C.byref(v)), self._L)
        return v

    def pack_features(self, d_edge_out, d_surface_out, d_offsets_out, capacity_points, stream=0):
        """Pack the last device batch's clouds into caller-owned device buffers (see lfx.h)."""
        B.check(self._ctx, self._L.lfx_pack_features(
            self._ctx, C.c_void_p(int(d_edge_out)), C.c_void_p(int(d_surface_out)), C.c_void_p(int(d_offsets_out)),
            int(capacity_points), C.c_void_p(int(stream))))

    def pack_xyz(self, d_edge_out, d_surface_out, d_offsets_out, capacity_points, stream=0):
        """As pack_features, but pcl::PointXYZ wire records (x, y, z, 1.0f): scan_edge / scan_surface payloads."""
        B.check(self._ctx, self._L.lfx_pack_xyz(
            self._ctx, C.c_void_p(int(d_edge_out)), C.c_void_p(int(d_surface_out)), C.c_void_p(int(d_offsets_out)),
            int(capacity_points), C.c_void_p(int(stream))))

    def pack_xyz12(self, d_edge_out, d_surface_out, d_offsets_out, capacity_points, stream=0):
        """As pack_features, but tight x, y, z triples ([capacity][3] floats): the gather payload."""
        B.check(self._ctx, self._L.lfx_pack_xyz12(
            self._ctx, C.c_void_p(int(d_edge_out)), C.c_void_p(int(d_surface_out)), C.c_void_p(int(d_offsets_out)),
            int(capacity_points), C.c_void_p(int(stream))))

    def pack_colored(self, d_colored_out, d_offsets_out, capacity_points, stream=0):
        """colored_scan of the last device batch as 32-byte pcl::PointXYZRGB wire records (see lfx.h)."""
        B.check(self._ctx, self._L.lfx_pack_colored(
            self._ctx, C.c_void_p(int(d_colored_out)), C.c_void_p(int(d_offsets_out)), int(capacity_points),
            C.c_void_p(int(stream))))

    def deskew(self, time, sweeps, to="end", out=None, stream=0):
        """lfx_deskew_batch: the sensor's motion during each sweep taken out of the last device batch's edge and surface
        clouds.  time: None or "index" (a record's firing time is its index in the scan over the scan's point count), or
        a B.TimeField (time_field_from_fields); sweeps: one per scan, a 3 x 4 motion (the sensor frame at the sweep's end in
        its frame at the start; index times) or (t0, t1, motion); to: "end" or "start", the frame the points are carried to;
        out: None = in place (every later call on this batch sees the de-skewed clouds), or (d_edge_out, d_surface_out),
        device addresses of buffers laid out like device_view().edge_points / surface_points.  Asynchronous on `stream`."""
        tf = _time_field(time)
        sw, n = _sweeps(sweeps)
        e, s = (0, 0) if out is None else out
        B.check(self._ctx, self._L.lfx_deskew_batch(
            self._ctx, C.byref(tf), sw, n, _deskew_to(to), C.c_void_p(int(e) or None), C.c_void_p(int(s) or None),
            C.c_void_p(int(stream))), self._L)

    def deskew_trajectory(self, time, trajectories, out=None, stream=0):
        """lfx_deskew_batch_trajectory: deskew() along the sensor's poses within each sweep.  trajectories: one per scan,
        (times [k], poses [k][3][4], t_ref) or a dict with those names: the sensor's pose, in one fixed frame, at 2 .. 64
        strictly ascending times (seconds with a time field, fractions of the sweep with index times); the records are
        brought to the sensor frame at t_ref.  time, out, stream: as deskew() takes them."""
        tf = _time_field(time)
        tr, n, _keep = _trajectories(trajectories)
        e, s = (0, 0) if out is None else out
        B.check(self._ctx, self._L.lfx_deskew_batch_trajectory(
            self._ctx, C.byref(tf), tr, n, C.c_void_p(int(e) or None), C.c_void_p(int(s) or None), C.c_void_p(int(stream))), self._L)

    def scan_context(self, config=None, out=None, stream=0):
        """lfx_scan_context_batch: the scan-context descriptor of every scan of the last device batch, from the batch's input
        records (which must still be alive).  config: None (the defaults: 20 rings x 60 sectors out to 80 m), a dict of
        lfx_scan_context_config's fields or a B.ScanContextConfig; out: None = a new float32 device tensor [n_scans][R][S] is
        returned, or the device address of such a buffer (nothing is returned).  Asynchronous on `stream`."""
        cfg = scan_context_config(config)
        n = int(self.device_view().batch)
        made = None
        if out is None:
            import torch
            made = torch.empty((n, cfg.n_rings, cfg.n_sectors), dtype=torch.float32, device=torch.device("cuda", self.device))
            out = made.data_ptr()
        B.check(self._ctx, self._L.lfx_scan_context_batch(self._ctx, C.byref(cfg), n, C.c_void_p(int(out) or None),
                                                          C.c_void_p(int(stream))), self._L)
        return made

    def batch_points(self):
        """lfx_batch_points: the input records of the last batch the context ran, whichever call ran it (0: none yet)."""
        n = C.c_uint64(0)
        B.check(self._ctx, self._L.lfx_batch_points(self._ctx, C.byref(n)), self._L)
        return int(n.value)

    def segment(self, config=None, classes=None, ids=None, counts=None, stream=0):
        """lfx_segment_batch: every input record of the last batch (whose records must still be alive) classed as
        B.SEG_NONE / SEG_GROUND / SEG_SEGMENT / SEG_CLUTTER through a range image, with its cluster's id.  config: None
        (the defaults: 16 x 1800), a dict of lfx_segment_config's fields or a B.SegmentConfig; classes (uint8, one per record),
        ids (one per record) and counts ([n_scans][4]) -- the library's uint32 in int32 tensors: B.SEG_NO_ID reads as -1 --:
        device tensors to write into, addressed by the view's scan_begin; None = new ones, sized by batch_points(); ids /
        counts False = not wanted (the library is handed NULL and None comes back in its place).  A tensor with fewer elements
        than the batch has records (counts: than 4 per scan) is refused.  Returns (classes, ids, counts).  Asynchronous on
        `stream`."""
        import torch
        cfg = segment_config(config)
        n = int(self.device_view().batch)
        dev = torch.device("cuda", self.device)
        total = self.batch_points()
        if classes is None:
            classes = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)[:total]
        if ids is None:
            ids = torch.empty(max(total, 1), dtype=torch.int32, device=dev)[:total]
        elif ids is False:
            ids = None
        if counts is None:
            counts = torch.empty((max(n, 1), 4), dtype=torch.int32, device=dev)[:n]
        elif counts is False:
            counts = None
        for name, t, need, size in (("classes", classes, total, 1), ("ids", ids, total, 4), ("counts", counts, 4 * n, 4)):
            if t is not None and (t.numel() < need or t.element_size() != size or not t.is_contiguous()):
                raise B.LfxError(B.ERR_INVALID_ARGUMENT, "%s must be a contiguous tensor of at least %d elements of %d byte(s): the last "
                                 "batch has %d records in %d scans" % (name, need, size, total, n))
        ptr = lambda t: C.c_void_p((t.data_ptr() or None) if t is not None else None)
        B.check(self._ctx, self._L.lfx_segment_batch(self._ctx, C.byref(cfg), n, ptr(classes), ptr(ids), ptr(counts), C.c_void_p(int(stream))),
                self._L)
        return classes, ids, counts

    def pack_features_segmented(self, classes, edge_mask=B.SEG_EDGE_MASK_DEFAULT, surface_mask=B.SEG_SURFACE_MASK_DEFAULT,
                                capacity=None, counts=False, stream=0):
        """lfx_pack_features_segmented: pack_features through a class mask -- a feature is kept iff bit 1 << class of its
        original point (classes: segment()'s uint8 device tensor for this batch) is set in its cloud's mask.  capacity: records
        per output buffer (None: room for every feature of the batch).  Returns (edge [capacity][4] float32, surface, offsets
        uint32-as-int32 [2][batch + 1]) and, with counts=True, the kept records per scan, [2][batch], as a fourth -- device
        tensors.  Asynchronous on `stream`."""
        import torch
        n = int(self.device_view().batch)
        dev = torch.device("cuda", self.device)
        total = self.batch_points()
        if classes.numel() < total or classes.element_size() != 1:
            raise B.LfxError(B.ERR_INVALID_ARGUMENT, "classes must hold one byte for each of the last batch's %d records" % total)
        if capacity is None:
            capacity = max(total, 1)
        capacity = int(capacity)
        edge = torch.empty((max(capacity, 1), 4), dtype=torch.float32, device=dev)
        surface = torch.empty((max(capacity, 1), 4), dtype=torch.float32, device=dev)
        offsets = torch.empty((2, n + 1), dtype=torch.int32, device=dev)
        kept = torch.empty((2, max(n, 1)), dtype=torch.int32, device=dev)[:, :n] if counts else None
        B.check(self._ctx, self._L.lfx_pack_features_segmented(
            self._ctx, C.c_void_p(classes.data_ptr() or None), int(edge_mask), int(surface_mask), C.c_void_p(edge.data_ptr()),
            C.c_void_p(surface.data_ptr()), C.c_void_p(offsets.data_ptr()), C.c_void_p(kept.data_ptr() if counts else None),
            capacity, C.c_void_p(int(stream))), self._L)
        return (edge, surface, offsets, kept) if counts else (edge, surface, offsets)

    def pose_graph(self, max_nodes, max_edges, config=None, **fields):
        """lfx_pose_graph_create: a pose graph of the given capacities on this context's device."""
        return PoseGraph(self, max_nodes, max_edges, config, **fields)

    def keyframes(self, max_keyframes, max_points):
        """lfx_keyframes_create: a keyframe store of the given capacities (max_points: one value for both kinds or
        (edge, surface) records) on this context's device."""
        return Keyframes(self, max_keyframes, max_points)

    def voxel_filter(self, log2_slots, max_records):
        """lfx_voxel_filter_create: a voxel filter of 2^log2_slots voxel entries (about twice the voxels expected) that can take
        max_records records between two resets, on this context's device."""
        return VoxelFilter(self, log2_slots, max_records)

    def occupancy_grid(self, width, height, resolution, origin=(0.0, 0.0), max_scans=1024, config=None, **fields):
        """lfx_occupancy_create: a 2-D occupancy grid of width x height cells of `resolution` metres whose cell (0, 0) has its
        lower-left corner at `origin`, with room for max_scans scans' beams, on this context's device; the other fields of
        lfx_occupancy_config as keywords."""
        return OccupancyGrid(self, width, height, resolution, origin, max_scans, config, **fields)

    def grid_matcher(self, width, height, resolution, origin=(0.0, 0.0), config=None, **fields):
        """lfx_grid_match_create: a scan matcher over grids of width x height cells on this context's device."""
        return GridMatcher(self, width, height, resolution, origin, config, **fields)

    def distance_field(self, width, height):
        """lfx_distance_create: a distance field over grids of width x height cells on this context's device."""
        return DistanceField(self, width, height)

    def visibility(self, max_window=1024, max_resident_images=None, config=None, **fields):
        """lfx_visibility_create: visibility votes over windows of up to max_window keyframes, max_resident_images (default:
        all of them) range images on the device at a time; the fields of lfx_visibility_config as keywords."""
        return Visibility(self, max_window, max_resident_images, config, **fields)

    def place_db(self, capacity, config=None):
        """lfx_place_db_create: a place index of `capacity` scan-context descriptors of `config` on this context's device."""
        return PlaceDb(self, capacity, config)

    def loop_closer(self, keyframes, place_db, graph, config=None, **fields):
        """lfx_loop_closer_create: a loop closer over a Keyframes store, a PlaceDb and a PoseGraph of this context (keyframe id
        == place entry == graph node id); the fields of lfx_loop_closer_config as keywords (submap_capacity is required)."""
        return LoopCloser(self, keyframes, place_db, graph, config, **fields)

    def download(self, scan, stream=0):
        r = B.ScanResult()
        B.check(self._ctx, self._L.lfx_download_scan(self._ctx, scan, C.c_void_p(int(stream)), C.byref(r)), self._L)
        return _result(r)

    # --- per-stage entry points ------------------------------------------------------------
    def stage_ring(self, x, y, flags, params=None, groups=None, curvature_in=None, range_in=None):
        """Run selected stages of the ring kernel on one angle-sorted ring.
        Returns dict(range, curvature, link, labels, status)."""
        x = np.ascontiguousarray(x, np.float32)
        y = np.ascontiguousarray(y, np.float32)
        n = len(x)
        g = None if groups is None else np.ascontiguousarray(groups, np.int32)
        ci = None if curvature_in is None else np.ascontiguousarray(curvature_in, np.float64)
        ri = None if range_in is None else np.ascontiguousarray(range_in, np.float64)
        out_r, out_c = np.zeros(n), np.zeros(n)
        out_l, out_lab = np.zeros(max(n - 1, 0), np.uint8), np.zeros(n, np.uint8)
        st = C.c_int32(0)
        cp = (params or self.params).to_c()

        def p(a):
            return None if a is None else C.c_void_p(a.ctypes.data)

        B.check(self._ctx, self._L.lfx_stage_ring(
            self._ctx, C.byref(cp), flags, n, p(x), p(y), p(g), p(ci), p(ri), p(out_r), p(out_c),
            p(out_l) if n > 1 else None, p(out_lab), C.cast(C.byref(st), C.c_void_p)))
        return {"range": out_r, "curvature": out_c, "link": out_l.astype(bool), "labels": out_lab,
                "status": st.value}

    def convolution1d(self, values, weight):
        """Convolution1D, convolution.cpp:35-66 (raises LfxError where the reference throws)."""
        v = np.ascontiguousarray(values, np.float64)
        w = np.ascontiguousarray(weight, np.float64)
        out = np.zeros(len(v))
        B.check(self._ctx, self._L.lfx_stage_convolution1d(
            self._ctx, C.c_void_p(v.ctypes.data), len(v), C.c_void_p(w.ctypes.data), len(w),
            C.c_void_p(out.ctypes.data)))
        return out

    def ring_projection(self, cloud):
        """ExtractAngleSortedRings, ring.hpp:141-147 -> {ring id: sorted original indices}."""
        cloud = np.ascontiguousarray(cloud)
        n = len(cloud)
        idx = np.zeros(n, np.uint32)
        nr = C.c_uint32(0)
        rid = np.zeros(B.MAX_RINGS, np.uint16)
        cnt = np.zeros(B.MAX_RINGS, np.uint32)
        B.check(self._ctx, self._L.lfx_stage_ring_projection(
            self._ctx, C.c_void_p(cloud.ctypes.data), n, C.c_void_p(idx.ctypes.data), C.byref(nr),
            C.c_void_p(rid.ctypes.data), C.c_void_p(cnt.ctypes.data)))
        out, off = {}, 0
        for k in range(nr.value):
            out[int(rid[k])] = idx[off:off + cnt[k]].copy()
            off += int(cnt[k])
        return out

    def ColorPointsByLabel(self, cloud, labels):
        """colored_scan (color_points.hpp:60-74): [n,4] f32 = x, y, z, packed rgb (as PCL's PointXYZRGB)."""
        cloud = np.ascontiguousarray(cloud)
        labels = np.ascontiguousarray(labels, np.uint8)
        out = np.zeros((len(cloud), 4), np.float32)
        B.check(self._ctx, self._L.lfx_color_points_by_label(
            self._ctx, C.c_void_p(cloud.ctypes.data), len(cloud), C.c_void_p(labels.ctypes.data),
            C.c_void_p(out.ctypes.data)))
        return out

    # --- measurement ---------------------------------------------------------------------
    def set_profiling(self, on, every=1):
        """HIP events around the kernels of every `every`-th batch (lfx_set_profiling_interval)."""
        B.check(self._ctx, self._L.lfx_set_profiling_interval(self._ctx, int(every)), self._L)
        B.check(self._ctx, self._L.lfx_set_profiling(self._ctx, int(bool(on))), self._L)

    def box_calibration(self, nbytes=0, stream=0):
        """(copy GB/s, shader clock MHz) of this device now: lfx_box_calibration."""
        gbs, mhz = C.c_double(0), C.c_double(0)
        B.check(self._ctx, self._L.lfx_box_calibration(self._ctx, int(nbytes), C.c_void_p(int(stream)), C.byref(gbs), C.byref(mhz)), self._L)
        return gbs.value, mhz.value

    def kernel_times(self):
        ms = (C.c_double * B.LFX_N_KERNELS)()
        cnt = (C.c_uint64 * B.LFX_N_KERNELS)()
        B.check(self._ctx, self._L.lfx_kernel_times(self._ctx, ms, cnt), self._L)
        return {self._L.lfx_kernel_name(k).decode(): (ms[k], int(cnt[k])) for k in range(B.LFX_N_KERNELS)}


def layout_from_fields(fields, point_step, is_bigendian=False):
    """fields: iterable of (name, offset, datatype, count) as in PointCloud2.fields -> binding.Layout for
    FeatureExtraction(layout=...).  Raises LfxError where the node would refuse the cloud (no ring channel)
    or pcl::fromROSMsg could not map x / y / z."""
    arr = (B.PointField * len(fields))(*[B.PointField(n.encode(), o, t, c) for (n, o, t, c) in fields])
    out = B.Layout()
    rc = B.load().lfx_layout_from_fields(arr, len(fields), point_step, int(bool(is_bigendian)), C.byref(out))
    if rc != 0:
        raise B.LfxError(rc, {-7: "the cloud has no ring field", -8: "x / y / z must be FLOAT32 and ring an integer field inside point_step"}.get(rc, "invalid field list"))
    return out



def _time_field(time):
    if time is None or (isinstance(time, str) and time == "index"):
        return B.TimeField(B.TIME_FROM_INDEX, 0, 0, 0, 1.0)
    if isinstance(time, B.TimeField):
        return time
    raise TypeError("time must be None, 'index' or a binding.TimeField")


def _deskew_to(to):
    if to in ("end", "start"):
        return B.DESKEW_TO_END if to == "end" else B.DESKEW_TO_START
    return int(to)


def _sweeps(sweeps):
    out = (B.Sweep * max(len(sweeps), 1))()
    for i, s in enumerate(sweeps):
        if isinstance(s, B.Sweep):
            out[i] = s
            continue
        if isinstance(s, (tuple, list)) and len(s) == 3 and np.ndim(s[0]) == 0:
            out[i].t0, out[i].t1, m = float(s[0]), float(s[1]), s[2]
        else:
            m = s
        out[i].motion[:] = [float(x) for x in np.asarray(m, np.float64).reshape(12)]
    return out, len(sweeps)


def _trajectories(trajectories):
    """(lfx_trajectory array, count, the arrays it points into: the caller keeps them alive over the call)."""
    out = (B.Trajectory * max(len(trajectories), 1))()
    keep = []
    for i, tr in enumerate(trajectories):
        times, poses, t_ref = (tr["times"], tr["poses"], tr["t_ref"]) if isinstance(tr, dict) else tr
        t = np.ascontiguousarray(times, np.float64).reshape(-1)
        p = np.ascontiguousarray(poses, np.float64).reshape(-1)
        if len(p) != 12 * len(t):
            raise ValueError("trajectory %d: %d times but %d pose values" % (i, len(t), len(p)))
        keep += [t, p]
        out[i].n_knots, out[i].times, out[i].poses, out[i].t_ref = len(t), _pd(t), _pd(p), float(t_ref)
    return out, len(trajectories), keep


def time_field_from_fields(fields, point_step, is_bigendian=False):
    """lfx_time_field_from_fields: the per-point time channel of a PointCloud2 field list (iterable of (name, offset,
    datatype, count)) -> binding.TimeField for deskew(): the first field named t, time, timestamp, time_stamp or
    offset_time with count 1; seconds in FLOAT32 / FLOAT64, nanoseconds in UINT32.  Raises LfxError (ERR_NO_TIME_FIELD,
    ERR_UNSUPPORTED_FIELD).  No device."""
    arr = (B.PointField * max(len(fields), 1))(*[B.PointField(n.encode(), o, t, c) for (n, o, t, c) in fields])
    out = B.TimeField()
    rc = B.load().lfx_time_field_from_fields(arr, len(fields), point_step, int(bool(is_bigendian)), C.byref(out))
    if rc != 0:
        raise B.LfxError(rc, {-10: "the cloud has no per-point time field",
                              -8: "the time field must be FLOAT32, FLOAT64 or UINT32 inside point_step"}.get(rc, "invalid field list"))
    return out


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def motion_between(pose0, pose1):
    """lfx_motion_between: pose0^-1 pose1 (3 x 4 [R | t]): the sensor's frame at pose1 expressed in its frame at pose0.  No device."""
    a = np.ascontiguousarray(pose0, np.float64).reshape(12)
    b = np.ascontiguousarray(pose1, np.float64).reshape(12)
    out = np.zeros(12, np.float64)
    if B.load().lfx_motion_between(_pd(a), _pd(b), _pd(out)) != 0:
        raise B.LfxError(-1, "invalid argument")
    return out.reshape(3, 4)


def motion_twist(motion):
    """lfx_motion_twist: (w, theta) of a motion's rotation -- the angle-axis vector Log(R) and its length, as the de-skew
    kernel is given them.  No device."""
    m = np.ascontiguousarray(motion, np.float64).reshape(12)
    w, th = np.zeros(3, np.float64), C.c_double(0)
    if B.load().lfx_motion_twist(_pd(m), _pd(w), C.byref(th)) != 0:
        raise B.LfxError(-1, "invalid argument")
    return w, th.value


def motion_scale(motion, ratio):
    """lfx_motion_scale: [Exp(ratio w) | ratio t] of a motion [Exp(w) | t] (a sweep shorter than the scan period).  No device."""
    m = np.ascontiguousarray(motion, np.float64).reshape(12)
    out = np.zeros(12, np.float64)
    if B.load().lfx_motion_scale(_pd(m), float(ratio), _pd(out)) != 0:
        raise B.LfxError(-1, "invalid argument")
    return out.reshape(3, 4)


def trajectory_segments(times, poses, t_ref):
    """lfx_trajectory_segments: the table the trajectory de-skew kernel is given, [n_knots - 1][24] doubles (include/lfx.h
    names the columns).  Raises LfxError where lfx_deskew_batch_trajectory would refuse the trajectory.  No device."""
    tr, _, _keep = _trajectories([(times, poses, t_ref)])
    n = int(tr[0].n_knots)
    out = np.zeros((max(n, 2) - 1, B.TRAJECTORY_SEGMENT_DOUBLES), np.float64)
    if n > B.MAX_TRAJECTORY_KNOTS or B.load().lfx_trajectory_segments(tr, _pd(out)) != 0:
        raise B.LfxError(-1, "invalid trajectory")
    return out


def trajectory_from_gyro(times, rates, bias=None, velocity=None):
    """lfx_trajectory_from_gyro: knot poses [n][3][4] from gyro samples (rates [n][3] rad/s in the sensor frame at times [n]),
    the first pose the identity; bias [3] is taken off the rates, velocity [3] is constant in the first sample's frame.  No device."""
    t = np.ascontiguousarray(times, np.float64).reshape(-1)
    r = np.ascontiguousarray(rates, np.float64).reshape(-1)
    if len(r) != 3 * len(t):
        raise ValueError("%d times but %d rate values" % (len(t), len(r)))
    b = None if bias is None else np.ascontiguousarray(bias, np.float64).reshape(3)
    v = None if velocity is None else np.ascontiguousarray(velocity, np.float64).reshape(3)
    out = np.zeros((max(len(t), 1), 3, 4), np.float64)
    if B.load().lfx_trajectory_from_gyro(_pd(t), _pd(r), len(t), None if b is None else _pd(b), None if v is None else _pd(v), _pd(out)) != 0:
        raise B.LfxError(-1, "invalid gyro samples")
    return out


def _config(struct, default_name, what, config, fields):
    """What the *_config functions share: a new `struct` holding the defaults (the library's default_name) with the given
    fields replaced.  config: None, a dict of fields, or a `struct` (copied); `what` names the settings in a refusal."""
    cfg = struct()
    if isinstance(config, struct):
        C.memmove(C.byref(cfg), C.byref(config), C.sizeof(cfg))
        config = None
    else:
        getattr(B.load(), default_name)(C.byref(cfg))
    for k, v in dict(config or {}, **fields).items():
        if k not in dict(struct._fields_):
            raise TypeError("unknown %s setting %r" % (what, k))
        setattr(cfg, k, v)
    return cfg


def _tables(tables_name, what, cfg, W, n_last):
    """What the *_tables functions share: (cos [W], sin [W], the config's third table [n_last]), float64, from the library's
    tables_name.  The arrays are sized for any config: a refused one must not write past them before it is refused -- it
    writes nothing."""
    cs, sn, last = np.zeros(max(W, 1)), np.zeros(max(W, 1)), np.zeros(n_last)
    rc = getattr(B.load(), tables_name)(C.byref(cfg), _pd(cs), _pd(sn), _pd(last))
    if rc != 0:
        raise B.LfxError(rc, "the %s config is refused" % what)
    return cs[:W], sn[:W], last


def scan_context_config(config=None, **fields):
    """lfx_scan_context_config: the defaults (lfx_scan_context_default_config) with the given fields replaced.  config: None,
    a dict of fields, or a B.ScanContextConfig (copied)."""
    return _config(B.ScanContextConfig, "lfx_scan_context_default_config", "scan-context", config, fields)


def scan_context_tables(config=None):
    """lfx_scan_context_tables: (sector_cos [S], sector_sin [S], ring_r2 [R + 1]), float64 -- the tables the descriptor kernel is
    given, and the only source of them.  Host only."""
    cfg = scan_context_config(config)
    return _tables("lfx_scan_context_tables", "scan-context", cfg, int(cfg.n_sectors), int(cfg.n_rings) + 1)


def segment_config(config=None, **fields):
    """lfx_segment_config: the defaults (lfx_segment_default_config) with the given fields replaced.  config: None, a dict of
    fields, or a B.SegmentConfig (copied)."""
    return _config(B.SegmentConfig, "lfx_segment_default_config", "segmentation", config, fields)


def segment_tables(config=None):
    """lfx_segment_tables: (col_cos [W], col_sin [W], consts [4]), float64 -- the tables the segmentation kernels are given, and
    the only source of them.  Host only."""
    cfg = segment_config(config)
    return _tables("lfx_segment_tables", "segmentation", cfg, int(cfg.n_columns), 4)


def visibility_config(config=None, **fields):
    """lfx_visibility_config: the defaults (lfx_visibility_default_config) with the given fields replaced.  config: None, a
    dict of fields, or a B.VisibilityConfig (copied)."""
    return _config(B.VisibilityConfig, "lfx_visibility_default_config", "visibility", config, fields)


def visibility_tables(config=None):
    """lfx_visibility_tables: (col_cos [W], col_sin [W], row_tan [H + 1]), float64 -- the tables the visibility kernels are
    given, and the only source of them.  Host only."""
    cfg = visibility_config(config)
    return _tables("lfx_visibility_tables", "visibility", cfg, int(cfg.n_columns), int(cfg.n_rows) + 1)


def occupancy_config(config=None, **fields):
    """lfx_occupancy_config: the defaults (lfx_occupancy_default_config; the grid's size, resolution, origin and max_scans are
    the caller's) with the given fields replaced.  config: None, a dict of fields, or a B.OccupancyConfig (copied)."""
    return _config(B.OccupancyConfig, "lfx_occupancy_default_config", "occupancy", config, fields)


def occupancy_tables(config):
    """lfx_occupancy_tables: (col_cos [W], col_sin [W]), float64 -- the column tables the reduce kernel is given, and the only
    source of them.  Host only."""
    cfg = occupancy_config(config)
    W = int(cfg.n_beams)
    cs, sn = np.zeros(max(W, 1)), np.zeros(max(W, 1))
    rc = B.load().lfx_occupancy_tables(C.byref(cfg), _pd(cs), _pd(sn))
    if rc != 0:
        raise B.LfxError(rc, "the occupancy config is refused")
    return cs[:W], sn[:W]


def occupancy_emit_config(config=None, **fields):
    """lfx_occupancy_emit_config: the defaults (OctoMap's log-odds in hundredths) with the given fields replaced."""
    return _config(B.OccupancyEmitConfig, "lfx_occupancy_emit_default_config", "occupancy emit", config, fields)


def occupancy_emit_table(config=None):
    """lfx_occupancy_emit_table: the int8 look-up table [l_max - l_min + 1] the emit kernel is handed.  Host only."""
    cfg = occupancy_emit_config(config)
    lut = np.zeros(4097, np.int8)
    rc = B.load().lfx_occupancy_emit_table(C.byref(cfg), C.c_void_p(lut.ctypes.data))
    if rc != 0:
        raise B.LfxError(rc, "the occupancy emit config is refused")
    return lut[:int(cfg.l_max) - int(cfg.l_min) + 1].copy()


def distance_config(config=None, **fields):
    """lfx_distance_config: the defaults (occupied_percent 65, unknown cells no obstacles, no cap, no inside field) with the
    given fields replaced."""
    return _config(B.DistanceConfig, "lfx_distance_default_config", "distance", config, fields)


def distance_cost_config(config=None, **fields):
    """lfx_distance_cost_config: nav2's inflation defaults (0.22 m, 0.55 m, 10.0, unknown cells tracked) with the given
    fields replaced."""
    return _config(B.DistanceCostConfig, "lfx_distance_cost_default_config", "distance cost", config, fields)


def distance_cost_table(config=None, resolution=0.05, n=None):
    """lfx_distance_cost_table: the uint8 table [Rc * Rc + 1] the costmap kernel is handed, and the only source of the decay.
    Host only.  n: the size to ask with (None: lfx_distance_cost_table_size's)."""
    cfg = distance_cost_config(config)
    L = B.load()
    if n is None:
        size = C.c_uint32(0)
        rc = L.lfx_distance_cost_table_size(C.byref(cfg), float(resolution), C.byref(size))
        if rc != 0:
            raise B.LfxError(rc, "the distance cost config is refused")
        n = int(size.value)
    lut = np.zeros(max(int(n), 1), np.uint8)
    rc = L.lfx_distance_cost_table(C.byref(cfg), float(resolution), C.c_void_p(lut.ctypes.data), int(n))
    if rc != 0:
        raise B.LfxError(rc, "the distance cost config is refused")
    return lut[:int(n)]


def grid_match_config(config=None, **fields):
    """lfx_grid_match_config: the defaults (64 scans of 1800 beams, windows of up to 101 x 101 cells and 61 headings; the
    grid's size, resolution and origin are the caller's) with the given fields replaced."""
    return _config(B.GridMatchConfig, "lfx_grid_match_default_config", "grid match", config, fields)


def grid_match_table_config(config=None, **fields):
    """lfx_grid_match_table_config: AMCL's likelihood field (sigma 0.2 m, reach 2.0 m) at a peak of 1000, with the given fields
    replaced."""
    return _config(B.GridMatchTableConfig, "lfx_grid_match_table_default_config", "grid match table", config, fields)


def grid_match_search_config(config=None, **fields):
    """lfx_grid_match_search_config: a window of 21 x 21 cells and one heading, with the given fields replaced."""
    return _config(B.GridMatchSearchConfig, "lfx_grid_match_search_default_config", "grid match search", config, fields)


def grid_match_table(config=None, resolution=0.05, n=None):
    """lfx_grid_match_table: the uint16 table [Rs * Rs + 1] the field kernel is handed, and the only source of the decay.
    Host only.  n: the size to ask with (None: lfx_grid_match_table_size's)."""
    cfg = grid_match_table_config(config)
    L = B.load()
    if n is None:
        size = C.c_uint32(0)
        rc = L.lfx_grid_match_table_size(C.byref(cfg), float(resolution), C.byref(size))
        if rc != 0:
            raise B.LfxError(rc, "the grid match table config is refused")
        n = int(size.value)
    lut = np.zeros(max(int(n), 1), np.uint16)
    rc = L.lfx_grid_match_table(C.byref(cfg), float(resolution), C.c_void_p(lut.ctypes.data), int(n))
    if rc != 0:
        raise B.LfxError(rc, "the grid match table config is refused")
    return lut[:int(n)]


def grid_match_search_size(search=None, **fields):
    """lfx_grid_match_search_size: (Nx, Ny, T) of a search config.  Host only."""
    cfg = grid_match_search_config(search, **fields)
    dims = (C.c_uint32 * 3)()
    rc = B.load().lfx_grid_match_search_size(C.byref(cfg), dims)
    if rc != 0:
        raise B.LfxError(rc, "the grid match search config is refused")
    return tuple(int(v) for v in dims)


def grid_match_rotations(yaw0, half_theta, theta_step):
    """lfx_grid_match_rotations: float64 [2 * half_theta + 1][2] = (cos, sin) of the search's headings, and the only source of
    them.  Host only."""
    cs = np.zeros((2 * min(int(half_theta), B.GRID_MATCH_MAX_HALF_THETA) + 1, 2))
    rc = B.load().lfx_grid_match_rotations(float(yaw0), int(half_theta), float(theta_step), C.c_void_p(cs.ctypes.data))
    if rc != 0:
        raise B.LfxError(rc, "the rotations are refused")
    return cs


def grid_match_candidate(search, resolution, centre, index):
    """lfx_grid_match_candidate: (x, y, yaw) of candidate `index` of a search around centre (x0, y0, yaw0).  Host only."""
    cfg = grid_match_search_config(search)
    c3, out = np.ascontiguousarray(centre, np.float64).reshape(3), np.zeros(3)
    rc = B.load().lfx_grid_match_candidate(C.byref(cfg), float(resolution), C.c_void_p(c3.ctypes.data), int(index), C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise B.LfxError(rc, "the candidate is refused")
    return out


def grid_match_pose3(pose2, level=None, z=0.0):
    """lfx_grid_match_pose3: [Rz(yaw) x level | (x, y, z)] as [3][4] float64 -- the initial pose the 3-D alignment asks for.
    level: [3][3] or None = identity.  Host only."""
    p2, out = np.ascontiguousarray(pose2, np.float64).reshape(3), np.zeros(12)
    lv = None if level is None else np.ascontiguousarray(level, np.float64).reshape(9)
    rc = B.load().lfx_grid_match_pose3(C.c_void_p(p2.ctypes.data), C.c_void_p(lv.ctypes.data if lv is not None else None), float(z),
                                       C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise B.LfxError(rc, "the pose is refused")
    return out.reshape(3, 4)


def write_occupancy_map(dirname, grid, resolution, origin=(0.0, 0.0), occupied_percent=65, free_percent=25):
    """lfx_occupancy_write_map: an int8 grid [height][width] (row 0 the lowest y) as dirname/map.pgm and dirname/map.yaml, the
    pair map_server reads.  Host only."""
    g = np.ascontiguousarray(grid, np.int8)
    if g.ndim != 2:
        raise ValueError("the grid must be [height][width]")
    rc = B.load().lfx_occupancy_write_map(os.fsencode(str(dirname)), C.c_void_p(g.ctypes.data if g.size else None), g.shape[1], g.shape[0],
                                          float(resolution), float(origin[0]), float(origin[1]), int(occupied_percent), int(free_percent))
    if rc != 0:
        raise B.LfxError(rc, "cannot write map.pgm / map.yaml in %s" % dirname)


def _msg_buffer():
    return C.create_string_buffer(512)


def read_pcd(path, drop_nonfinite=False, with_count=False):
    """lfx_pcd_read: the records ([n, 4] float32: x, y, z, 1.0) of a PCD file as pcl::io::loadPCDFile<pcl::PointXYZ> reads
    it (ascii, binary, binary_compressed).  drop_nonfinite: leave out records with a non-finite coordinate.  with_count:
    return (records, records with a non-finite coordinate).  Raises LfxError (LFX_ERR_FILE, LFX_ERR_UNSUPPORTED_FIELD)
    with the reader's message.  No device."""
    L = B.load()
    n, bad, msg = C.c_uint64(0), C.c_uint64(0), _msg_buffer()
    rc = L.lfx_pcd_read(os.fsencode(path), None, 0, int(bool(drop_nonfinite)), C.byref(n), C.byref(bad), msg, len(msg))
    if rc != 0:
        raise B.LfxError(rc, msg.value.decode(errors="replace"))
    out = np.zeros((max(int(n.value), 1), 4), np.float32)
    rc = L.lfx_pcd_read(os.fsencode(path), C.c_void_p(out.ctypes.data), len(out), int(bool(drop_nonfinite)), C.byref(n), C.byref(bad),
                        msg, len(msg))
    if rc != 0:
        raise B.LfxError(rc, msg.value.decode(errors="replace"))
    out = out[:int(n.value)]
    return (out, int(bad.value)) if with_count else out


def write_pcd(path, points):
    """lfx_pcd_write: records ([n, 4] or [n, 3] float32) as pcl::io::save writes a PointCloud<PointXYZ> (DATA binary).  No device."""
    p = np.asarray(points, np.float32)
    if p.ndim == 2 and p.shape[1] == 3:
        p = np.hstack([p, np.ones((len(p), 1), np.float32)])
    p = np.ascontiguousarray(p, np.float32).reshape(-1, 4)
    msg = _msg_buffer()
    rc = B.load().lfx_pcd_write(os.fsencode(path), C.c_void_p(p.ctypes.data), len(p), msg, len(msg))
    if rc != 0:
        raise B.LfxError(rc, msg.value.decode(errors="replace"))


def pose_diff(pose0, pose1):
    """lfx_pose_diff: (|d.translation()|, |Quaterniond(d.rotation()).vec()|) with d = pose0^-1 pose1 -- the two quantities
    PoseDiffIsSufficientlySmall (map.hpp:49-60) compares.  Poses 3 x 4 [R | t].  No device."""
    a = np.ascontiguousarray(pose0, np.float64).reshape(12)
    b = np.ascontiguousarray(pose1, np.float64).reshape(12)
    t, r = C.c_double(0), C.c_double(0)
    pd = C.POINTER(C.c_double)
    rc = B.load().lfx_pose_diff(a.ctypes.data_as(pd), b.ctypes.data_as(pd), C.byref(t), C.byref(r))
    if rc != 0:
        raise B.LfxError(rc, "invalid argument")
    return t.value, r.value


def covariance_ros(pose, covariance):
    """lfx_align_covariance_ros: a report's 6 x 6 covariance (rotation increment in the scan's frame first, then the translation
    in the map frame) in the order of geometry_msgs/PoseWithCovariance (x, y, z, rotation about the fixed X, Y, Z axes):
    T C T^T with T = [[0, I], [R, 0]], R the rotation of `pose` (3 x 4).  No device."""
    a = np.ascontiguousarray(pose, np.float64).reshape(12)
    c = np.ascontiguousarray(covariance, np.float64).reshape(36)
    out = np.zeros(36, np.float64)
    pd = C.POINTER(C.c_double)
    rc = B.load().lfx_align_covariance_ros(a.ctypes.data_as(pd), c.ctypes.data_as(pd), out.ctypes.data_as(pd))
    if rc != 0:
        raise B.LfxError(rc, "invalid argument")
    return out.reshape(6, 6)


def _download(L, ptr, n_records, stream=0):
    """n_records records of 4 floats from device address ptr (the HIP runtime liblfx.so is bound to)."""
    out = np.zeros((int(n_records), 4), np.float32)
    if n_records:
        L.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        L.hipStreamSynchronize.argtypes = [C.c_void_p]
        if L.hipMemcpyAsync(out.ctypes.data, int(ptr), out.nbytes, 2, C.c_void_p(int(stream))) != 0 or \
                L.hipStreamSynchronize(C.c_void_p(int(stream))) != 0:
            raise B.LfxError(-3, "cannot copy the map to the host")
    return out


class _Handle:
    """What the classes over an object of the library share: `handle` (set by their __init__, after _fx and _L), the check
    of a return code against the context's message, and close() -- the destroy call named by _destroy, once."""

    _destroy = None

    def _check(self, rc):
        B.check(self._fx._ctx, rc, self._L)

    def close(self):
        if self.handle:
            getattr(self._L, self._destroy)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ScanMap(_Handle):
    """lfx_map: the index a scan is matched against -- the place of the reference's KDTreeEigen (kdtree.hpp:50-71)."""

    _destroy = "lfx_map_destroy"

    def __init__(self, fx, d_points, n_points, cell_size=1.0, stream=0, host_points=None):
        self._fx = fx
        self._L = fx._L
        h = C.c_void_p()
        if host_points is not None:
            pts = np.ascontiguousarray(host_points, np.float32).reshape(-1, 4)
            B.check(fx._ctx, self._L.lfx_map_create_host(fx._ctx, C.c_void_p(pts.ctypes.data), len(pts), float(cell_size), C.byref(h),
                                                         C.c_void_p(int(stream))))
        else:
            B.check(fx._ctx, self._L.lfx_map_create(fx._ctx, C.c_void_p(int(d_points)), int(n_points), float(cell_size), C.byref(h),
                                                    C.c_void_p(int(stream))))
        self.handle = h

    @classmethod
    def from_pcd(cls, fx, path, cell_size=1.0, stream=0):
        """A map from a PCD file, as the localization node loads its maps (localization.cpp:78-85): read with
        lfx_pcd_read, records with a non-finite coordinate left out (lfx_map_create requires finite points)."""
        return cls(fx, 0, 0, cell_size, stream, host_points=read_pcd(path, drop_nonfinite=True))

    def info(self):
        n, cell, dims = C.c_uint32(), C.c_float(), (C.c_int32 * 3)()
        self._L.lfx_map_info(self.handle, C.byref(n), C.byref(cell), dims)
        return dict(n_points=n.value, cell_size=cell.value, dims=tuple(dims))

    def nearest(self, d_queries, n_queries, k, d_neighbours=0, d_squared_distances=0, d_indices=0, stream=0):
        """lfx_map_nearest: KDTreeEigen::NearestKSearch (src/kdtree.cpp:44-68) for a batch of queries on the device."""
        B.check(self._fx._ctx, self._L.lfx_map_nearest(
            self._fx._ctx, self.handle, C.c_void_p(int(d_queries)), int(n_queries), int(k), C.c_void_p(int(d_neighbours)),
            C.c_void_p(int(d_squared_distances)), C.c_void_p(int(d_indices)), C.c_void_p(int(stream))))


class Odometry(_Handle):
    """lfx_odometry: scan-to-local-map odometry -- Odometry<..., EdgeSurfaceMap, EdgeSurfaceScan> (odometry.hpp:52-63) with the
    store and the window maps on the device.  Poses are 3 x 4 [R | t] (point_to_map)."""

    _destroy = "lfx_odometry_destroy"

    def __init__(self, fx, reports=False, **config):
        self._fx = fx
        self._L = fx._L
        cfg = B.OdometryConfig()
        self._L.lfx_odometry_default_config(C.byref(cfg))
        for k, v in config.items():
            if k == "initial_pose":
                cfg.initial_pose[:] = [float(x) for x in np.asarray(v, np.float64).reshape(12)]
            elif k in dict(B.OdometryConfig._fields_):
                setattr(cfg, k, v)
            else:
                raise TypeError("unknown odometry setting %r" % k)
        h = C.c_void_p()
        B.check(fx._ctx, self._L.lfx_odometry_create(fx._ctx, C.byref(cfg), C.byref(h)))
        self.handle = h
        self.config = {k: getattr(cfg, k) for k, _ in B.OdometryConfig._fields_ if k != "initial_pose"}
        if reports:
            self.set_reports(True)

    def set_reports(self, on):
        """lfx_odometry_set_reports: keep an lfx_align_report per scan of every update* call (off by default)."""
        B.check(self._fx._ctx, self._L.lfx_odometry_set_reports(self.handle, int(bool(on))))

    def reports(self):
        """lfx_odometry_reports: the reports of the scans of the last update* call, one dict per scan (valid False for a scan
        that was not aligned); empty while reports are off."""
        n = C.c_uint32(0)
        B.check(self._fx._ctx, self._L.lfx_odometry_reports(self.handle, None, 0, C.byref(n)))
        reps = (B.AlignReport * max(n.value, 1))()
        B.check(self._fx._ctx, self._L.lfx_odometry_reports(self.handle, reps, n.value, C.byref(n)))
        return FeatureExtraction._align_reports(reps[:n.value])

    def _results(self, res):
        out = []
        for r, a in zip(res, self._fx._align_results([r.align for r in res])):
            a.update(n_edge_map=r.n_edge_map, n_surface_map=r.n_surface_map, aligned=bool(r.aligned))
            out.append(a)
        return out

    def update_batch(self, n_scans=None, stream=0):
        """lfx_odometry_update_batch: Odometry::Update for every scan of the last device batch; one dict per scan (the
        alignment's pose, error, error_scale, iteration, code, success, message, plus n_edge_map, n_surface_map, aligned)."""
        n = int(self._fx.device_view().batch if n_scans is None else n_scans)
        res = (B.OdometryResult * max(n, 1))()
        B.check(self._fx._ctx, self._L.lfx_odometry_update_batch(self._fx._ctx, self.handle, n, res, C.c_void_p(int(stream))))
        return self._results(res[:n])

    def update_batch_deskewed(self, time=None, sweep_times=None, sweep_ratio=1.0, to="end", n_scans=None, stream=0):
        """lfx_odometry_update_batch_deskewed: update_batch with every scan de-skewed by its own constant-velocity prediction
        (the motion between the last two poses, scaled by sweep_ratio) before it is aligned and added.  time as
        FeatureExtraction.deskew takes it; sweep_times: [n][2] = t0, t1 per scan with a time field.  The batch's clouds in
        the context stay raw."""
        n = int(self._fx.device_view().batch if n_scans is None else n_scans)
        tf = _time_field(time)
        st = None if sweep_times is None else np.ascontiguousarray(sweep_times, np.float64).reshape(-1)
        if st is not None and len(st) != 2 * n:
            raise ValueError("expected %d pairs of sweep times" % n)
        res = (B.OdometryResult * max(n, 1))()
        B.check(self._fx._ctx, self._L.lfx_odometry_update_batch_deskewed(
            self._fx._ctx, self.handle, C.byref(tf), None if st is None else _pd(st), float(sweep_ratio), _deskew_to(to), n, res,
            C.c_void_p(int(stream))))
        return self._results(res[:n])

    def update_batch_trajectory(self, time, trajectories, n_scans=None, stream=0):
        """lfx_odometry_update_batch_trajectory: update_batch with every scan de-skewed along the caller's trajectory of it
        (FeatureExtraction.deskew_trajectory's arguments) before it is aligned and added.  The batch's clouds in the context
        stay raw."""
        tf = _time_field(time)
        tr, n_tr, _keep = _trajectories(trajectories)
        n = int(n_tr if n_scans is None else n_scans)
        res = (B.OdometryResult * max(n, 1))()
        B.check(self._fx._ctx, self._L.lfx_odometry_update_batch_trajectory(
            self._fx._ctx, self.handle, C.byref(tf), tr, n, res, C.c_void_p(int(stream))))
        return self._results(res[:n])

    def update(self, d_edge, n_edge, d_surface, n_surface, stream=0):
        """lfx_odometry_update: Odometry::Update for one scan whose clouds (records of 4 floats) are on the device."""
        res = (B.OdometryResult * 1)()
        B.check(self._fx._ctx, self._L.lfx_odometry_update(
            self._fx._ctx, self.handle, C.c_void_p(int(d_edge)), int(n_edge), C.c_void_p(int(d_surface)), int(n_surface), res,
            C.c_void_p(int(stream))))
        return self._results(res)[0]

    def update_host(self, edge_points, surface_points, stream=0):
        """lfx_odometry_update_host: the same for clouds ([n][4] float32) on the host."""
        e = np.ascontiguousarray(edge_points, np.float32).reshape(-1, 4)
        sf = np.ascontiguousarray(surface_points, np.float32).reshape(-1, 4)
        res = (B.OdometryResult * 1)()
        B.check(self._fx._ctx, self._L.lfx_odometry_update_host(
            self._fx._ctx, self.handle, C.c_void_p(e.ctypes.data), len(e), C.c_void_p(sf.ctypes.data), len(sf), res,
            C.c_void_p(int(stream))))
        return self._results(res)[0]

    def add(self, pose, d_edge, n_edge, d_surface, n_surface, stream=0):
        """lfx_odometry_add: EdgeSurfaceMap::Add at a given pose (3 x 4); the current pose stays as it is."""
        pm = np.ascontiguousarray(pose, np.float64).reshape(12)
        B.check(self._fx._ctx, self._L.lfx_odometry_add(
            self._fx._ctx, self.handle, pm.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(int(d_edge)), int(n_edge),
            C.c_void_p(int(d_surface)), int(n_surface), C.c_void_p(int(stream))))

    def pose(self):
        """CurrentPose, 3 x 4."""
        out = np.zeros(12, np.float64)
        B.check(self._fx._ctx, self._L.lfx_odometry_pose(self.handle, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out.reshape(3, 4)

    def view(self):
        """lfx_odometry_view: device addresses and sizes of the store (GetAll) and the window (GetRecent), per-scan offsets
        (numpy copies), scans added / dropped, compactions, the current pose."""
        v = B.OdometryStoreView()
        B.check(self._fx._ctx, self._L.lfx_odometry_view(self.handle, C.byref(v)))
        n = v.n_scans
        return dict(n_scans=n, n_window_scans=v.n_window_scans, n_added=v.n_added, dropped_scans=v.dropped_scans,
                    compactions=v.compactions, edge_points=v.edge_points or 0, surface_points=v.surface_points or 0,
                    n_edge=v.n_edge, n_surface=v.n_surface, edge_window=v.edge_window or 0, surface_window=v.surface_window or 0,
                    n_edge_window=v.n_edge_window, n_surface_window=v.n_surface_window,
                    edge_offsets=np.array(v.edge_offsets[:n + 1], np.uint32), surface_offsets=np.array(v.surface_offsets[:n + 1], np.uint32),
                    pose=np.array(v.pose[:], np.float64).reshape(3, 4))

    def save(self, dirname, stream=0):
        """lfx_odometry_save: EdgeSurfaceMap::Save(dirname) -- dirname/edge.pcd and dirname/surface.pcd from the store, each only
        if non-empty.  Returns (edge written, surface written)."""
        w = (C.c_int32 * 2)()
        B.check(self._fx._ctx, self._L.lfx_odometry_save(self._fx._ctx, self.handle, os.fsencode(dirname), w, C.c_void_p(int(stream))))
        return bool(w[0]), bool(w[1])


class Mapper(_Handle):
    """lfx_mapper: MapBuilder<PointType> (map.hpp:95-153) with its map on the device -- per cloud: empty -> EMPTY; the pose too
    close to the last added pose (PoseDiffIsSufficientlySmall) -> TOO_CLOSE; else ADDED, the cloud transformed by its pose
    appended to the map.  Poses are 3 x 4 [R | t].  Outcomes: binding.KEYFRAME_ADDED / _EMPTY / _TOO_CLOSE."""

    _destroy = "lfx_mapper_destroy"

    def __init__(self, fx, **config):
        self._fx = fx
        self._L = fx._L
        cfg = B.MapperConfig()
        self._L.lfx_mapper_default_config(C.byref(cfg))
        for k, v in config.items():
            if k not in dict(B.MapperConfig._fields_):
                raise TypeError("unknown mapper setting %r" % k)
            setattr(cfg, k, v)
        h = C.c_void_p()
        B.check(fx._ctx, self._L.lfx_mapper_create(fx._ctx, C.byref(cfg), C.byref(h)))
        self.handle = h
        self.config = {k: getattr(cfg, k) for k, _ in B.MapperConfig._fields_}

    @staticmethod
    def _poses(poses, n):
        pm = np.ascontiguousarray(poses, np.float64).reshape(-1)
        if len(pm) != 12 * n:
            raise ValueError("expected %d poses of 3 x 4" % n)
        return pm

    def add(self, d_points, d_begin, d_count, count_stride, n_clouds, total_points, poses, stream=0):
        """lfx_mapper_add: MapBuilder::Callback for n_clouds device clouds (cloud s: d_count[s * count_stride] records from
        record d_begin[s] of d_points); poses [n][3][4].  Returns the outcomes (uint8 [n])."""
        n = int(n_clouds)
        pm = self._poses(poses, n)
        out = np.zeros(max(n, 1), np.uint8)
        B.check(self._fx._ctx, self._L.lfx_mapper_add(
            self._fx._ctx, self.handle, C.c_void_p(int(d_points)), C.c_void_p(int(d_begin)), C.c_void_p(int(d_count)), int(count_stride),
            n, int(total_points), pm.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(out.ctypes.data), C.c_void_p(int(stream))))
        return out[:n]

    def add_batch(self, which, poses, stream=0):
        """The edge ('edge') or surface ('surface') clouds of the last device batch, one pose per scan."""
        if which not in ("edge", "surface"):
            raise ValueError("which must be 'edge' or 'surface'")
        v = self._fx.device_view()
        pts = v.edge_points if which == "edge" else v.surface_points
        info = int(v.scan_info) + 4 * (2 if which == "edge" else 3)
        # (the batch's clouds lie inside the context's cloud buffers: max_points_per_scan x max_batch records)
        return self.add(pts, v.scan_begin, info, 4, v.batch, self._fx.max_points_per_scan * self._fx.max_batch, poses, stream)

    def add_host(self, points, pose, stream=0):
        """lfx_mapper_add_host: one cloud ([n, 4] float32) on the host.  Returns its outcome."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
        pm = self._poses(pose, 1)
        out = C.c_uint8(0)
        B.check(self._fx._ctx, self._L.lfx_mapper_add_host(
            self._fx._ctx, self.handle, C.c_void_p(p.ctypes.data if len(p) else 0), len(p), pm.ctypes.data_as(C.POINTER(C.c_double)),
            C.byref(out), C.c_void_p(int(stream))))
        return int(out.value)

    def view(self):
        """lfx_mapper_view: the map's device address and size, the counters, the last added pose."""
        v = B.MapperStoreView()
        B.check(self._fx._ctx, self._L.lfx_mapper_view(self.handle, C.byref(v)))
        return dict(points=v.points or 0, n_points=v.n_points, capacity_points=v.capacity_points, n_added=v.n_added,
                    n_empty=v.n_empty, n_too_close=v.n_too_close, has_pose=bool(v.has_pose),
                    last_pose=np.array(v.last_pose[:], np.float64).reshape(3, 4))

    def points(self, stream=0):
        """The map ([n, 4] float32) copied to the host after `stream`."""
        v = self.view()
        return _download(self._L, v["points"], v["n_points"], stream)

    def save(self, path, stream=0):
        """lfx_mapper_save: SaveMap -- nothing for an empty map.  Returns whether a file was written."""
        w = C.c_int32(0)
        B.check(self._fx._ctx, self._L.lfx_mapper_save(self._fx._ctx, self.handle, os.fsencode(path), C.byref(w), C.c_void_p(int(stream))))
        return bool(w.value)


class RollingMap(_Handle):
    """lfx_rolling_map: one point per voxel in a window that follows the vehicle, an edge store and a surface store (kind:
    'edge' / 'surface' or binding.ROLLING_EDGE / ROLLING_SURFACE).  Inserts keep the first point of a voxel (lowest (cloud,
    index) of the call that first reaches it); extract cuts a box out in ascending (vz, vy, vx).  Poses are 3 x 4 [R | t]."""

    _destroy = "lfx_rolling_map_destroy"

    KINDS = {"edge": B.ROLLING_EDGE, "surface": B.ROLLING_SURFACE}

    def __init__(self, fx, **config):
        self._fx = fx
        self._L = fx._L
        cfg = B.RollingMapConfig()
        self._L.lfx_rolling_map_default_config(C.byref(cfg))
        for k, v in config.items():
            if k not in dict(B.RollingMapConfig._fields_):
                raise TypeError("unknown rolling map setting %r" % k)
            if k.endswith("_dims"):
                v = (C.c_uint32 * 3)(*[int(x) for x in v])
            elif k == "match_half_extent":
                v = (C.c_float * 3)(*[float(x) for x in v])
            elif k == "initial_pose":
                v = (C.c_double * 12)(*[float(x) for x in np.asarray(v, np.float64).reshape(12)])
            setattr(cfg, k, v)
        h = C.c_void_p()
        B.check(fx._ctx, self._L.lfx_rolling_map_create(fx._ctx, C.byref(cfg), C.byref(h)))
        self.handle = h
        self.config = {k: (tuple(getattr(cfg, k)) if hasattr(getattr(cfg, k), "__len__") else getattr(cfg, k))
                       for k, _ in B.RollingMapConfig._fields_ if k != "initial_pose"}

    @classmethod
    def _kind(cls, kind):
        return cls.KINDS[kind] if isinstance(kind, str) else int(kind)

    def recenter(self, center):
        """lfx_rolling_map_recenter: both windows centred on `center` (m).  No device work."""
        ctr = np.ascontiguousarray(center, np.float64).reshape(3)
        rc = self._L.lfx_rolling_map_recenter(self.handle, ctr.ctypes.data_as(C.POINTER(C.c_double)))
        if rc != 0:
            raise B.LfxError(rc, "the centre must be finite and have a voxel")

    def insert(self, kind, d_points, d_begin, d_count, count_stride, n_clouds, total_points, poses, stream=0):
        """lfx_rolling_map_insert: n_clouds device clouds (lfx_mapper_add's addressing), poses [n][3][4]."""
        n = int(n_clouds)
        pm = Mapper._poses(poses, n)
        B.check(self._fx._ctx, self._L.lfx_rolling_map_insert(
            self._fx._ctx, self.handle, self._kind(kind), C.c_void_p(int(d_points)), C.c_void_p(int(d_begin)), C.c_void_p(int(d_count)),
            int(count_stride), n, int(total_points), pm.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(int(stream))))

    def insert_batch(self, kind, poses, stream=0):
        """The edge or surface clouds of the last device batch, one pose per scan."""
        k = self._kind(kind)
        v = self._fx.device_view()
        pts = v.edge_points if k == B.ROLLING_EDGE else v.surface_points
        info = int(v.scan_info) + 4 * (2 if k == B.ROLLING_EDGE else 3)
        self.insert(k, pts, v.scan_begin, info, 4, v.batch, self._fx.max_points_per_scan * self._fx.max_batch, poses, stream)

    def insert_host(self, kind, points, pose=None, stream=0):
        """lfx_rolling_map_insert_host: one cloud ([n, 4] float32) on the host (pose: identity)."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
        pm = Mapper._poses(np.eye(4)[:3] if pose is None else pose, 1)
        B.check(self._fx._ctx, self._L.lfx_rolling_map_insert_host(
            self._fx._ctx, self.handle, self._kind(kind), C.c_void_p(p.ctypes.data if len(p) else 0), len(p),
            pm.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(int(stream))))

    def extract_device(self, kind, lo, hi, d_out, capacity_points, stream=0):
        """lfx_rolling_map_extract into device memory (d_out: an address, capacity_points records of 4 floats).  Returns the
        number of live voxels in the box, whatever the capacity."""
        lo_, hi_ = (np.ascontiguousarray(a, np.float64).reshape(3) for a in (lo, hi))
        n = C.c_uint64(0)
        pd = C.POINTER(C.c_double)
        B.check(self._fx._ctx, self._L.lfx_rolling_map_extract(
            self._fx._ctx, self.handle, self._kind(kind), lo_.ctypes.data_as(pd), hi_.ctypes.data_as(pd), C.c_void_p(int(d_out)),
            int(capacity_points), C.byref(n), C.c_void_p(int(stream))))
        return int(n.value)

    def extract(self, kind, lo, hi, stream=0):
        """The live voxels of the box lo .. hi (m) as [n, 4] float32 on the host, ascending (vz, vy, vx)."""
        import torch
        n = self.extract_device(kind, lo, hi, 0, 0, stream)
        if n == 0:
            return np.zeros((0, 4), np.float32)
        out = torch.empty((n, 4), dtype=torch.float32, device=torch.device("cuda", self._fx.device))
        self.extract_device(kind, lo, hi, out.data_ptr(), n, stream)
        return _download(self._L, out.data_ptr(), n, stream)

    def view(self, stream=0):
        """lfx_rolling_map_view: per kind leaf, dims, origin, the counters summed since create and the live voxels."""
        v = B.RollingMapView()
        B.check(self._fx._ctx, self._L.lfx_rolling_map_view(self._fx._ctx, self.handle, C.byref(v), C.c_void_p(int(stream))))
        out = {name: dict(leaf=v.leaf[k], dims=tuple(v.dims[k]), origin=tuple(v.origin[k]), inserted=v.n_inserted[k],
                          merged=v.n_merged[k], outside=v.n_outside[k], nonfinite=v.n_nonfinite[k], live=v.n_live[k])
               for name, k in self.KINDS.items()}
        out["pose"] = np.array(v.pose[:], np.float64).reshape(3, 4)
        out["correction"] = np.array(v.correction[:], np.float64).reshape(3, 4)
        return out

    def update_batch(self, odometry_poses=None, n_scans=None, stream=0):
        """lfx_rolling_map_update_batch: LOAM's mapping stage for every scan of the last device batch -- the scan aligned
        against the boxes cut out of both stores around C x odometry_poses[k] (or the current pose), then inserted at the
        result.  One dict per scan: the alignment's fields plus initial_pose, n_edge_map, n_surface_map, aligned, inserted,
        recentered."""
        n = int(self._fx.device_view().batch if n_scans is None else n_scans)
        poses = None if odometry_poses is None else Mapper._poses(odometry_poses, n)
        res = (B.RollingMapResult * max(n, 1))()
        B.check(self._fx._ctx, self._L.lfx_rolling_map_update_batch(
            self._fx._ctx, self.handle, n, None if poses is None else poses.ctypes.data_as(C.POINTER(C.c_double)), res,
            C.c_void_p(int(stream))))
        out = []
        for r, a in zip(res[:n], self._fx._align_results([r.align for r in res[:n]])):
            a.update(initial_pose=np.array(r.initial_pose[:], np.float64).reshape(3, 4), n_edge_map=r.n_edge_map,
                     n_surface_map=r.n_surface_map, aligned=bool(r.aligned), inserted=bool(r.inserted), recentered=bool(r.recentered))
            out.append(a)
        return out

    def pose(self):
        """lfx_rolling_map_pose: the current pose (3 x 4)."""
        p = np.zeros(12, np.float64)
        B.check(self._fx._ctx, self._L.lfx_rolling_map_pose(self.handle, p.ctypes.data_as(C.POINTER(C.c_double))))
        return p.reshape(3, 4)

    def save(self, dirname, stream=0):
        """lfx_rolling_map_save: edge.pcd and surface.pcd of the whole windows under dirname.  Returns (edge written,
        surface written)."""
        w = (C.c_int32 * 2)()
        B.check(self._fx._ctx, self._L.lfx_rolling_map_save(self._fx._ctx, self.handle, os.fsencode(dirname), w, C.c_void_p(int(stream))))
        return bool(w[0]), bool(w[1])


class PlaceDb(_Handle):
    """lfx_place_db: scan-context descriptors of one config on the device, compared with a query under every column shift.
    Entries are numbered in insertion order.  A match is a dict: entry (None where the range held fewer than k entries),
    shift, distance, yaw -- a sensor that revisits the entry's place turned by +yaw about z gives that shift, so the revisit's
    initial pose is the entry's pose times Rz(yaw)."""

    _destroy = "lfx_place_db_destroy"

    def __init__(self, fx, capacity, config=None):
        self._fx = fx
        self._L = fx._L
        self.config = scan_context_config(config)
        self.shape = (int(self.config.n_rings), int(self.config.n_sectors))
        h = C.c_void_p()
        B.check(fx._ctx, self._L.lfx_place_db_create(fx._ctx, C.byref(self.config), int(capacity), C.byref(h)), self._L)
        self.handle = h
        self.capacity = int(capacity)

    def add(self, d_desc, n, stream=0):
        """lfx_place_db_add: n descriptors ([n][R][S] float32) at device address d_desc (or a device tensor), appended."""
        ptr = d_desc.data_ptr() if hasattr(d_desc, "data_ptr") else int(d_desc)
        B.check(self._fx._ctx, self._L.lfx_place_db_add(self._fx._ctx, self.handle, C.c_void_p(ptr or None), int(n), C.c_void_p(int(stream))),
                self._L)

    def add_host(self, desc, stream=0):
        """lfx_place_db_add_host: descriptors ([n][R][S] float32) on the host, appended."""
        d = np.ascontiguousarray(desc, np.float32).reshape((-1,) + self.shape)
        B.check(self._fx._ctx, self._L.lfx_place_db_add_host(
            self._fx._ctx, self.handle, C.c_void_p(d.ctypes.data if len(d) else None), len(d), C.c_void_p(int(stream))), self._L)

    def __len__(self):
        n = C.c_uint32(0)
        B.check(self._fx._ctx, self._L.lfx_place_db_size(self.handle, C.byref(n)), self._L)
        return int(n.value)

    def download(self, first=0, count=None, stream=0):
        """lfx_place_db_download: entries first .. first + count - 1 ([count][R][S] float32) on the host."""
        count = len(self) - int(first) if count is None else int(count)
        out = np.zeros((max(count, 0),) + self.shape, np.float32)
        B.check(self._fx._ctx, self._L.lfx_place_db_download(
            self._fx._ctx, self.handle, int(first), count, C.c_void_p(out.ctypes.data if out.size else None), C.c_void_p(int(stream))), self._L)
        return out

    def query_raw(self, d_desc, n_queries, k=1, first=0, count=None, stream=0):
        """lfx_place_db_query as it returns: a B.PlaceMatch array [n_queries * k]."""
        ptr = d_desc.data_ptr() if hasattr(d_desc, "data_ptr") else int(d_desc)
        count = len(self) - int(first) if count is None else int(count)
        res = (B.PlaceMatch * max(int(n_queries) * int(k), 1))()
        B.check(self._fx._ctx, self._L.lfx_place_db_query(
            self._fx._ctx, self.handle, C.c_void_p(ptr or None), int(n_queries), int(first), count, int(k), res, C.c_void_p(int(stream))),
            self._L)
        return res

    def query(self, d_desc, n_queries, k=1, first=0, count=None, stream=0):
        """The k (1 .. 16) best of entries [first, first + count) for each of n_queries descriptors on the device: a list per
        query of k dicts, ascending distance, equal distances by the lower entry.  Synchronous."""
        res = self.query_raw(d_desc, n_queries, k, first, count, stream)
        k = int(k)
        return [[_match(m) for m in res[q * k:(q + 1) * k]] for q in range(int(n_queries))]

    def query_gated_raw(self, d_desc, gates, d_poses=0, radius=float("inf"), k=1, stream=0):
        """lfx_place_db_query_gated as it returns: (a B.PlaceMatch array [len(gates) * k], n_eligible uint32 [len(gates)]).
        gates: (limit, pose) pairs, pose None = B.PLACE_NO_POSE; d_poses: the device address of [.][12] float64 (or a device
        tensor), 0 = no position test."""
        ptr = d_desc.data_ptr() if hasattr(d_desc, "data_ptr") else int(d_desc)
        pp = d_poses.data_ptr() if hasattr(d_poses, "data_ptr") else int(d_poses or 0)
        g = (B.PlaceGate * max(len(gates), 1))(*[B.PlaceGate(int(lim), B.PLACE_NO_POSE if pose is None else int(pose)) for lim, pose in gates])
        res = (B.PlaceMatch * max(len(gates) * int(k), 1))()
        n_eligible = np.zeros(max(len(gates), 1), np.uint32)
        B.check(self._fx._ctx, self._L.lfx_place_db_query_gated(
            self._fx._ctx, self.handle, C.c_void_p(ptr or None), len(gates), g, C.c_void_p(pp or None), float(radius), int(k), res,
            n_eligible.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_void_p(int(stream))), self._L)
        return res, n_eligible[:len(gates)]

    def query_gated(self, d_desc, gates, d_poses=0, radius=float("inf"), k=1, stream=0):
        """The k best ELIGIBLE entries for each query: entry e is eligible for query q iff e < gates[q][0] and, where d_poses is
        given and gates[q][1] is not None, the translation of d_poses[e] lies within `radius` of that of d_poses[gates[q][1]].
        Returns (a list per query of k dicts as query gives them, n_eligible per query).  Synchronous."""
        res, n_eligible = self.query_gated_raw(d_desc, gates, d_poses, radius, k, stream)
        k = int(k)
        return [[_match(m) for m in res[q * k:(q + 1) * k]] for q in range(len(gates))], [int(n) for n in n_eligible]


def _match(m):
    """lfx_place_match as a dict (entry None: the empty match)"""
    return dict(entry=None if m.entry == B.PLACE_NO_ENTRY else int(m.entry), shift=int(m.shift), distance=float(m.distance), yaw=float(m.yaw))


def pose_graph_config(config=None, **fields):
    """lfx_pose_graph_config: the defaults (lfx_pose_graph_default_config) with the given fields replaced.  config: None, a
    dict of fields, or a B.PoseGraphConfig (copied)."""
    return _config(B.PoseGraphConfig, "lfx_pose_graph_default_config", "pose-graph", config, fields)


def edge_information(pose_j, report_information):
    """lfx_pose_graph_edge_information: an alignment report's information ([6][6]; a in the scan's frame, b in the map frame)
    in a pose-graph edge's residual coordinates, B H B^T with B = blkdiag(I, R_j^T).  Host only."""
    p = np.ascontiguousarray(pose_j, np.float64).reshape(12)
    h = np.ascontiguousarray(report_information, np.float64).reshape(36)
    out = np.zeros(36)
    rc = B.load().lfx_pose_graph_edge_information(C.c_void_p(p.ctypes.data), C.c_void_p(h.ctypes.data), C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise B.LfxError(rc, "lfx_pose_graph_edge_information")
    return out.reshape(6, 6)


def relative_covariance(pose_i, pose_j, joint):
    """lfx_pose_graph_relative_covariance: the covariance [6][6] of the residual of an edge (i, j, Z = T_i^-1 T_j) at the current
    poses, from the pair's [12][12] block of PoseGraph.joint_covariances.  Its inverse gates a loop candidate.  Host only."""
    pi = np.ascontiguousarray(pose_i, np.float64).reshape(12)
    pj = np.ascontiguousarray(pose_j, np.float64).reshape(12)
    s = np.ascontiguousarray(joint, np.float64).reshape(144)
    out = np.zeros(36)
    rc = B.load().lfx_pose_graph_relative_covariance(C.c_void_p(pi.ctypes.data), C.c_void_p(pj.ctypes.data), C.c_void_p(s.ctypes.data),
                                                     C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise B.LfxError(rc, "lfx_pose_graph_relative_covariance")
    return out.reshape(6, 6)


def pose_graph_edges(i, j, z, information, flags=0):
    """Edges as the records lfx_pose_graph_add_edges takes (B.POSE_GRAPH_EDGE_DTYPE): i, j [n], z [n][3][4] or [n][12],
    information [n][6][6], flags one value or [n]."""
    i = np.atleast_1d(np.asarray(i))
    e = np.zeros(len(i), B.POSE_GRAPH_EDGE_DTYPE)
    e["i"], e["j"], e["flags"] = i, np.atleast_1d(np.asarray(j)), flags
    e["z"] = np.asarray(z, np.float64).reshape(len(i), 12)
    e["information"] = np.asarray(information, np.float64).reshape(len(i), 36)
    return e


def pose_graph_priors(node, z, information, lever=None, position=False, robust=False):
    """Priors as the records lfx_pose_graph_add_priors takes (B.POSE_GRAPH_PRIOR_DTYPE): node [n]; position False: z [n][3][4]
    or [n][12], information [n][6][6]; position True: z [n][3] (the fix) or [n][12], information [n][3][3] (placed in the
    lower right block) or [n][6][6], lever [n][3] or one [3] (None: zero).  position and robust: one value or [n]."""
    node = np.atleast_1d(np.asarray(node))
    n = len(node)
    p = np.zeros(n, B.POSE_GRAPH_PRIOR_DTYPE)
    position = np.broadcast_to(np.asarray(position, bool), (n,))
    p["node"] = node
    p["flags"] = np.where(position, B.PRIOR_POSITION, 0) | np.where(np.broadcast_to(np.asarray(robust, bool), (n,)), B.PRIOR_ROBUST, 0)
    z = np.asarray(z, np.float64).reshape(n, -1)
    if z.shape[1] == 3:
        p["z"][:, [3, 7, 11]] = z
    else:
        p["z"] = z.reshape(n, 12)
    om = np.asarray(information, np.float64).reshape(n, -1)
    if om.shape[1] == 9:
        full = np.zeros((n, 6, 6))
        full[:, 3:, 3:] = om.reshape(n, 3, 3)
        om = full.reshape(n, 36)
    p["information"] = om.reshape(n, 36)
    if lever is not None:
        p["lever"] = np.broadcast_to(np.asarray(lever, np.float64), (n, 3))
    return p


class PoseGraph(_Handle):
    """lfx_pose_graph: poses (nodes) and relative-pose measurements (edges) on the device, optimised there by Gauss-Newton with
    the chain-and-loop solver (include/lfx.h, the pose graph section).  Poses are [3][4] = [R | t] float64; node 0 is fixed
    unless release_first frees it.  Absolute fixes of single nodes are priors: reserve_priors once, then add_priors."""

    _destroy = "lfx_pose_graph_destroy"

    def __init__(self, fx, max_nodes, max_edges, config=None, **fields):
        self._fx = fx
        self._L = fx._L
        self.config = pose_graph_config(config, max_nodes=int(max_nodes), max_edges=int(max_edges), **fields)
        h = C.c_void_p()
        B.check(fx._ctx, self._L.lfx_pose_graph_create(fx._ctx, C.byref(self.config), C.byref(h)), self._L)
        self.handle = h

    def info(self):
        i = B.PoseGraphInfo()
        self._check(self._L.lfx_pose_graph_info(self.handle, C.byref(i)))
        return dict(n_nodes=int(i.n_nodes), n_edges=int(i.n_edges), n_chain=int(i.n_chain), n_loop=int(i.n_loop),
                    device_bytes=int(i.device_bytes))

    def __len__(self):
        return self.info()["n_nodes"]

    def add_nodes(self, poses, stream=0):
        """lfx_pose_graph_add_nodes: poses [n][3][4] appended; the id of the first."""
        p = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        first = C.c_uint32(0)
        self._check(self._L.lfx_pose_graph_add_nodes(self._fx._ctx, self.handle, C.c_void_p(p.ctypes.data if len(p) else None), len(p),
                                                     C.byref(first), C.c_void_p(int(stream))))
        return int(first.value)

    def set_fixed(self, node, fixed=True, stream=0):
        self._check(self._L.lfx_pose_graph_set_fixed(self._fx._ctx, self.handle, int(node), int(bool(fixed)), C.c_void_p(int(stream))))

    def add_edges(self, edges, stream=0):
        """lfx_pose_graph_add_edges: records of B.POSE_GRAPH_EDGE_DTYPE (pose_graph_edges builds them)."""
        e = np.ascontiguousarray(edges, B.POSE_GRAPH_EDGE_DTYPE).reshape(-1)
        self._check(self._L.lfx_pose_graph_add_edges(self._fx._ctx, self.handle, C.c_void_p(e.ctypes.data if len(e) else None), len(e),
                                                     C.c_void_p(int(stream))))

    def add_edge(self, i, j, z, information, robust=False, stream=0):
        self.add_edges(pose_graph_edges([i], [j], [z], [information], B.EDGE_ROBUST if robust else 0), stream)

    def optimize(self, stream=0):
        """lfx_pose_graph_optimize: a dict of the result's fields (code: B.POSE_GRAPH_*).  Synchronous."""
        r = B.PoseGraphResult()
        self._check(self._L.lfx_pose_graph_optimize(self._fx._ctx, self.handle, C.byref(r), C.c_void_p(int(stream))))
        return dict(code=int(r.code), iterations=int(r.iterations), chi2_initial=float(r.chi2_initial), chi2_final=float(r.chi2_final),
                    max_step=float(r.max_step), n_chain=int(r.n_chain), n_loop=int(r.n_loop),
                    n_robust_downweighted=int(r.n_robust_downweighted))

    def poses(self, first=0, count=None, stream=0):
        """lfx_pose_graph_poses: nodes first .. first + count - 1 as [count][3][4] float64 on the host."""
        count = len(self) - int(first) if count is None else int(count)
        out = np.zeros((max(count, 0), 3, 4))
        self._check(self._L.lfx_pose_graph_poses(self._fx._ctx, self.handle, int(first), count, C.c_void_p(out.ctypes.data if out.size else None),
                                                 C.c_void_p(int(stream))))
        return out

    def set_poses(self, poses, first=0, stream=0):
        p = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        self._check(self._L.lfx_pose_graph_set_poses(self._fx._ctx, self.handle, int(first), len(p), C.c_void_p(p.ctypes.data if len(p) else None),
                                                     C.c_void_p(int(stream))))

    def view(self, stream=0):
        """lfx_pose_graph_view: (device address of [n_nodes][12] float64, n_nodes), current behind `stream`."""
        ptr, n = C.c_void_p(), C.c_uint32(0)
        self._check(self._L.lfx_pose_graph_view(self._fx._ctx, self.handle, C.byref(ptr), C.byref(n), C.c_void_p(int(stream))))
        return int(ptr.value or 0), int(n.value)

    def edge_chi2(self, first=0, count=None, stream=0):
        """lfx_pose_graph_edge_chi2: (rho [count], w [count]) at the poses the last optimize left."""
        count = self.info()["n_edges"] - int(first) if count is None else int(count)
        rho, w = np.zeros(max(count, 0)), np.zeros(max(count, 0))
        self._check(self._L.lfx_pose_graph_edge_chi2(self._fx._ctx, self.handle, int(first), count, C.c_void_p(rho.ctypes.data if count else None),
                                                     C.c_void_p(w.ctypes.data if count else None), C.c_void_p(int(stream))))
        return rho, w

    def reserve_priors(self, max_priors):
        """lfx_pose_graph_reserve_priors: room for max_priors priors; once, before the first prior."""
        self._check(self._L.lfx_pose_graph_reserve_priors(self._fx._ctx, self.handle, int(max_priors)))

    def add_priors(self, priors, stream=0):
        """lfx_pose_graph_add_priors: records of B.POSE_GRAPH_PRIOR_DTYPE (pose_graph_priors builds them)."""
        p = np.ascontiguousarray(priors, B.POSE_GRAPH_PRIOR_DTYPE).reshape(-1)
        self._check(self._L.lfx_pose_graph_add_priors(self._fx._ctx, self.handle, C.c_void_p(p.ctypes.data if len(p) else None), len(p),
                                                      C.c_void_p(int(stream))))

    def add_prior(self, node, z, information, lever=None, position=False, robust=False, stream=0):
        self.add_priors(pose_graph_priors([node], [z], [information], None if lever is None else [lever], position, robust), stream)

    def release_first(self, released=True, stream=0):
        """lfx_pose_graph_release_first: node 0 free (unless set_fixed(0) holds it), or fixed again."""
        self._check(self._L.lfx_pose_graph_release_first(self._fx._ctx, self.handle, int(bool(released)), C.c_void_p(int(stream))))

    def prior_chi2(self, first=0, count=None, stream=0):
        """lfx_pose_graph_prior_chi2: (rho [count], w [count]) at the poses the last optimize left."""
        count = self.prior_info()["n_priors"] - int(first) if count is None else int(count)
        rho, w = np.zeros(max(count, 0)), np.zeros(max(count, 0))
        self._check(self._L.lfx_pose_graph_prior_chi2(self._fx._ctx, self.handle, int(first), count, C.c_void_p(rho.ctypes.data if count else None),
                                                      C.c_void_p(w.ctypes.data if count else None), C.c_void_p(int(stream))))
        return rho, w

    def reserve_marginals(self):
        """lfx_pose_graph_reserve_marginals: room for the covariances; once."""
        self._check(self._L.lfx_pose_graph_reserve_marginals(self._fx._ctx, self.handle))

    def marginals(self, first=0, count=None, stream=0, out=None, return_code=False):
        """lfx_pose_graph_marginals: Sigma_kk of nodes first .. first + count - 1 as [count][6][6] float64, over the increments
        (a, b) of include/lfx.h.  A matrix that is not positive definite raises B.LfxError unless return_code, which returns
        (array, code) with the array (`out`, where given) untouched."""
        count = len(self) - int(first) if count is None else int(count)
        out = np.zeros((max(count, 0), 6, 6)) if out is None else out
        code = C.c_int(0)
        self._check(self._L.lfx_pose_graph_marginals(self._fx._ctx, self.handle, int(first), count, C.c_void_p(out.ctypes.data if out.size else None),
                                                     C.byref(code), C.c_void_p(int(stream))))
        return self._coded(out, code, return_code)

    def joint_covariances(self, pairs, stream=0, out=None, return_code=False):
        """lfx_pose_graph_joint_covariances: pairs [n][2] -> [n][12][12] float64, [[Sigma_ii, Sigma_ij], [Sigma_ji, Sigma_jj]]."""
        p = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
        out = np.zeros((len(p), 12, 12)) if out is None else out
        code = C.c_int(0)
        self._check(self._L.lfx_pose_graph_joint_covariances(self._fx._ctx, self.handle, C.c_void_p(p.ctypes.data if len(p) else None), len(p),
                                                             C.c_void_p(out.ctypes.data if out.size else None), C.byref(code), C.c_void_p(int(stream))))
        return self._coded(out, code, return_code)

    @staticmethod
    def _coded(out, code, return_code):
        if return_code:
            return out, int(code.value)
        if code.value != B.POSE_GRAPH_CONVERGED:
            raise B.LfxError(B.ERR_INVALID_ARGUMENT, "H + lambda I is not positive definite")
        return out

    def prior_info(self):
        i = B.PoseGraphPriorInfo()
        self._check(self._L.lfx_pose_graph_prior_info(self.handle, C.byref(i)))
        return dict(n_priors=int(i.n_priors), max_priors=int(i.max_priors), n_downweighted=int(i.n_downweighted), reserved=int(i.reserved),
                    chi2=float(i.chi2))


class Keyframes(_Handle):
    """lfx_keyframes: every keyframe's edge and surface records on the device in the SENSOR frame with one pose per keyframe,
    and world clouds written from the two at the poses of the moment (include/lfx.h, the keyframe store section) -- what makes
    a map follow a pose graph.  kind: 'edge' / 'surface' (or B.KEYFRAMES_EDGE / _SURFACE).  Poses are [3][4] = [R | t] float64;
    keyframe ids count from 0 in order of addition."""

    _destroy = "lfx_keyframes_destroy"

    KINDS = {"edge": B.KEYFRAMES_EDGE, "surface": B.KEYFRAMES_SURFACE, B.KEYFRAMES_EDGE: B.KEYFRAMES_EDGE, B.KEYFRAMES_SURFACE: B.KEYFRAMES_SURFACE}

    def __init__(self, fx, max_keyframes, max_points):
        self._fx = fx
        self._L = fx._L
        cfg = B.KeyframesConfig()
        self._L.lfx_keyframes_default_config(C.byref(cfg))
        cfg.max_keyframes = int(max_keyframes)
        mp = (max_points, max_points) if np.isscalar(max_points) else tuple(max_points)
        cfg.max_points[0], cfg.max_points[1] = int(mp[0]), int(mp[1])
        h = C.c_void_p()
        B.check(fx._ctx, self._L.lfx_keyframes_create(fx._ctx, C.byref(cfg), C.byref(h)), self._L)
        self.handle = h
        self.config = cfg

    @classmethod
    def _kind(cls, kind):
        if kind not in cls.KINDS:
            raise ValueError("kind must be 'edge' or 'surface'")
        return cls.KINDS[kind]

    def info(self):
        i = B.KeyframesInfo()
        self._check(self._L.lfx_keyframes_info(self.handle, C.byref(i)))
        return dict(n_keyframes=int(i.n_keyframes), max_keyframes=int(i.max_keyframes), n_points=(int(i.n_points[0]), int(i.n_points[1])),
                    max_points=(int(i.max_points[0]), int(i.max_points[1])), device_bytes=int(i.device_bytes))

    def __len__(self):
        return self.info()["n_keyframes"]

    def view(self, stream=0):
        """lfx_keyframes_view: the device addresses of the records and begin tables ([0] edge, [1] surface) and of the poses,
        current behind `stream`, and the host's counts."""
        v = B.KeyframesStoreView()
        self._check(self._L.lfx_keyframes_view(self._fx._ctx, self.handle, C.byref(v), C.c_void_p(int(stream))))
        return dict(points=(v.points[0] or 0, v.points[1] or 0), begin=(v.begin[0] or 0, v.begin[1] or 0), poses=v.poses or 0,
                    n_keyframes=int(v.n_keyframes), n_points=(int(v.n_points[0]), int(v.n_points[1])))

    @staticmethod
    def clouds(d_points, d_begin, d_count, count_stride, total_points):
        """lfx_keyframes_clouds: device clouds addressed as Mapper.add addresses them."""
        return B.KeyframesClouds(C.c_void_p(int(d_points)), C.c_void_p(int(d_begin)), C.c_void_p(int(d_count)), int(count_stride), 0, int(total_points))

    def add(self, edge, surface, poses, stream=0):
        """lfx_keyframes_add: edge and surface are Keyframes.clouds(...) of n clouds each, poses [n][3][4]; the id of the first
        keyframe added."""
        pm = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        first = C.c_uint32(0)
        self._check(self._L.lfx_keyframes_add(self._fx._ctx, self.handle, C.byref(edge), C.byref(surface), len(pm),
                                              C.c_void_p(pm.ctypes.data if len(pm) else None), C.byref(first), C.c_void_p(int(stream))))
        return int(first.value)

    def add_batch(self, poses, stream=0):
        """Both clouds of every scan of the last device batch, one pose per scan (as Mapper.add_batch takes one kind)."""
        v = self._fx.device_view()
        cap = self._fx.max_points_per_scan * self._fx.max_batch
        info = int(v.scan_info)
        pm = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        if len(pm) != v.batch:
            raise ValueError("expected %d poses of 3 x 4" % v.batch)
        return self.add(self.clouds(v.edge_points, v.scan_begin, info + 8, 4, cap), self.clouds(v.surface_points, v.scan_begin, info + 12, 4, cap),
                        pm, stream)

    def add_host(self, edge_points, surface_points, pose, stream=0):
        """lfx_keyframes_add_host: one keyframe from host clouds ([n, 4] float32 each, either may be empty); its id."""
        e = np.ascontiguousarray(edge_points, np.float32).reshape(-1, 4)
        s = np.ascontiguousarray(surface_points, np.float32).reshape(-1, 4)
        pm = np.ascontiguousarray(pose, np.float64).reshape(12)
        kid = C.c_uint32(0)
        self._check(self._L.lfx_keyframes_add_host(
            self._fx._ctx, self.handle, C.c_void_p(e.ctypes.data if len(e) else None), len(e), C.c_void_p(s.ctypes.data if len(s) else None), len(s),
            C.c_void_p(pm.ctypes.data), C.byref(kid), C.c_void_p(int(stream))))
        return int(kid.value)

    def set_poses(self, poses, first=0, stream=0):
        p = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        self._check(self._L.lfx_keyframes_set_poses(self._fx._ctx, self.handle, int(first), len(p), C.c_void_p(p.ctypes.data if len(p) else None),
                                                    C.c_void_p(int(stream))))

    def poses(self, first=0, count=None, stream=0):
        """lfx_keyframes_poses: keyframes first .. first + count - 1 as [count][3][4] float64 on the host."""
        count = len(self) - int(first) if count is None else int(count)
        out = np.zeros((max(count, 0), 3, 4))
        self._check(self._L.lfx_keyframes_poses(self._fx._ctx, self.handle, int(first), count, C.c_void_p(out.ctypes.data if out.size else None),
                                                C.c_void_p(int(stream))))
        return out

    def follow(self, graph_or_pointer, first=0, count=None, stream=0):
        """lfx_keyframes_follow: the poses of keyframes [first, first + count) taken, device to device, from a PoseGraph (its
        view on `stream`) or from the device address of a [.][12] float64 array."""
        if isinstance(graph_or_pointer, PoseGraph):
            ptr, n = graph_or_pointer.view(stream)
            count = min(n, len(self)) - int(first) if count is None else int(count)
        else:
            ptr = int(graph_or_pointer)
            count = len(self) - int(first) if count is None else int(count)
        self._check(self._L.lfx_keyframes_follow(self._fx._ctx, self.handle, C.c_void_p(ptr), int(first), count, C.c_void_p(int(stream))))

    def build(self, kind, first=0, count=None, d_out=None, capacity_points=None, stream=0):
        """lfx_keyframes_build: the world cloud of keyframes [first, first + count) at the current poses.  Without d_out: a new
        torch tensor [n, 4] float32 on the device, written behind `stream`.  With d_out (a device address of capacity_points
        records): the number of records."""
        import torch
        kind = self._kind(kind)
        count = len(self) - int(first) if count is None else int(count)
        n = C.c_uint64(0)
        if d_out is not None:
            self._check(self._L.lfx_keyframes_build(self._fx._ctx, self.handle, kind, int(first), count, C.c_void_p(int(d_out) or None),
                                                    int(capacity_points), C.byref(n), C.c_void_p(int(stream))))
            return int(n.value)
        need = self._range_points(kind, first, count)
        out = torch.empty((need, 4), dtype=torch.float32, device=torch.device("cuda", self._fx.device))
        self._check(self._L.lfx_keyframes_build(self._fx._ctx, self.handle, kind, int(first), count, C.c_void_p(out.data_ptr() if need else None),
                                                need, C.byref(n), C.c_void_p(int(stream))))
        return out

    def submap(self, kind, center, radius, first=0, count=None, d_out=None, capacity_points=None, stream=0, _call="lfx_keyframes_submap"):
        """lfx_keyframes_submap: the keyframes of [first, first + count) within `radius` of `center`, written whole in
        ascending id until capacity_points.  Returns (cloud, result): result the dict of lfx_keyframes_submap_result; cloud a
        torch tensor [n_points, 4] (a view of a new tensor of capacity_points records, default the whole window's) or,
        with d_out, None."""
        import torch
        kind = self._kind(kind)
        count = len(self) - int(first) if count is None else int(count)
        c = np.ascontiguousarray(center, np.float64).reshape(3)
        out = None
        if d_out is None:
            capacity_points = self._range_points(kind, first, count) if capacity_points is None else int(capacity_points)
            out = torch.empty((capacity_points, 4), dtype=torch.float32, device=torch.device("cuda", self._fx.device))
            d_out = out.data_ptr() if capacity_points else 0
        r = B.KeyframesSubmapResult()
        self._check(getattr(self._L, _call)(self._fx._ctx, self.handle, kind, C.c_void_p(c.ctypes.data), float(radius), int(first), count,
                                            C.c_void_p(int(d_out) or None), int(capacity_points), C.byref(r), C.c_void_p(int(stream))))
        res = dict(n_selected=int(r.n_selected), n_written_keyframes=int(r.n_written_keyframes), n_points=int(r.n_points),
                   first_id=None if r.first_id == B.KEYFRAMES_NO_ID else int(r.first_id),
                   last_id=None if r.last_id == B.KEYFRAMES_NO_ID else int(r.last_id), truncated=bool(r.truncated))
        return (None if out is None else out[:res["n_points"]]), res

    def build_masked(self, kind, flags, first=0, count=None, begins=False, d_out=None, capacity_points=None, stream=0):
        """lfx_keyframes_build_masked: Keyframes.build without the records whose byte of `flags` (a uint8 device tensor or a
        device address, addressed by the store's record index of `kind`, as Visibility.run returns it) is non-zero.  Without
        d_out: a torch tensor [n_kept, 4] (a view of a new one of capacity_points records, default the range's).  With
        d_out: the number of kept records.  begins: also the [count + 1] int64 device tensor of the kept records before each
        keyframe -- (cloud, begins) or (n, begins)."""
        import torch
        kind = self._kind(kind)
        count = len(self) - int(first) if count is None else int(count)
        d_flags = flags.data_ptr() if hasattr(flags, "data_ptr") else int(flags)
        dev = torch.device("cuda", self._fx.device)
        d_begin = torch.empty(count + 1, dtype=torch.int64, device=dev) if begins else None
        out = None
        if d_out is None:
            capacity_points = self._range_points(kind, first, count) if capacity_points is None else int(capacity_points)
            out = torch.empty((capacity_points, 4), dtype=torch.float32, device=dev)
            d_out = out.data_ptr() if capacity_points else 0
        n = C.c_uint64(0)
        self._check(self._L.lfx_keyframes_build_masked(
            self._fx._ctx, self.handle, kind, int(first), count, C.c_void_p(d_flags or None), C.c_void_p(int(d_out) or None), int(capacity_points),
            C.c_void_p(d_begin.data_ptr() if begins else None), C.byref(n), C.c_void_p(int(stream))))
        got = int(n.value) if out is None else out[:int(n.value)]
        return (got, d_begin) if begins else got

    def _range_points(self, kind, first, count):
        """the records of keyframes [first, first + count) of `kind`, from the host's mirror: a build without room, which
        queues nothing and reports the records needed"""
        n = C.c_uint64(0)
        rc = self._L.lfx_keyframes_build(self._fx._ctx, self.handle, kind, int(first), int(count), None, 0, C.byref(n), None)
        if rc != B.ERR_CAPACITY:
            self._check(rc)
        return int(n.value)

    def save(self, dirname, stream=0):
        """lfx_keyframes_save: dirname/edge.pcd and dirname/surface.pcd at the current poses; (edge written, surface written)."""
        w = (C.c_int32 * 2)(0, 0)
        self._check(self._L.lfx_keyframes_save(self._fx._ctx, self.handle, os.fsencode(dirname), w, C.c_void_p(int(stream))))
        return bool(w[0]), bool(w[1])

    # --- flags kept in the store (include/lfx.h, the section behind lfx_keyframes_build_masked) ---
    def reserve_flags(self, stream=0):
        """lfx_keyframes_reserve_flags: one byte per record and kind, zeroed, that the masked calls below read.  Idempotent."""
        self._check(self._L.lfx_keyframes_reserve_flags(self._fx._ctx, self.handle, C.c_void_p(int(stream))))

    def flags(self, stream=0):
        """lfx_keyframes_flags: (edge, surface) uint8 device tensors OVER the store's memory, max_points[kind] long, addressed
        by the store's record index of the kind and current behind `stream` -- what Visibility.run(flags=...) and
        build_masked take.  They are views: they must not outlive the store."""
        p = (C.c_void_p * 2)()
        self._check(self._L.lfx_keyframes_flags(self._fx._ctx, self.handle, p, C.c_void_p(int(stream))))
        return tuple(_device_bytes(p[k], int(self.config.max_points[k]), self._fx.device, self) for k in range(2))

    def set_flags(self, kind, flags, first=0, count=None, stream=0):
        """lfx_keyframes_set_flags: the flag bytes of keyframes [first, first + count) copied from `flags` (a uint8 device
        tensor or a device address), which is addressed by the store's record index of `kind`."""
        count = len(self) - int(first) if count is None else int(count)
        d_src = flags.data_ptr() if hasattr(flags, "data_ptr") else int(flags)
        self._check(self._L.lfx_keyframes_set_flags(self._fx._ctx, self.handle, self._kind(kind), int(first), count, C.c_void_p(d_src or None),
                                                    C.c_void_p(int(stream))))

    def clear_flags(self, kind, first=0, count=None, stream=0):
        count = len(self) - int(first) if count is None else int(count)
        self._check(self._L.lfx_keyframes_clear_flags(self._fx._ctx, self.handle, self._kind(kind), int(first), count, C.c_void_p(int(stream))))

    def flags_info(self, stream=0):
        i = B.KeyframesFlagsInfo()
        self._check(self._L.lfx_keyframes_flags_info(self._fx._ctx, self.handle, C.byref(i), C.c_void_p(int(stream))))
        return dict(reserved=bool(i.reserved), device_bytes=int(i.device_bytes), n_flagged=(int(i.n_flagged[0]), int(i.n_flagged[1])))

    def submap_masked(self, kind, center, radius, first=0, count=None, d_out=None, capacity_points=None, stream=0):
        """lfx_keyframes_submap_masked: Keyframes.submap without the records the store's flags leave out; the same arguments
        and the same (cloud, result), n_points counting kept records."""
        return self.submap(kind, center, radius, first, count, d_out, capacity_points, stream, _call="lfx_keyframes_submap_masked")

    def save_masked(self, dirname, stream=0):
        """lfx_keyframes_save_masked: Keyframes.save without the flagged records; a kind without a kept record writes no file."""
        w = (C.c_int32 * 2)(0, 0)
        self._check(self._L.lfx_keyframes_save_masked(self._fx._ctx, self.handle, os.fsencode(dirname), w, C.c_void_p(int(stream))))
        return bool(w[0]), bool(w[1])

    def save_filtered(self, voxel_filter, dirname, leaf=(0.2, 0.4), min_points=1, masked=False, stream=0):
        """lfx_keyframes_save_filtered: Keyframes.save through a VoxelFilter -- per kind one centroid per voxel of leaf[kind]
        (edge, surface) with at least min_points records, in the order of first appearance; masked: without the records the
        store's flags leave out.  A kind without a surviving voxel writes no file."""
        w = (C.c_int32 * 2)(0, 0)
        lf = (C.c_float * 2)(float(leaf[0]), float(leaf[1]))
        self._check(self._L.lfx_keyframes_save_filtered(self._fx._ctx, self.handle, voxel_filter.handle, lf, int(min_points), int(bool(masked)),
                                                        os.fsencode(dirname), w, C.c_void_p(int(stream))))
        return bool(w[0]), bool(w[1])


class VoxelFilter(_Handle):
    """lfx_voxel_filter: clouds of any size thinned to one centroid per voxel of a grid anchored at the world origin
    (include/lfx.h, the voxel filter section): reset(leaf), add / add_keyframes as often as wanted, emit.  The output is a
    pure function of the sequence of records: the order of first appearance, centroids from integer sums."""

    _destroy = "lfx_voxel_filter_destroy"

    def __init__(self, fx, log2_slots, max_records):
        self._fx = fx
        self._L = fx._L
        cfg = B.VoxelFilterConfig()
        self._L.lfx_voxel_filter_default_config(C.byref(cfg))
        cfg.log2_slots = int(log2_slots)
        cfg.max_records = int(max_records)
        h = C.c_void_p()
        B.check(fx._ctx, self._L.lfx_voxel_filter_create(fx._ctx, C.byref(cfg), C.byref(h)), self._L)
        self.handle = h
        self.config = cfg

    def info(self):
        i = B.VoxelFilterInfo()
        self._check(self._L.lfx_voxel_filter_info(self.handle, C.byref(i)))
        return dict(slots=int(i.slots), max_records=int(i.max_records), n_records=int(i.n_records), leaf=float(i.leaf),
                    device_bytes=int(i.device_bytes))

    def reset(self, leaf, stream=0):
        """lfx_voxel_filter_reset: the table emptied, the leaf set, ranks from 0 again."""
        self._check(self._L.lfx_voxel_filter_reset(self._fx._ctx, self.handle, float(leaf), C.c_void_p(int(stream))))

    def add(self, points, n_points=None, stream=0):
        """lfx_voxel_filter_add / _add_host: records of 4 floats -- a float32 device tensor [n, 4], a device address with
        n_points, or a host array [n, 4] (which goes through the host call)."""
        if hasattr(points, "data_ptr"):
            n = points.shape[0] if n_points is None else int(n_points)
            self._check(self._L.lfx_voxel_filter_add(self._fx._ctx, self.handle, C.c_void_p(points.data_ptr() if n else None), n, C.c_void_p(int(stream))))
        elif isinstance(points, (int, np.integer)):
            self._check(self._L.lfx_voxel_filter_add(self._fx._ctx, self.handle, C.c_void_p(int(points) or None), int(n_points), C.c_void_p(int(stream))))
        else:
            p = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
            self._check(self._L.lfx_voxel_filter_add_host(self._fx._ctx, self.handle, C.c_void_p(p.ctypes.data if len(p) else None), len(p),
                                                          C.c_void_p(int(stream))))

    def add_keyframes(self, keyframes, kind, first=0, count=None, masked=False, stream=0):
        """lfx_voxel_filter_add_keyframes: keyframes [first, first + count) of a Keyframes store at its current poses, straight
        from the store's sensor-frame records; masked: without the records the store's flags leave out."""
        count = len(keyframes) - int(first) if count is None else int(count)
        self._check(self._L.lfx_voxel_filter_add_keyframes(self._fx._ctx, self.handle, keyframes.handle, Keyframes._kind(kind), int(first), count,
                                                           int(bool(masked)), C.c_void_p(int(stream))))

    @staticmethod
    def result(r):
        return {n: int(getattr(r, n)) for n, _ in B.VoxelFilterResult._fields_}

    def emit_raw(self, min_points, d_out, capacity_points, d_counts_out=0, stream=0):
        """lfx_voxel_filter_emit into device addresses: (return code, result dict) -- LFX_ERR_CAPACITY comes back with the
        result filled, so nothing is raised here."""
        r = B.VoxelFilterResult()
        rc = self._L.lfx_voxel_filter_emit(self._fx._ctx, self.handle, int(min_points), C.c_void_p(int(d_out) or None), int(capacity_points),
                                           C.c_void_p(int(d_counts_out) or None), C.byref(r), C.c_void_p(int(stream)))
        return rc, self.result(r)

    def emit(self, min_points=1, capacity_points=None, counts=False, stream=0):
        """lfx_voxel_filter_emit: (cloud, result) or (cloud, counts, result) -- cloud a torch tensor [n_written, 4] float32 (a
        view of a new one of capacity_points records, default the records added), counts its uint32 counts as int32 bits."""
        import torch
        dev = torch.device("cuda", self._fx.device)
        cap = self.info()["n_records"] if capacity_points is None else int(capacity_points)
        out = torch.empty((cap, 4), dtype=torch.float32, device=dev)
        cnt = torch.empty(cap, dtype=torch.int32, device=dev) if counts else None
        rc, res = self.emit_raw(min_points, out.data_ptr() if cap else 0, cap, cnt.data_ptr() if counts and cap else 0, stream)
        self._check(rc)
        n = res["n_written"]
        return (out[:n], cnt[:n], res) if counts else (out[:n], res)


def _device_bytes(ptr, n, device, owner):
    """a uint8 torch tensor over n bytes of device memory at `ptr` that the library owns; `owner` is kept alive with it"""
    import torch

    class _Span:
        pass
    span = _Span()
    span.owner = owner
    span.__cuda_array_interface__ = dict(shape=(int(n),), typestr="|u1", data=(int(ptr), False), version=2)
    return torch.as_tensor(span, device=torch.device("cuda", device))


class OccupancyGrid(_Handle):
    """lfx_occupancy: a 2-D occupancy grid rendered from scans by ray casting (include/lfx.h, the occupancy section).
    add_batch reduces the last device batch's scans to W beams each and keeps them with one pose per scan; render casts the
    kept beams through the grid at the poses of the moment (set_poses / follow move them); emit gives
    nav_msgs/OccupancyGrid.data.  Poses are [3][4] = [R | t] float64; scan ids count from 0 in order of addition."""

    _destroy = "lfx_occupancy_destroy"

    def __init__(self, fx, width, height, resolution, origin=(0.0, 0.0), max_scans=1024, config=None, **fields):
        self._fx = fx
        self._L = fx._L
        cfg = occupancy_config(config, **dict(dict(width=int(width), height=int(height), resolution=float(resolution), origin_x=float(origin[0]),
                                                   origin_y=float(origin[1]), max_scans=int(max_scans)), **fields))
        h = C.c_void_p()
        B.check(fx._ctx, self._L.lfx_occupancy_create(fx._ctx, C.byref(cfg), C.byref(h)), self._L)
        self.handle = h
        self.config = cfg

    def info(self):
        i = B.OccupancyInfo()
        self._check(self._L.lfx_occupancy_info(self.handle, C.byref(i)))
        return {n: int(getattr(i, n)) for n, _ in B.OccupancyInfo._fields_ if n != "reserved"}

    def __len__(self):
        return self.info()["n_scans"]

    def view(self, stream=0):
        """lfx_occupancy_view: the device addresses of the beams, the poses and the two count arrays, current behind
        `stream`, and the number of scans."""
        v = B.OccupancyView()
        self._check(self._L.lfx_occupancy_view(self._fx._ctx, self.handle, C.byref(v), C.c_void_p(int(stream))))
        return dict(beams=v.beams or 0, poses=v.poses or 0, hits=v.hits or 0, misses=v.misses or 0, n_scans=int(v.n_scans))

    def add_batch(self, poses, select=None, classes=None, obstacle_mask=15, clear_mask=15, stream=0):
        """lfx_occupancy_add_batch: the scans of the last device batch (whose records must still be alive), one pose per
        scan of the batch; select: None or one flag per scan (0: left out); classes: segment()'s uint8 device tensor for this
        batch, or None, with the two masks over B.SEG_*.  The id of the first scan added.  Asynchronous: the records are read
        behind `stream`, which the caller waits for before the context is handed its next scans."""
        pm = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        sel = None if select is None else np.ascontiguousarray(np.asarray(select) != 0, np.uint8)
        if sel is not None and len(sel) != len(pm):
            raise ValueError("select must hold one flag per pose")
        if classes is not None and (classes.numel() < self._fx.batch_points() or classes.element_size() != 1):
            raise B.LfxError(B.ERR_INVALID_ARGUMENT, "classes must hold one byte for each of the last batch's records")
        first = C.c_uint32(0)
        self._check(self._L.lfx_occupancy_add_batch(
            self._fx._ctx, self.handle, len(pm), C.c_void_p(pm.ctypes.data if len(pm) else None), C.c_void_p(sel.ctypes.data if sel is not None and len(sel) else None),
            C.c_void_p((classes.data_ptr() or None) if classes is not None else None), int(obstacle_mask), int(clear_mask), C.byref(first),
            C.c_void_p(int(stream))))
        return int(first.value)

    def set_poses(self, poses, first=0, stream=0):
        p = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        self._check(self._L.lfx_occupancy_set_poses(self._fx._ctx, self.handle, int(first), len(p), C.c_void_p(p.ctypes.data if len(p) else None),
                                                    C.c_void_p(int(stream))))

    def poses(self, first=0, count=None, stream=0):
        """lfx_occupancy_poses: scans first .. first + count - 1 as [count][3][4] float64 on the host."""
        count = len(self) - int(first) if count is None else int(count)
        out = np.zeros((max(count, 0), 3, 4))
        self._check(self._L.lfx_occupancy_poses(self._fx._ctx, self.handle, int(first), count, C.c_void_p(out.ctypes.data if out.size else None),
                                                C.c_void_p(int(stream))))
        return out

    def follow(self, graph_or_pointer, first=0, count=None, stream=0):
        """lfx_occupancy_follow: the poses of scans [first, first + count) taken, device to device, from a PoseGraph (its view
        on `stream`) or from the device address of a [.][12] float64 array."""
        if isinstance(graph_or_pointer, PoseGraph):
            ptr, n = graph_or_pointer.view(stream)
            count = min(n, len(self)) - int(first) if count is None else int(count)
        else:
            ptr = int(graph_or_pointer)
            count = len(self) - int(first) if count is None else int(count)
        self._check(self._L.lfx_occupancy_follow(self._fx._ctx, self.handle, C.c_void_p(ptr), int(first), count, C.c_void_p(int(stream))))

    def truncate(self, n_scans=0, stream=0):
        """lfx_occupancy_truncate: the kept scans from n_scans on are dropped (the counts stay) -- a grid of 1 x 1 cells as the
        reducer of live scans starts every batch with truncate(0)."""
        self._check(self._L.lfx_occupancy_truncate(self._fx._ctx, self.handle, int(n_scans), C.c_void_p(int(stream))))

    def clear(self, stream=0):
        self._check(self._L.lfx_occupancy_clear(self._fx._ctx, self.handle, C.c_void_p(int(stream))))

    def render(self, first=0, count=None, stream=0):
        """lfx_occupancy_render: the votes of scans [first, first + count) at their current poses added to the counts."""
        count = len(self) - int(first) if count is None else int(count)
        self._check(self._L.lfx_occupancy_render(self._fx._ctx, self.handle, int(first), count, C.c_void_p(int(stream))))

    def counters(self, stream=0):
        r = B.OccupancyCounters()
        self._check(self._L.lfx_occupancy_counters(self._fx._ctx, self.handle, C.byref(r), C.c_void_p(int(stream))))
        return {n: int(getattr(r, n)) for n, _ in B.OccupancyCounters._fields_}

    def emit(self, config=None, out=None, stream=0, **fields):
        """lfx_occupancy_emit: the grid as int8 [height][width], row 0 the lowest y.  out: None = a new int8 device tensor is
        returned, or the address of device memory or of a pinned block (nothing is returned).  Asynchronous on `stream`."""
        cfg = occupancy_emit_config(config, **fields)
        made = None
        if out is None:
            import torch
            made = torch.empty((int(self.config.height), int(self.config.width)), dtype=torch.int8, device=torch.device("cuda", self._fx.device))
            out = made.data_ptr()
        self._check(self._L.lfx_occupancy_emit(self._fx._ctx, self.handle, C.byref(cfg), C.c_void_p(int(out) or None), C.c_void_p(int(stream))))
        return made

    def save(self, dirname, config=None, occupied_percent=65, free_percent=25, stream=0, **fields):
        """lfx_occupancy_save: dirname/map.pgm and dirname/map.yaml of the grid as it stands.  Synchronous."""
        cfg = occupancy_emit_config(config, **fields)
        self._check(self._L.lfx_occupancy_save(self._fx._ctx, self.handle, C.byref(cfg), os.fsencode(str(dirname)), int(occupied_percent),
                                               int(free_percent), C.c_void_p(int(stream))))

    def _array(self, ptr, shape, dtype, stream):
        import torch
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        if n == 0:
            return np.zeros(shape, dtype)
        torch.cuda.synchronize(self._fx.device)              # (a read-back for inspection: everything queued has landed)
        return _device_bytes(ptr, n, self._fx.device, self).cpu().numpy().view(dtype).reshape(shape).copy()

    def beams(self, stream=0):
        """The kept beams on the host: (xyz [n_scans][W][3] float32, kind [n_scans][W] uint32)."""
        v = self.view(stream)
        raw = self._array(v["beams"], (v["n_scans"], int(self.config.n_beams), 4), np.float32, stream)
        return np.ascontiguousarray(raw[..., :3]), np.ascontiguousarray(raw[..., 3]).view(np.uint32)

    def counts(self, stream=0):
        """(hits, misses) on the host, uint32 [height][width] each."""
        v = self.view(stream)
        shape = (int(self.config.height), int(self.config.width))
        return self._array(v["hits"], shape, np.uint32, stream), self._array(v["misses"], shape, np.uint32, stream)


class DistanceField(_Handle):
    """lfx_distance: the exact squared distance of every cell of an occupancy grid to the nearest obstacle cell, and what
    planners take from it -- metres (an ESDF) and nav2's inflated costmap (include/lfx.h, the distance section).  A transform
    (from_grid, from_occupancy) rebuilds the whole field; metres, costmap and stats read the last one."""

    _destroy = "lfx_distance_destroy"

    def __init__(self, fx, width, height):
        self._fx = fx
        self._L = fx._L
        h = C.c_void_p()
        B.check(fx._ctx, self._L.lfx_distance_create(fx._ctx, int(width), int(height), C.byref(h)), self._L)
        self.handle = h
        self.width, self.height = int(width), int(height)

    def info(self):
        i = B.DistanceInfo()
        self._check(self._L.lfx_distance_info(self.handle, C.byref(i)))
        return {n: int(getattr(i, n)) for n, _ in B.DistanceInfo._fields_ if n != "reserved"}

    def from_grid(self, grid, config=None, stream=0, **fields):
        """lfx_distance_from_grid: the transform of an int8 grid [height][width] in emit's format -- a device tensor or the
        address of device memory.  Asynchronous: the grid is read behind `stream`."""
        cfg = distance_config(config, **fields)
        if hasattr(grid, "data_ptr"):
            if grid.element_size() != 1 or grid.numel() != self.width * self.height or not grid.is_contiguous():
                raise ValueError("the grid is a contiguous int8 tensor of height x width cells")
            grid = grid.data_ptr()
        self._check(self._L.lfx_distance_from_grid(self._fx._ctx, self.handle, C.c_void_p(int(grid) or None), C.byref(cfg), C.c_void_p(int(stream))))

    def from_occupancy(self, occupancy, emit_config=None, config=None, stream=0, **fields):
        """lfx_distance_from_occupancy: the transform of an OccupancyGrid's counts as they stand -- the bytes of its emit with
        emit_config and from_grid of them, without the int8 grid in between."""
        ecfg = occupancy_emit_config(emit_config)
        cfg = distance_config(config, **fields)
        self._check(self._L.lfx_distance_from_occupancy(self._fx._ctx, self.handle, occupancy.handle, C.byref(ecfg), C.byref(cfg),
                                                        C.c_void_p(int(stream))))

    def view(self, stream=0):
        """lfx_distance_view: the device addresses of the classes, d2 and i2 (0 without `inside`), current behind `stream`."""
        v = B.DistanceView()
        self._check(self._L.lfx_distance_view(self._fx._ctx, self.handle, C.byref(v), C.c_void_p(int(stream))))
        return dict(classes=v.classes or 0, d2=v.d2 or 0, i2=v.i2 or 0)

    def _new(self, dtype):
        import torch
        return torch.empty((self.height, self.width), dtype=dtype, device=torch.device("cuda", self._fx.device))

    def metres(self, resolution, out=None, stream=0):
        """lfx_distance_metres: float32 [height][width].  out: None = a new device tensor is returned, or the address of
        device memory or of a pinned block (nothing is returned).  Asynchronous on `stream`."""
        made = None
        if out is None:
            import torch
            made = self._new(torch.float32)
            out = made.data_ptr()
        self._check(self._L.lfx_distance_metres(self._fx._ctx, self.handle, float(resolution), C.c_void_p(int(out) or None), C.c_void_p(int(stream))))
        return made

    def costmap(self, resolution, config=None, out=None, stream=0, **fields):
        """lfx_distance_costmap: nav2's costs, uint8 [height][width]; out as for metres."""
        cfg = distance_cost_config(config, **fields)
        made = None
        if out is None:
            import torch
            made = self._new(torch.uint8)
            out = made.data_ptr()
        self._check(self._L.lfx_distance_costmap(self._fx._ctx, self.handle, C.byref(cfg), float(resolution), C.c_void_p(int(out) or None),
                                                 C.c_void_p(int(stream))))
        return made

    def stats(self, stream=0):
        r = B.DistanceStats()
        self._check(self._L.lfx_distance_stats(self._fx._ctx, self.handle, C.byref(r), C.c_void_p(int(stream))))
        return {n: int(getattr(r, n)) for n, _ in B.DistanceStats._fields_}

    def fields(self, stream=0):
        """The last transform on the host: (classes uint8, d2 uint32, i2 uint32 or None), [height][width] each."""
        import torch
        v = self.view(stream)
        torch.cuda.synchronize(self._fx.device)              # (a read-back for inspection: everything queued has landed)
        shape = (self.height, self.width)

        def get(ptr, dtype):
            n = self.width * self.height * np.dtype(dtype).itemsize
            return _device_bytes(ptr, n, self._fx.device, self).cpu().numpy().view(dtype).reshape(shape).copy()
        return get(v["classes"], np.uint8), get(v["d2"], np.uint32), (get(v["i2"], np.uint32) if v["i2"] else None)


class GridMatcher(_Handle):
    """lfx_grid_match: where a scan is in an occupancy grid (include/lfx.h, the grid-match section).  set_field turns a
    DistanceField's last transform into a score field through a table, set_scans keeps scans as levelled 2-D points; score
    rates arbitrary candidate poses, search a window of whole-cell shifts and headings around a centre.  Outputs are uint32
    device tensors."""

    _destroy = "lfx_grid_match_destroy"

    def __init__(self, fx, width, height, resolution, origin=(0.0, 0.0), config=None, **fields):
        self._fx = fx
        self._L = fx._L
        cfg = grid_match_config(config, **dict(dict(width=int(width), height=int(height), resolution=float(resolution), origin_x=float(origin[0]),
                                                    origin_y=float(origin[1])), **fields))
        h = C.c_void_p()
        B.check(fx._ctx, self._L.lfx_grid_match_create(fx._ctx, C.byref(cfg), C.byref(h)), self._L)
        self.handle = h
        self.config = cfg

    def info(self):
        i = B.GridMatchInfo()
        self._check(self._L.lfx_grid_match_info(self.handle, C.byref(i)))
        return {n: int(getattr(i, n)) for n, _ in B.GridMatchInfo._fields_ if n != "reserved"}

    def view(self, stream=0):
        """lfx_grid_match_view: the device addresses of the field, the points and their counts, current behind `stream`."""
        v = B.GridMatchView()
        self._check(self._L.lfx_grid_match_view(self._fx._ctx, self.handle, C.byref(v), C.c_void_p(int(stream))))
        return dict(field=v.field or 0, points=v.points or 0, n_points=v.n_points or 0)

    def set_field(self, field, table=None, stream=0, **fields):
        """lfx_grid_match_set_field: the score field of a DistanceField's last transform.  table: None or a dict (the fields of
        lfx_grid_match_table_config, the table made at the matcher's resolution), or a uint16 array handed as it is."""
        if table is None or isinstance(table, (dict, B.GridMatchTableConfig)):
            lut = grid_match_table(grid_match_table_config(table, **fields), float(self.config.resolution))
        else:
            lut = np.ascontiguousarray(table, np.uint16).reshape(-1)
        self._check(self._L.lfx_grid_match_set_field(self._fx._ctx, self.handle, field.handle, C.c_void_p(lut.ctypes.data if len(lut) else None), len(lut),
                                                     C.c_void_p(int(stream))))

    def set_scans(self, beams, n_scans=None, n_beams=None, levels=None, stream=0):
        """lfx_grid_match_set_scans: scans 0 .. n - 1 from beams -- a float32 device tensor [n][W][4] as OccupancyGrid.view()'s, or
        the address of one with n_scans and n_beams; levels: None or [n][3][3] float64."""
        if hasattr(beams, "data_ptr"):
            if beams.dim() != 3 or beams.shape[2] != 4 or beams.element_size() != 4 or not beams.is_contiguous():
                raise ValueError("the beams are a contiguous float32 tensor [n][W][4]")
            n_scans, n_beams = int(beams.shape[0]), int(beams.shape[1])
            beams = beams.data_ptr()
        lv = None if levels is None else np.ascontiguousarray(levels, np.float64).reshape(-1, 9)
        if lv is not None and len(lv) != int(n_scans):
            raise ValueError("levels must hold one matrix per scan")
        self._check(self._L.lfx_grid_match_set_scans(self._fx._ctx, self.handle, C.c_void_p(int(beams) or None), int(n_scans), int(n_beams),
                                                     C.c_void_p(lv.ctypes.data if lv is not None and len(lv) else None), C.c_void_p(int(stream))))

    def set_scans_occupancy(self, occupancy, first=0, count=None, use_rotation=True, stream=0):
        """lfx_grid_match_set_scans_occupancy: an OccupancyGrid's scans [first, first + count), levelled by the rotations of the
        poses it holds now (use_rotation) or not at all."""
        count = len(occupancy) - int(first) if count is None else int(count)
        self._check(self._L.lfx_grid_match_set_scans_occupancy(self._fx._ctx, self.handle, occupancy.handle, int(first), count, int(bool(use_rotation)),
                                                               C.c_void_p(int(stream))))

    def _new(self, shape):
        import torch
        return torch.empty(shape, dtype=torch.int32, device=torch.device("cuda", self._fx.device))

    def score(self, scan, candidates, inside=True, stream=0):
        """lfx_grid_match_score: candidates float64 [P][4] = (tx, ty, cos, sin), a device tensor or a host array (uploaded on the
        current stream); (score, inside) int32 device tensors [P] holding uint32 bits (inside None if not asked for)."""
        import torch
        if not hasattr(candidates, "data_ptr"):
            candidates = torch.from_numpy(np.ascontiguousarray(candidates, np.float64).reshape(-1, 4)).to(torch.device("cuda", self._fx.device))
        if candidates.dim() != 2 or candidates.shape[1] != 4 or candidates.element_size() != 8 or not candidates.is_contiguous():
            raise ValueError("the candidates are a contiguous float64 tensor [P][4]")
        P = int(candidates.shape[0])
        sc, ins = self._new((P,)), (self._new((P,)) if inside else None)
        self._check(self._L.lfx_grid_match_score(self._fx._ctx, self.handle, int(scan), C.c_void_p(candidates.data_ptr() or None), P,
                                                 C.c_void_p(sc.data_ptr() or None), C.c_void_p(ins.data_ptr() if ins is not None else None),
                                                 C.c_void_p(int(stream))))
        return sc, ins

    def search(self, centres, search=None, first=0, slice_best=False, volume=False, stream=0, **fields):
        """lfx_grid_match_search: centres [n][3] = (x0, y0, yaw0), one per scan of [first, first + n); (best [n][4] = score,
        index, inside, n_points; slice_best [n][T][2] or None; volume [n][T][Ny][Nx] or None), int32 device tensors holding
        uint32 bits."""
        cfg = grid_match_search_config(search, **fields)
        cs = np.ascontiguousarray(centres, np.float64).reshape(-1, 3)
        n = len(cs)
        Nx, Ny, T = 2 * int(cfg.half_x) + 1, 2 * int(cfg.half_y) + 1, 2 * int(cfg.half_theta) + 1
        big = max(int(cfg.half_x), int(cfg.half_y)) > B.GRID_MATCH_MAX_HALF or int(cfg.half_theta) > B.GRID_MATCH_MAX_HALF_THETA
        best = self._new((n, 4))
        sl = self._new((n, T, 2)) if slice_best and not big else None
        vol = self._new((n, T, Ny, Nx)) if volume and not big else None
        self._check(self._L.lfx_grid_match_search(self._fx._ctx, self.handle, int(first), n, C.c_void_p(cs.ctypes.data if n else None), C.byref(cfg),
                                                  C.c_void_p(best.data_ptr() or None), C.c_void_p(sl.data_ptr() if sl is not None else None),
                                                  C.c_void_p(vol.data_ptr() if vol is not None else None), C.c_void_p(int(stream))))
        return best, sl, vol

    def field(self, stream=0):
        """The score field on the host, uint16 [height][width]."""
        import torch
        v = self.view(stream)
        torch.cuda.synchronize(self._fx.device)              # (a read-back for inspection: everything queued has landed)
        h, w = int(self.config.height), int(self.config.width)
        return _device_bytes(v["field"], 2 * h * w, self._fx.device, self).cpu().numpy().view(np.uint16).reshape(h, w).copy()

    def points(self, stream=0):
        """The kept points on the host: a list of float64 [n_points[s]][2], one per scan set."""
        import torch
        v = self.view(stream)
        torch.cuda.synchronize(self._fx.device)
        n, B_ = self.info()["n_scans"], int(self.config.max_beams)
        if n == 0:
            return []
        counts = _device_bytes(v["n_points"], 4 * n, self._fx.device, self).cpu().numpy().view(np.uint32)
        pts = _device_bytes(v["points"], 16 * n * B_, self._fx.device, self).cpu().numpy().view(np.float64).reshape(n, B_, 2)
        return [pts[s, :int(counts[s])].copy() for s in range(n)]


class Visibility(_Handle):
    """lfx_visibility: the visibility votes of a window of a Keyframes store's keyframes on each other's records, and the
    DYNAMIC flag they decide (include/lfx.h, the visibility section).  The fields of lfx_visibility_config as keywords."""

    _destroy = "lfx_visibility_destroy"

    def __init__(self, fx, max_window=1024, max_resident_images=None, config=None, **fields):
        self._fx = fx
        self._L = fx._L
        cfg = visibility_config(config, **fields)
        resident = int(max_window) if max_resident_images is None else int(max_resident_images)
        h = C.c_void_p()
        B.check(fx._ctx, self._L.lfx_visibility_create(fx._ctx, C.byref(cfg), int(max_window), resident, C.byref(h)), self._L)
        self.handle = h
        self.config = cfg

    def info(self):
        i = B.VisibilityInfo()
        self._check(self._L.lfx_visibility_info(self.handle, C.byref(i)))
        return dict(config={k: getattr(i.config, k) for k, _ in B.VisibilityConfig._fields_}, max_window=int(i.max_window),
                    max_resident_images=int(i.max_resident_images), device_bytes=int(i.device_bytes))

    @staticmethod
    def result(r):
        return dict(n_pairs=int(r.n_pairs), n_viewer_chunks=int(r.n_viewer_chunks), n_records=(int(r.n_records[0]), int(r.n_records[1])),
                    n_voted=(int(r.n_voted[0]), int(r.n_voted[1])), n_dynamic=(int(r.n_dynamic[0]), int(r.n_dynamic[1])),
                    occupied_cells=int(r.occupied_cells), total_cells=int(r.total_cells))

    def run(self, keyframes, first=0, count=None, votes=False, flags=None, stream=0):
        """lfx_visibility_run over keyframes [first, first + count) of `keyframes`.  Returns (flags, votes, result): flags
        (edge, surface) uint8 device tensors and votes (edge, surface) int32 device tensors (the library's uint32: through |
        agree << 16) or None, each addressed by the store's record index of its kind and as long as the store's records --
        only the window's elements are written, the others keep what they held (new tensors: 0); result the dict of
        lfx_visibility_result.  flags / votes may be given as pairs of tensors to write into; votes False: not wanted."""
        import torch
        count = len(keyframes) - int(first) if count is None else int(count)
        n = keyframes.info()["n_points"]
        dev = torch.device("cuda", self._fx.device)
        if flags is None:
            flags = tuple(torch.zeros(max(n[k], 1), dtype=torch.uint8, device=dev) for k in range(2))
        if votes is True:
            votes = tuple(torch.zeros(max(n[k], 1), dtype=torch.int32, device=dev) for k in range(2))
        elif votes is False or votes is None:
            votes = None
        for k in range(2):
            if flags[k].dtype != torch.uint8 or flags[k].numel() < n[k] or (votes is not None and (votes[k].dtype != torch.int32 or votes[k].numel() < n[k])):
                raise ValueError("flags are uint8 and votes int32 tensors of at least the store's records of their kind")
        pf = (C.c_void_p * 2)(flags[0].data_ptr(), flags[1].data_ptr())
        pv = (C.c_void_p * 2)(votes[0].data_ptr() if votes else None, votes[1].data_ptr() if votes else None)
        r = B.VisibilityResult()
        self._check(self._L.lfx_visibility_run(self._fx._ctx, self.handle, keyframes.handle, int(first), count, pv, pf, C.byref(r),
                                               C.c_void_p(int(stream))))
        return flags, votes, self.result(r)


def loop_closer_config(config=None, **fields):
    """lfx_loop_closer_config: the defaults (lfx_loop_closer_default_config) with the given fields replaced.  config: None, a
    dict of fields, or a B.LoopCloserConfig (copied).  submap_capacity: one number or (edge, surface)."""
    if not isinstance(config, B.LoopCloserConfig):
        config, fields = None, dict(config or {}, **fields)
    capacity = fields.pop("submap_capacity", None)
    cfg = _config(B.LoopCloserConfig, "lfx_loop_closer_default_config", "loop-closer", config, fields)
    if capacity is not None:
        v = (capacity, capacity) if np.isscalar(capacity) else tuple(capacity)
        cfg.submap_capacity[0], cfg.submap_capacity[1] = int(v[0]), int(v[1])
    return cfg


class LoopCloser(_Handle):
    """lfx_loop_closer: revisits found in a PlaceDb, verified against submaps of a Keyframes store and closed in a PoseGraph
    (include/lfx.h, the loop closer section).  Keyframe id == place entry == graph node id.  The three outlive the closer."""

    _destroy = "lfx_loop_closer_destroy"

    REASONS = ("accepted", "no_candidate", "empty_query", "empty_submap", "align_failed", "no_report", "rank", "degenerate", "rms_edge",
               "rms_surface", "inliers", "sigma2")

    def __init__(self, fx, keyframes, place_db, graph, config=None, **fields):
        self._fx = fx
        self._L = fx._L
        self.config = loop_closer_config(config, **fields)
        self.keyframes, self.place_db, self.graph = keyframes, place_db, graph
        h = C.c_void_p()
        B.check(fx._ctx, self._L.lfx_loop_closer_create(fx._ctx, C.byref(self.config), keyframes.handle, place_db.handle, graph.handle, C.byref(h)),
                self._L)
        self.handle = h

    def info(self):
        i = B.LoopCloserInfo()
        self._check(self._L.lfx_loop_closer_info(self.handle, C.byref(i)))
        return dict(device_bytes=int(i.device_bytes))

    def set_masked(self, masked=True):
        """lfx_loop_closer_set_masked: verify against submaps without the store's flagged records (the store has reserved
        flags: Keyframes.reserve_flags).  The query keyframe's own clouds are used as stored."""
        rc = self._L.lfx_loop_closer_set_masked(self.handle, int(bool(masked)))
        if rc != 0:
            raise B.LfxError(rc, "set_masked: the closer's store has no flags reserved")

    @property
    def masked(self):
        m = C.c_int32(0)
        self._check(self._L.lfx_loop_closer_get_masked(self.handle, C.byref(m)))
        return bool(m.value)

    def detect_raw(self, first, count, stream=0):
        """lfx_loop_closer_detect as it returns: (a B.PlaceMatch array [count * n_candidates], n_eligible uint32 [count])."""
        k = int(self.config.n_candidates)
        res = (B.PlaceMatch * max(int(count) * k, 1))()
        n_eligible = np.zeros(max(int(count), 1), np.uint32)
        self._check(self._L.lfx_loop_closer_detect(self._fx._ctx, self.handle, int(first), int(count), res,
                                                   n_eligible.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_void_p(int(stream))))
        return res, n_eligible[:max(int(count), 0)]

    def detect(self, first, count, stream=0):
        """The candidates of keyframes first .. first + count - 1: (a list per keyframe of n_candidates match dicts, best first,
        entry None where none is left; n_eligible per keyframe)."""
        res, n_eligible = self.detect_raw(first, count, stream)
        k = int(self.config.n_candidates)
        return [[_match(m) for m in res[q * k:(q + 1) * k]] for q in range(int(count))], [int(n) for n in n_eligible]

    @staticmethod
    def _candidate(candidate):
        if isinstance(candidate, B.PlaceMatch):
            return candidate
        entry = B.PLACE_NO_ENTRY if candidate["entry"] is None else int(candidate["entry"])
        return B.PlaceMatch(entry, int(candidate.get("shift", 0)), float(candidate.get("distance", 0.0)), float(candidate["yaw"]))

    def verify_raw(self, query_id, candidate, stream=0):
        """lfx_loop_closer_verify as it returns: a B.LoopClosure.  candidate: a B.PlaceMatch or a match dict."""
        out = B.LoopClosure()
        m = self._candidate(candidate)
        self._check(self._L.lfx_loop_closer_verify(self._fx._ctx, self.handle, int(query_id), C.byref(m), C.byref(out), C.c_void_p(int(stream))))
        return out

    def closure(self, c):
        """A B.LoopClosure as a dict: query, candidate, accepted, reason (a name of REASONS), match, result, report, submap (a
        pair of dicts), edge (a B.POSE_GRAPH_EDGE_DTYPE record), raw (the record's bytes)."""
        edge = np.frombuffer(bytes(c.edge), B.POSE_GRAPH_EDGE_DTYPE)[0]
        sub = [dict(n_selected=int(r.n_selected), n_written_keyframes=int(r.n_written_keyframes), n_points=int(r.n_points),
                    first_id=None if r.first_id == B.KEYFRAMES_NO_ID else int(r.first_id),
                    last_id=None if r.last_id == B.KEYFRAMES_NO_ID else int(r.last_id), truncated=bool(r.truncated)) for r in c.submap]
        return dict(query=int(c.query), candidate=None if c.candidate == B.PLACE_NO_ENTRY else int(c.candidate), accepted=bool(c.accepted),
                    reason=self.REASONS[c.reason], match=_match(c.match), result=self._fx._align_results([c.result])[0],
                    report=self._fx._align_reports([c.report])[0], submap=sub, edge=edge, raw=bytes(c))

    def verify(self, query_id, candidate, stream=0):
        return self.closure(self.verify_raw(query_id, candidate, stream))

    def update_raw(self, first, count, stream=0):
        """lfx_loop_closer_update as it returns: (rc, a B.LoopClosure array [count], a B.LoopCloserResult) -- rc so that a
        caller can look at the closures of a call that ended with B.ERR_CAPACITY."""
        closures = (B.LoopClosure * max(int(count), 1))()
        result = B.LoopCloserResult()
        rc = self._L.lfx_loop_closer_update(self._fx._ctx, self.handle, int(first), int(count), closures, C.byref(result), C.c_void_p(int(stream)))
        return rc, closures, result

    def update(self, first, count, stream=0):
        """Detect, verify, add the accepted edges, optimise, make the store follow: (a closure dict per keyframe, a dict of
        n_detected, n_verified, n_accepted, followed and graph -- PoseGraph.optimize's dict, None where it did not run)."""
        rc, closures, r = self.update_raw(first, count, stream)
        self._check(rc)
        g = r.graph
        graph = dict(code=int(g.code), iterations=int(g.iterations), chi2_initial=float(g.chi2_initial), chi2_final=float(g.chi2_final),
                     max_step=float(g.max_step), n_chain=int(g.n_chain), n_loop=int(g.n_loop),
                     n_robust_downweighted=int(g.n_robust_downweighted)) if r.n_accepted else None
        return ([self.closure(c) for c in closures[:int(count)]],
                dict(n_detected=int(r.n_detected), n_verified=int(r.n_verified), n_accepted=int(r.n_accepted), followed=bool(r.followed), graph=graph))
