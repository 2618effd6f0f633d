"""ctypes binding of the C ABI in include/lfx.h (liblfx.so: HIP kernels + host side).

There is no fallback: if the library has not been built, or no MI355X is present when a
context is created, this raises.  Build with `python __graft_entry__.py` (or
`make -C lidar_feature_extraction_amd/csrc`).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LFX_LIB_PATH") or os.path.join(_HERE, "_lib", "liblfx.so")   # override: A/B builds only

LFX_N_KERNELS = 24
MAX_RING_POINTS = 4608            # LFX_MAX_RING_POINTS: the longest ring the LDS-resident kernels take; the default ring capacity
MAX_LONG_RING_POINTS = 262144     # LFX_MAX_LONG_RING_POINTS: the largest max_points_per_ring (longer rings: HBM workspace)
MAX_RINGS = 256

STAGE_LABEL, STAGE_OCCLUSION, STAGE_OUT_OF_RANGE, STAGE_PARALLEL_BEAM = 1, 2, 4, 8
STAGE_SINGLE_BLOCK, STAGE_CURVATURE, STAGE_ALL = 16, 32, 47


class LfxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("lfx error %d: %s" % (code, msg))
        self.code = code


class Params(C.Structure):
    """lfx_params == HyperParameters, extraction/include/lidar_feature_extraction/hyper_parameter.hpp:32-65"""
    _fields_ = [("padding", C.c_int32), ("neighbor_degree_threshold", C.c_double),
                ("distance_diff_threshold", C.c_double), ("parallel_beam_min_range_ratio", C.c_double),
                ("edge_threshold", C.c_double), ("surface_threshold", C.c_double),
                ("min_range", C.c_double), ("max_range", C.c_double), ("n_blocks", C.c_int32)]


class Layout(C.Structure):
    _fields_ = [("point_step", C.c_uint32), ("off_x", C.c_uint32), ("off_y", C.c_uint32),
                ("off_z", C.c_uint32), ("off_ring", C.c_uint32), ("ring_datatype", C.c_uint32),
                ("big_endian", C.c_uint32)]


class PointField(C.Structure):
    _fields_ = [("name", C.c_char_p), ("offset", C.c_uint32), ("datatype", C.c_uint8), ("count", C.c_uint32)]


# sensor_msgs/msg/PointField datatype codes
INT8, UINT8, INT16, UINT16, INT32, UINT32, FLOAT32, FLOAT64 = range(1, 9)


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_points_per_scan", C.c_uint32), ("max_batch", C.c_uint32),
                ("max_points_per_ring", C.c_uint32), ("max_rings", C.c_uint32), ("drop_zero_points", C.c_uint32),
                ("layout", Layout), ("outputs", C.c_uint32), ("stream_hint", C.c_uint32),
                ("ring_ids", C.POINTER(C.c_uint16)), ("n_ring_ids", C.c_uint32)]


class GatherStep(C.Structure):
    """lfx_gather_step (include/lfx.h): one step of a grouped exchange, lfx_gather_payload2."""
    _fields_ = [("dst", C.c_int), ("slot", C.c_uint32), ("d_edge", C.c_void_p), ("d_surface", C.c_void_p), ("d_offsets", C.c_void_p),
                ("d_edge_all", C.c_void_p), ("d_surface_all", C.c_void_p), ("d_offsets_all", C.c_void_p), ("counts_out", C.c_void_p)]


OUT_FEATURES, OUT_LABELS, OUT_CURVATURE, OUT_SORTED_INDEX, OUT_ALL = 1, 2, 4, 8, 15
STREAM_UNKNOWN, STREAM_TURNED_RINGS, STREAM_NO_GRID, STREAM_GRID_WITH_HOLES = 0, 1, 2, 3


class ScanResult(C.Structure):
    _fields_ = [("n_points", C.c_uint32), ("labels", C.POINTER(C.c_uint8)), ("curvature", C.POINTER(C.c_double)),
                ("sorted_index", C.POINTER(C.c_uint32)), ("n_sorted", C.c_uint32), ("n_rings", C.c_uint32),
                ("ring_id", C.POINTER(C.c_uint16)), ("ring_count", C.POINTER(C.c_uint32)),
                ("ring_offset", C.POINTER(C.c_uint32)), ("ring_status", C.POINTER(C.c_uint8)),
                ("n_edge", C.c_uint32), ("edge_points", C.POINTER(C.c_float)), ("edge_index", C.POINTER(C.c_uint32)),
                ("n_surface", C.c_uint32), ("surface_points", C.POINTER(C.c_float)),
                ("surface_index", C.POINTER(C.c_uint32))]


class AlignResult(C.Structure):
    """lfx_align_result (OptimizationResult, optimization_result.hpp:35-43)."""
    _fields_ = [("pose", C.c_double * 12), ("error", C.c_double), ("error_scale", C.c_double), ("iteration", C.c_int32),
                ("code", C.c_int32)]


class AlignReport(C.Structure):
    """lfx_align_report: information matrix, its eigen-decomposition, covariance, degeneracy and fit counts at result.pose."""
    _fields_ = [("information", C.c_double * 36), ("eigenvalues", C.c_double * 6), ("eigenvectors", C.c_double * 36),
                ("covariance", C.c_double * 36), ("sigma2", C.c_double), ("min_eigenvalue_d", C.c_double), ("error", C.c_double),
                ("error_scale", C.c_double), ("rms_edge", C.c_double), ("rms_surface", C.c_double), ("n_edge", C.c_uint32),
                ("n_surface", C.c_uint32), ("n_edge_inliers", C.c_uint32), ("n_surface_inliers", C.c_uint32),
                ("n_surface_no_plane", C.c_uint32), ("rank", C.c_int32), ("degenerate", C.c_int32), ("valid", C.c_int32)]


class OdometryConfig(C.Structure):
    """lfx_odometry_config (EdgeSurfaceMap(n_local_scans) + the problem Localizer::Update runs)."""
    _fields_ = [("n_local_scans", C.c_uint32), ("n_neighbors", C.c_uint32), ("max_iter", C.c_int32), ("surface_leaf", C.c_float),
                ("edge_cell", C.c_float), ("surface_cell", C.c_float), ("edge_capacity_points", C.c_uint64),
                ("surface_capacity_points", C.c_uint64), ("initial_pose", C.c_double * 12)]


class OdometryResult(C.Structure):
    _fields_ = [("align", AlignResult), ("n_edge_map", C.c_uint32), ("n_surface_map", C.c_uint32), ("aligned", C.c_int32)]


class OdometryStoreView(C.Structure):
    _fields_ = [("n_scans", C.c_uint32), ("n_window_scans", C.c_uint32), ("n_added", C.c_uint64), ("dropped_scans", C.c_uint64),
                ("compactions", C.c_uint64), ("edge_points", C.c_void_p), ("surface_points", C.c_void_p), ("n_edge", C.c_uint64),
                ("n_surface", C.c_uint64), ("edge_window", C.c_void_p), ("surface_window", C.c_void_p), ("n_edge_window", C.c_uint32),
                ("n_surface_window", C.c_uint32), ("edge_offsets", C.POINTER(C.c_uint32)), ("surface_offsets", C.POINTER(C.c_uint32)),
                ("pose", C.c_double * 12)]


class MapperConfig(C.Structure):
    """lfx_mapper_config (MapBuilder's thresholds, map.hpp:89-90, and the map's capacity)."""
    _fields_ = [("translation_threshold", C.c_double), ("rotation_threshold", C.c_double),
                ("initial_capacity_points", C.c_uint64), ("max_points", C.c_uint64)]


class MapperStoreView(C.Structure):
    _fields_ = [("points", C.c_void_p), ("n_points", C.c_uint64), ("capacity_points", C.c_uint64), ("n_added", C.c_uint64),
                ("n_empty", C.c_uint64), ("n_too_close", C.c_uint64), ("has_pose", C.c_int32), ("last_pose", C.c_double * 12)]


class RollingMapConfig(C.Structure):
    """lfx_rolling_map_config: leaf size (m) and window dimensions (voxels) of the edge and the surface store."""
    _fields_ = [("edge_leaf", C.c_float), ("surface_leaf", C.c_float), ("edge_dims", C.c_uint32 * 3),
                ("surface_dims", C.c_uint32 * 3), ("match_half_extent", C.c_float * 3), ("n_neighbors", C.c_uint32),
                ("max_iter", C.c_int32), ("scan_surface_leaf", C.c_float), ("edge_cell", C.c_float), ("surface_cell", C.c_float),
                ("initial_pose", C.c_double * 12)]


class RollingMapResult(C.Structure):
    _fields_ = [("align", AlignResult), ("initial_pose", C.c_double * 12), ("n_edge_map", C.c_uint32), ("n_surface_map", C.c_uint32),
                ("aligned", C.c_int32), ("inserted", C.c_int32), ("recentered", C.c_int32)]


class RollingMapView(C.Structure):
    """lfx_rolling_map_view_t: per store ([0] edge, [1] surface) leaf, dims, origin, the counters and the live voxels."""
    _fields_ = [("leaf", C.c_float * 2), ("dims", (C.c_uint32 * 3) * 2), ("origin", (C.c_int32 * 3) * 2),
                ("n_inserted", C.c_uint64 * 2), ("n_merged", C.c_uint64 * 2), ("n_outside", C.c_uint64 * 2),
                ("n_nonfinite", C.c_uint64 * 2), ("n_live", C.c_uint64 * 2), ("pose", C.c_double * 12),
                ("correction", C.c_double * 12)]


ROLLING_EDGE, ROLLING_SURFACE = 0, 1
KEYFRAME_ADDED, KEYFRAME_EMPTY, KEYFRAME_TOO_CLOSE = 0, 1, 2
ERR_CAPACITY, ERR_OUT_OF_MEMORY, ERR_UNSUPPORTED_FIELD, ERR_FILE = -4, -6, -8, -9
ERR_INVALID_ARGUMENT, ERR_NO_TIME_FIELD = -1, -10


class TimeField(C.Structure):
    """lfx_time_field: where a record's firing time comes from (its index in the scan, or a field of the point record)."""
    _fields_ = [("source", C.c_uint32), ("offset", C.c_uint32), ("datatype", C.c_uint32), ("big_endian", C.c_uint32),
                ("scale", C.c_double)]


class Sweep(C.Structure):
    """lfx_sweep: start and end time of a sweep and the sensor's motion over it (the frame at t1 in the frame at t0)."""
    _fields_ = [("t0", C.c_double), ("t1", C.c_double), ("motion", C.c_double * 12)]


class Trajectory(C.Structure):
    """lfx_trajectory: the sensor's poses at n_knots times within a sweep and the time the records are brought to."""
    _fields_ = [("n_knots", C.c_uint32), ("times", C.POINTER(C.c_double)), ("poses", C.POINTER(C.c_double)), ("t_ref", C.c_double)]


MAX_TRAJECTORY_KNOTS, TRAJECTORY_SEGMENT_DOUBLES = 64, 24
TIME_FROM_INDEX, TIME_FROM_FIELD = 0, 1
DESKEW_TO_START, DESKEW_TO_END = 0, 1


class ScanContextConfig(C.Structure):
    """lfx_scan_context_config: the polar grid of a scan-context descriptor (R rings x S sectors out to max_radius)."""
    _fields_ = [("n_rings", C.c_uint32), ("n_sectors", C.c_uint32), ("max_radius", C.c_float), ("min_radius", C.c_float),
                ("sensor_height", C.c_float)]


class PlaceMatch(C.Structure):
    """lfx_place_match: one entry of a place index as a query sees it."""
    _fields_ = [("entry", C.c_uint32), ("shift", C.c_uint32), ("distance", C.c_double), ("yaw", C.c_double)]


SCAN_CONTEXT_MAX_RINGS, SCAN_CONTEXT_MAX_SECTORS, PLACE_MAX_MATCHES = 40, 120, 16
PLACE_NO_ENTRY = 0xFFFFFFFF


class SegmentConfig(C.Structure):
    """lfx_segment_config: the range image (H rows x W columns) and the thresholds of the ground, join and size tests."""
    _fields_ = [("n_rows", C.c_uint32), ("n_columns", C.c_uint32), ("row_step", C.c_float), ("min_range", C.c_float),
                ("max_range", C.c_float), ("ground_first_row", C.c_uint32), ("ground_last_row", C.c_uint32), ("ground_tan", C.c_float),
                ("segment_tan", C.c_float), ("segment_min_points", C.c_uint32), ("small_min_points", C.c_uint32),
                ("small_min_rows", C.c_uint32)]


SEG_NONE, SEG_GROUND, SEG_SEGMENT, SEG_CLUTTER = 0, 1, 2, 3
SEG_EDGE_MASK_DEFAULT, SEG_SURFACE_MASK_DEFAULT = 1 << SEG_SEGMENT, (1 << SEG_GROUND) | (1 << SEG_SEGMENT)
SEG_NO_ID = 0xFFFFFFFF
SEGMENT_MAX_ROWS, SEGMENT_MAX_COLUMNS, SEGMENT_BUDGET_CELLS = 128, 4096, 1 << 24


class PoseGraphConfig(C.Structure):
    """lfx_pose_graph_config: the capacities a pose graph is allocated for and the optimiser's settings."""
    _fields_ = [("max_nodes", C.c_uint32), ("max_edges", C.c_uint32), ("max_loop_edges", C.c_uint32), ("max_iter", C.c_uint32),
                ("damping", C.c_double), ("tolerance", C.c_double), ("huber_delta", C.c_double)]


class PoseGraphEdge(C.Structure):
    """lfx_pose_graph_edge: Z = T_i^-1 T_j with its information in the residual's coordinates."""
    _fields_ = [("i", C.c_uint32), ("j", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32), ("z", C.c_double * 12),
                ("information", C.c_double * 36)]


class PoseGraphResult(C.Structure):
    _fields_ = [("code", C.c_int32), ("iterations", C.c_int32), ("chi2_initial", C.c_double), ("chi2_final", C.c_double),
                ("max_step", C.c_double), ("n_chain", C.c_uint32), ("n_loop", C.c_uint32), ("n_robust_downweighted", C.c_uint32),
                ("reserved", C.c_uint32)]


class PoseGraphInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("n_edges", C.c_uint32), ("n_chain", C.c_uint32), ("n_loop", C.c_uint32),
                ("device_bytes", C.c_uint64)]


EDGE_ROBUST = 1
POSE_GRAPH_CONVERGED, POSE_GRAPH_MAX_ITERATIONS, POSE_GRAPH_DIVERGED, POSE_GRAPH_NOT_POSITIVE_DEFINITE = 0, 1, 2, 3
POSE_GRAPH_MAX_LOOP_EDGES = 10000
POSE_GRAPH_EDGE_DTYPE = [("i", "<u4"), ("j", "<u4"), ("flags", "<u4"), ("reserved", "<u4"), ("z", "<f8", 12), ("information", "<f8", 36)]
"""lfx_pose_graph_edge as a numpy record (400 bytes)."""


class PoseGraphPrior(C.Structure):
    """lfx_pose_graph_prior: an absolute fix of one node, a full pose or (PRIOR_POSITION) a position with a lever arm."""
    _fields_ = [("node", C.c_uint32), ("flags", C.c_uint32), ("z", C.c_double * 12), ("information", C.c_double * 36),
                ("lever", C.c_double * 3)]


class PoseGraphPriorInfo(C.Structure):
    _fields_ = [("n_priors", C.c_uint32), ("max_priors", C.c_uint32), ("n_downweighted", C.c_uint32), ("reserved", C.c_uint32),
                ("chi2", C.c_double)]


PRIOR_ROBUST, PRIOR_POSITION = 1, 2
POSE_GRAPH_PRIOR_DTYPE = [("node", "<u4"), ("flags", "<u4"), ("z", "<f8", 12), ("information", "<f8", 36), ("lever", "<f8", 3)]
"""lfx_pose_graph_prior as a numpy record (416 bytes)."""


class KeyframesConfig(C.Structure):
    """lfx_keyframes_config: the capacities a keyframe store is allocated for ([0] edge, [1] surface records)."""
    _fields_ = [("max_keyframes", C.c_uint32), ("reserved", C.c_uint32), ("max_points", C.c_uint64 * 2)]


class KeyframesInfo(C.Structure):
    _fields_ = [("n_keyframes", C.c_uint32), ("max_keyframes", C.c_uint32), ("n_points", C.c_uint64 * 2), ("max_points", C.c_uint64 * 2),
                ("device_bytes", C.c_uint64)]


class KeyframesStoreView(C.Structure):
    _fields_ = [("points", C.c_void_p * 2), ("begin", C.c_void_p * 2), ("poses", C.c_void_p), ("n_keyframes", C.c_uint32),
                ("reserved", C.c_uint32), ("n_points", C.c_uint64 * 2)]


class KeyframesClouds(C.Structure):
    """lfx_keyframes_clouds: n device clouds of one kind, addressed as lfx_mapper_add addresses its clouds."""
    _fields_ = [("d_points", C.c_void_p), ("d_begin", C.c_void_p), ("d_count", C.c_void_p), ("count_stride", C.c_uint32),
                ("reserved", C.c_uint32), ("total_points", C.c_uint64)]


class KeyframesSubmapResult(C.Structure):
    _fields_ = [("n_selected", C.c_uint32), ("n_written_keyframes", C.c_uint32), ("n_points", C.c_uint64), ("first_id", C.c_uint32),
                ("last_id", C.c_uint32), ("truncated", C.c_int32), ("reserved", C.c_uint32)]


class KeyframesFlagsInfo(C.Structure):
    """lfx_keyframes_flags_info_t: the flags a store keeps (lfx_keyframes_reserve_flags) and how many are set."""
    _fields_ = [("reserved", C.c_int32), ("pad", C.c_uint32), ("device_bytes", C.c_uint64), ("n_flagged", C.c_uint64 * 2)]


KEYFRAMES_EDGE, KEYFRAMES_SURFACE = 0, 1
KEYFRAMES_NO_ID = 0xFFFFFFFF


class VoxelFilterConfig(C.Structure):
    """lfx_voxel_filter_config: 2^log2_slots voxel entries, max_records ranks between two resets."""
    _fields_ = [("log2_slots", C.c_uint32), ("reserved", C.c_uint32), ("max_records", C.c_uint64)]


class VoxelFilterResult(C.Structure):
    """lfx_voxel_filter_result: what an emit reports about the records since the reset and the voxels it wrote."""
    _fields_ = [(n, C.c_uint64) for n in ("n_records", "n_accumulated", "n_nonfinite", "n_out_of_range", "n_table_full", "n_voxels", "n_written")]


class VoxelFilterInfo(C.Structure):
    _fields_ = [("slots", C.c_uint64), ("max_records", C.c_uint64), ("n_records", C.c_uint64), ("device_bytes", C.c_uint64),
                ("leaf", C.c_float), ("reserved", C.c_uint32)]


class OccupancyConfig(C.Structure):
    """lfx_occupancy_config: the virtual scan (W beams), the grid (cells, resolution, origin), the gates and the height band."""
    _fields_ = [("n_beams", C.c_uint32), ("max_scans", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("resolution", C.c_float), ("min_range", C.c_float), ("max_range", C.c_float), ("z_min", C.c_float), ("z_max", C.c_float),
                ("chunk_scans", C.c_uint32), ("origin_x", C.c_double), ("origin_y", C.c_double)]


class OccupancyEmitConfig(C.Structure):
    """lfx_occupancy_emit_config: the log-odds weights and clamps (hundredths) and the observations a known cell needs."""
    _fields_ = [("w_hit", C.c_int32), ("w_miss", C.c_int32), ("l_min", C.c_int32), ("l_max", C.c_int32), ("min_observations", C.c_uint32),
                ("reserved", C.c_uint32)]


class OccupancyInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("n_scans", "max_scans", "n_beams", "width", "height", "chunk_scans", "window", "reserved")] + \
        [("device_bytes", C.c_uint64)]


class OccupancyView(C.Structure):
    _fields_ = [("beams", C.c_void_p), ("poses", C.c_void_p), ("hits", C.c_void_p), ("misses", C.c_void_p), ("n_scans", C.c_uint32),
                ("reserved", C.c_uint32)]


class OccupancyCounters(C.Structure):
    """lfx_occupancy_counters_t: what the renders since the last clear cast and voted."""
    _fields_ = [(n, C.c_uint64) for n in ("n_hit_beams", "n_clear_beams", "n_skipped_beams", "n_occupied_votes", "n_free_votes", "n_window_miss")]


OCCUPANCY_NONE, OCCUPANCY_HIT, OCCUPANCY_CLEAR = 0, 1, 2


class DistanceConfig(C.Structure):
    """lfx_distance_config: what counts as an obstacle, the cap in cells (0: none) and whether the inside field is wanted."""
    _fields_ = [("occupied_percent", C.c_int32), ("unknown_is_obstacle", C.c_uint32), ("max_cells", C.c_uint32), ("inside", C.c_uint32),
                ("reserved", C.c_uint32)]


class DistanceCostConfig(C.Structure):
    """lfx_distance_cost_config: nav2's inflation layer -- the two radii in metres, the decay and whether unknown cells cost 255."""
    _fields_ = [("inscribed_radius", C.c_float), ("inflation_radius", C.c_float), ("cost_scaling_factor", C.c_float), ("track_unknown", C.c_uint32)]


class DistanceInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "transformed", "max_cells", "inside", "reserved")] + [("device_bytes", C.c_uint64)]


class DistanceView(C.Structure):
    _fields_ = [("classes", C.c_void_p), ("d2", C.c_void_p), ("i2", C.c_void_p)]


class DistanceStats(C.Structure):
    """lfx_distance_stats_t: the last transform's cells by class, its FAR cells and the largest d2 that is not FAR."""
    _fields_ = [(n, C.c_uint64) for n in ("n_obstacle", "n_unknown", "n_far", "max_d2")]


DISTANCE_FAR = 0xFFFFFFFF
DISTANCE_FREE, DISTANCE_UNKNOWN, DISTANCE_OBSTACLE = 0, 1, 2
DISTANCE_MAX_COST_CELLS = 1024


class GridMatchConfig(C.Structure):
    """lfx_grid_match_config: the grid's geometry (lfx_distance carries none), the scans the object holds and the largest window."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("resolution", C.c_float), ("max_scans", C.c_uint32), ("max_beams", C.c_uint32),
                ("max_half_x", C.c_uint32), ("max_half_y", C.c_uint32), ("max_half_theta", C.c_uint32), ("origin_x", C.c_double), ("origin_y", C.c_double)]


class GridMatchTableConfig(C.Structure):
    """lfx_grid_match_table_config: the likelihood field's Gaussian -- sigma and reach in metres, the score of distance 0."""
    _fields_ = [("sigma", C.c_float), ("max_distance", C.c_float), ("peak", C.c_uint32), ("reserved", C.c_uint32)]


class GridMatchSearchConfig(C.Structure):
    """lfx_grid_match_search_config: the window -- half sides in candidates, the cells between two, headings either side and their step."""
    _fields_ = [("half_x", C.c_uint32), ("half_y", C.c_uint32), ("step_cells", C.c_uint32), ("half_theta", C.c_uint32), ("theta_step", C.c_double)]


class GridMatchInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "max_scans", "max_beams", "max_half_x", "max_half_y", "max_half_theta", "field_set",
                                          "table_cells", "n_scans", "n_beams", "reserved")] + [("device_bytes", C.c_uint64)]


class GridMatchView(C.Structure):
    _fields_ = [("field", C.c_void_p), ("points", C.c_void_p), ("n_points", C.c_void_p)]


GRID_MATCH_MAX_CELLS, GRID_MATCH_MAX_HALF, GRID_MATCH_MAX_HALF_THETA = 64, 256, 180
OCCUPANCY_MAX_BEAMS, OCCUPANCY_MAX_SIDE = 4096, 16384


class VisibilityConfig(C.Structure):
    """lfx_visibility_config: the range images, the pairs that vote and the decision (include/lfx.h, the visibility section)."""
    _fields_ = [("n_rows", C.c_uint32), ("n_columns", C.c_uint32), ("elev_min", C.c_float), ("elev_step", C.c_float),
                ("min_range", C.c_float), ("max_range", C.c_float), ("radius", C.c_float), ("margin_abs", C.c_float),
                ("margin_rel", C.c_float), ("guard", C.c_uint32), ("min_through", C.c_uint32), ("agree_weight", C.c_uint32),
                ("reserved", C.c_uint32)]


class VisibilityInfo(C.Structure):
    _fields_ = [("config", VisibilityConfig), ("max_window", C.c_uint32), ("max_resident_images", C.c_uint32), ("device_bytes", C.c_uint64)]


class VisibilityResult(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64), ("n_records", C.c_uint64 * 2), ("n_voted", C.c_uint64 * 2), ("n_dynamic", C.c_uint64 * 2),
                ("occupied_cells", C.c_uint64), ("total_cells", C.c_uint64), ("n_viewer_chunks", C.c_uint32), ("reserved", C.c_uint32)]


VISIBILITY_MAX_WINDOW = 65536
VISIBILITY_SCRATCH_WORDS = 1 << 22


class PlaceGate(C.Structure):
    """lfx_place_gate: the entries one query of lfx_place_db_query_gated may match (e < limit, near pose `pose`)."""
    _fields_ = [("limit", C.c_uint32), ("pose", C.c_uint32)]


PLACE_NO_POSE = 0xFFFFFFFF


class LoopCloserConfig(C.Structure):
    """lfx_loop_closer_config: which revisits are looked for, what they are aligned against, and what is accepted."""
    _fields_ = [("min_gap", C.c_uint32), ("n_candidates", C.c_uint32), ("max_verify", C.c_uint32), ("submap_half_window", C.c_uint32),
                ("search_radius", C.c_double), ("max_distance", C.c_double), ("submap_radius", C.c_double),
                ("submap_capacity", C.c_uint64 * 2), ("map_cell_size", C.c_float), ("surface_leaf", C.c_float),
                ("n_neighbors", C.c_uint32), ("max_iter", C.c_int32), ("max_rms_edge", C.c_double), ("max_rms_surface", C.c_double),
                ("min_inlier_share", C.c_double), ("reject_degenerate", C.c_int32), ("scale_by_sigma2", C.c_int32),
                ("downsample_capacity", C.c_uint64)]


class LoopClosure(C.Structure):
    """lfx_loop_closure: one verification -- the candidate, the alignment and its report, both submaps, the edge."""
    _fields_ = [("query", C.c_uint32), ("candidate", C.c_uint32), ("accepted", C.c_int32), ("reason", C.c_int32), ("match", PlaceMatch),
                ("result", AlignResult), ("report", AlignReport), ("submap", KeyframesSubmapResult * 2), ("edge", PoseGraphEdge)]


class LoopCloserResult(C.Structure):
    _fields_ = [("n_detected", C.c_uint32), ("n_verified", C.c_uint32), ("n_accepted", C.c_uint32), ("followed", C.c_int32),
                ("graph", PoseGraphResult)]


class LoopCloserInfo(C.Structure):
    _fields_ = [("device_bytes", C.c_uint64)]


(LOOP_ACCEPTED, LOOP_NO_CANDIDATE, LOOP_EMPTY_QUERY, LOOP_EMPTY_SUBMAP, LOOP_ALIGN_FAILED, LOOP_NO_REPORT, LOOP_RANK, LOOP_DEGENERATE,
 LOOP_RMS_EDGE, LOOP_RMS_SURFACE, LOOP_INLIERS, LOOP_SIGMA2) = range(12)


class DeviceView(C.Structure):
    _fields_ = [("batch", C.c_uint32), ("max_rings", C.c_uint32), ("ring_capacity", C.c_uint32)] + \
        [(n, C.c_void_p) for n in (
            "scan_begin", "labels_sorted", "curvature_sorted", "sorted_index", "scan_info",
            "ring_count", "ring_status", "edge_points", "edge_index", "surface_points", "surface_index")]


EXPORTS = [
    "lfx_default_params", "lfx_launch_params", "lfx_create", "lfx_destroy", "lfx_last_error",
    "lfx_status_string", "lfx_ring_message", "lfx_range_message", "lfx_extract", "lfx_extract_submit", "lfx_extract_wait", "lfx_extract_batch", "lfx_extract_batch_device",
    "lfx_device_results", "lfx_batch_points", "lfx_batch_status", "lfx_scan_routes", "lfx_host_alloc", "lfx_host_free", "lfx_comm_unique_id", "lfx_comm_create",
    "lfx_comm_destroy", "lfx_comm_stats", "lfx_gather_counts", "lfx_gather_payload", "lfx_gather", "lfx_voxel_downsample", "lfx_downsample_surface",
    "lfx_map_create", "lfx_map_create_host", "lfx_map_destroy", "lfx_map_info", "lfx_map_nearest",
    "lfx_scan_to_map_residuals", "lfx_edge_residuals", "lfx_align_message", "lfx_scan_to_map_align", "lfx_align_point_pairs",
    "lfx_localize_batch", "lfx_localize_host",
    "lfx_scan_to_map_align_report", "lfx_localize_batch_report", "lfx_localize_host_report", "lfx_align_covariance_ros",
    "lfx_odometry_set_reports", "lfx_odometry_reports",
    "lfx_odometry_default_config", "lfx_odometry_create", "lfx_odometry_destroy", "lfx_odometry_update_batch", "lfx_odometry_update",
    "lfx_odometry_update_host", "lfx_odometry_add", "lfx_odometry_pose", "lfx_odometry_view", "lfx_odometry_save",
    "lfx_pcd_read", "lfx_pcd_write", "lfx_pose_diff", "lfx_mapper_default_config", "lfx_mapper_create", "lfx_mapper_destroy",
    "lfx_mapper_add", "lfx_mapper_add_host", "lfx_mapper_view", "lfx_mapper_save",
    "lfx_rolling_map_default_config", "lfx_rolling_map_create", "lfx_rolling_map_destroy", "lfx_rolling_map_recenter",
    "lfx_rolling_map_insert", "lfx_rolling_map_insert_host", "lfx_rolling_map_extract", "lfx_rolling_map_view",
    "lfx_rolling_map_save", "lfx_rolling_map_update_batch", "lfx_rolling_map_pose",
    "lfx_layout_from_fields", "lfx_pack_xyz", "lfx_pack_xyz12", "lfx_pack_colored", "lfx_pack_features", "lfx_download_scan", "lfx_stage_ring", "lfx_stage_convolution1d",
    "lfx_stage_ring_projection", "lfx_label_to_color", "lfx_color_points_by_label", "lfx_set_profiling", "lfx_set_profiling_interval", "lfx_kernel_times", "lfx_kernel_name",
    "lfx_time_field_from_fields", "lfx_motion_between", "lfx_motion_twist", "lfx_motion_scale", "lfx_deskew_batch",
    "lfx_odometry_update_batch_deskewed",
    "lfx_trajectory_segments", "lfx_trajectory_from_gyro", "lfx_deskew_batch_trajectory", "lfx_odometry_update_batch_trajectory",
    "lfx_scan_context_default_config", "lfx_scan_context_tables", "lfx_scan_context_batch", "lfx_place_db_create",
    "lfx_place_db_destroy", "lfx_place_db_add", "lfx_place_db_add_host", "lfx_place_db_size", "lfx_place_db_download",
    "lfx_place_db_query", "lfx_place_db_query_gated",
    "lfx_loop_closer_default_config", "lfx_loop_closer_create", "lfx_loop_closer_destroy", "lfx_loop_closer_info", "lfx_loop_closer_detect",
    "lfx_loop_closer_verify", "lfx_loop_closer_update", "lfx_loop_closer_set_masked", "lfx_loop_closer_get_masked",
    "lfx_segment_default_config", "lfx_segment_tables", "lfx_segment_batch", "lfx_pack_features_segmented",
    "lfx_pose_graph_default_config", "lfx_pose_graph_create", "lfx_pose_graph_destroy", "lfx_pose_graph_info", "lfx_pose_graph_add_nodes",
    "lfx_pose_graph_set_fixed", "lfx_pose_graph_add_edges", "lfx_pose_graph_optimize", "lfx_pose_graph_poses", "lfx_pose_graph_set_poses",
    "lfx_pose_graph_view", "lfx_pose_graph_edge_chi2", "lfx_pose_graph_edge_information",
    "lfx_pose_graph_reserve_priors", "lfx_pose_graph_add_priors", "lfx_pose_graph_release_first", "lfx_pose_graph_prior_chi2",
    "lfx_pose_graph_prior_info",
    "lfx_pose_graph_reserve_marginals", "lfx_pose_graph_marginals", "lfx_pose_graph_joint_covariances", "lfx_pose_graph_relative_covariance",
    "lfx_keyframes_default_config", "lfx_keyframes_create", "lfx_keyframes_destroy", "lfx_keyframes_info", "lfx_keyframes_view",
    "lfx_keyframes_add", "lfx_keyframes_add_host", "lfx_keyframes_set_poses", "lfx_keyframes_poses", "lfx_keyframes_follow",
    "lfx_keyframes_build", "lfx_keyframes_submap", "lfx_keyframes_save", "lfx_keyframes_build_masked",
    "lfx_keyframes_reserve_flags", "lfx_keyframes_flags", "lfx_keyframes_set_flags", "lfx_keyframes_clear_flags", "lfx_keyframes_flags_info",
    "lfx_keyframes_submap_masked", "lfx_keyframes_save_masked",
    "lfx_visibility_default_config", "lfx_visibility_tables", "lfx_visibility_create", "lfx_visibility_destroy", "lfx_visibility_info",
    "lfx_visibility_run",
    "lfx_voxel_filter_default_config", "lfx_voxel_filter_create", "lfx_voxel_filter_destroy", "lfx_voxel_filter_info", "lfx_voxel_filter_reset",
    "lfx_voxel_filter_add", "lfx_voxel_filter_add_host", "lfx_voxel_filter_emit", "lfx_voxel_filter_add_keyframes", "lfx_keyframes_save_filtered",
    "lfx_occupancy_default_config", "lfx_occupancy_tables", "lfx_occupancy_emit_default_config", "lfx_occupancy_emit_table",
    "lfx_occupancy_create", "lfx_occupancy_destroy", "lfx_occupancy_info", "lfx_occupancy_view", "lfx_occupancy_add_batch",
    "lfx_occupancy_set_poses", "lfx_occupancy_poses", "lfx_occupancy_follow", "lfx_occupancy_truncate", "lfx_occupancy_clear", "lfx_occupancy_render",
    "lfx_occupancy_counters", "lfx_occupancy_emit", "lfx_occupancy_write_map", "lfx_occupancy_save",
    "lfx_distance_default_config", "lfx_distance_cost_default_config", "lfx_distance_cost_table_size", "lfx_distance_cost_table",
    "lfx_distance_create", "lfx_distance_destroy", "lfx_distance_info", "lfx_distance_from_grid", "lfx_distance_from_occupancy",
    "lfx_distance_view", "lfx_distance_metres", "lfx_distance_costmap", "lfx_distance_stats",
    "lfx_grid_match_default_config", "lfx_grid_match_table_default_config", "lfx_grid_match_search_default_config", "lfx_grid_match_table_size",
    "lfx_grid_match_table", "lfx_grid_match_search_size", "lfx_grid_match_rotations", "lfx_grid_match_candidate", "lfx_grid_match_pose3",
    "lfx_grid_match_create", "lfx_grid_match_destroy", "lfx_grid_match_info", "lfx_grid_match_view", "lfx_grid_match_set_field",
    "lfx_grid_match_set_scans", "lfx_grid_match_set_scans_occupancy", "lfx_grid_match_score", "lfx_grid_match_search",
    "lfx_route_choice", "lfx_set_log_callback", "lfx_box_calibration", "lfx_gather_counts_slot", "lfx_gather_payload2", "lfx_set_ring_ids",
]
"""Every symbol include/lfx.h declares (tests/test_abi.py checks the library exports each)."""

HOOKS_LIB_PATH = os.path.join(_HERE, "_lib", "liblfx_testhooks.so")
"""Test infrastructure: the same library built -DLFX_TEST_HOOKS -- the only build whose lfx_create reads the LFX_DEBUG_*
switches (route pins, span variants, ablation flags) and whose gather takes another RCCL (LFX_RCCL_LIB)."""

_libs = {}


def load(test_hooks=False):
    """The library (test_hooks: its test-hooks build; with LFX_LIB_PATH set, that file either way)."""
    path = LIB_PATH if (not test_hooks or os.environ.get("LFX_LIB_PATH")) else HOOKS_LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise ImportError(
            "liblfx.so is not built (%s): run `python __graft_entry__.py` -- there is no CPU fallback" % path)
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 (SONAME libamdhip64.so.7,
    # the name liblfx.so needs).  Loading torch first makes liblfx.so bind to that copy; the other
    # order would put a second runtime into the process, and the later one sees no GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
    L.lfx_default_params.argtypes = [C.POINTER(Params)]
    L.lfx_default_params.restype = None
    L.lfx_launch_params.argtypes = [C.POINTER(Params)]
    L.lfx_launch_params.restype = None
    L.lfx_create.argtypes = [C.POINTER(vp), i32, C.POINTER(Params), C.POINTER(Config)]
    L.lfx_destroy.argtypes = [vp]
    L.lfx_destroy.restype = None
    L.lfx_last_error.argtypes = [vp]
    L.lfx_last_error.restype = C.c_char_p
    L.lfx_status_string.argtypes = [i32]
    L.lfx_status_string.restype = C.c_char_p
    L.lfx_ring_message.argtypes = [i32, u32, C.POINTER(Params), C.c_char_p, C.c_size_t]
    L.lfx_range_message.argtypes = [i32, C.c_char_p, C.c_char_p, C.c_longlong, C.c_longlong, C.c_char_p, C.c_size_t]
    L.lfx_extract.argtypes = [vp, vp, C.c_size_t, C.POINTER(ScanResult)]
    L.lfx_extract_submit.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_uint64)]
    L.lfx_extract_wait.argtypes = [vp, C.c_uint64, C.POINTER(ScanResult)]
    L.lfx_extract_batch.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t), u32, C.POINTER(ScanResult)]
    L.lfx_extract_batch_device.argtypes = [vp, vp, C.POINTER(u32), u32, vp]
    L.lfx_device_results.argtypes = [vp, C.POINTER(DeviceView)]
    L.lfx_batch_points.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.lfx_batch_status.argtypes = [vp, vp, C.POINTER(u32)]
    L.lfx_scan_routes.argtypes = [vp, vp, vp]
    L.lfx_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.lfx_host_free.argtypes = [vp, vp]
    L.lfx_host_free.restype = None
    L.lfx_comm_unique_id.argtypes = [vp]
    L.lfx_comm_create.argtypes = [vp, vp, i32, i32, C.POINTER(vp)]
    L.lfx_comm_destroy.argtypes = [vp]
    L.lfx_comm_destroy.restype = None
    L.lfx_comm_stats.argtypes = [vp, vp]
    L.lfx_gather_counts.argtypes = [vp, vp, vp, u32, vp]
    L.lfx_gather_payload.argtypes = [vp, vp, i32, vp, vp, vp, u32, u32, vp, vp, vp, C.c_size_t, vp, vp]
    L.lfx_gather_counts_slot.argtypes = [vp, vp, u32, vp, u32, vp]
    L.lfx_gather_payload2.argtypes = [vp, vp, C.POINTER(GatherStep), u32, u32, u32, C.c_size_t, vp]
    L.lfx_voxel_downsample.argtypes = [vp, vp, vp, vp, u32, u32, C.c_size_t, C.c_float, vp, vp, vp, vp]
    L.lfx_map_create.argtypes = [vp, vp, u32, C.c_float, C.POINTER(vp), vp]
    L.lfx_map_create_host.argtypes = [vp, vp, u32, C.c_float, C.POINTER(vp), vp]
    L.lfx_map_destroy.argtypes = [vp]
    L.lfx_map_destroy.restype = None
    L.lfx_map_info.argtypes = [vp, C.POINTER(u32), C.POINTER(C.c_float), C.POINTER(i32)]
    L.lfx_map_nearest.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp, vp]
    L.lfx_scan_to_map_residuals.argtypes = [vp, i32, vp, C.POINTER(C.c_double), u32, vp, vp, vp, u32, u32, u32, vp, vp, vp]
    L.lfx_edge_residuals.argtypes = [vp, vp, C.POINTER(C.c_double), u32, vp, vp, vp]
    L.lfx_align_message.argtypes = [i32]
    L.lfx_align_message.restype = C.c_char_p
    pd, pres = C.POINTER(C.c_double), C.POINTER(AlignResult)
    L.lfx_scan_to_map_align.argtypes = [vp, vp, vp, u32, i32, vp, vp, vp, u32, u32, C.c_size_t, vp, vp, vp, u32, u32,
                                        C.c_size_t, u32, pd, pres, vp]
    L.lfx_align_point_pairs.argtypes = [vp, vp, vp, vp, vp, u32, C.c_size_t, u32, i32, pd, pres, vp]
    L.lfx_localize_batch.argtypes = [vp, vp, vp, u32, i32, C.c_float, u32, pd, pres, vp]
    L.lfx_localize_host.argtypes = [vp, vp, vp, u32, i32, C.c_float, vp, u32, vp, u32, pd, pres, vp]
    prep = C.POINTER(AlignReport)
    L.lfx_scan_to_map_align_report.argtypes = L.lfx_scan_to_map_align.argtypes[:-1] + [prep, vp]
    L.lfx_localize_batch_report.argtypes = [vp, vp, vp, u32, i32, C.c_float, u32, pd, pres, prep, vp]
    L.lfx_localize_host_report.argtypes = [vp, vp, vp, u32, i32, C.c_float, vp, u32, vp, u32, pd, pres, prep, vp]
    L.lfx_align_covariance_ros.argtypes = [pd, pd, pd]
    L.lfx_odometry_set_reports.argtypes = [vp, C.c_int]
    L.lfx_odometry_reports.argtypes = [vp, prep, u32, C.POINTER(u32)]
    L.lfx_downsample_surface.argtypes = [vp, C.c_float, vp, vp, vp, vp]
    L.lfx_odometry_default_config.argtypes = [C.POINTER(OdometryConfig)]
    L.lfx_odometry_default_config.restype = None
    L.lfx_odometry_create.argtypes = [vp, C.POINTER(OdometryConfig), C.POINTER(vp)]
    L.lfx_odometry_destroy.argtypes = [vp]
    L.lfx_odometry_destroy.restype = None
    L.lfx_odometry_update_batch.argtypes = [vp, vp, u32, C.POINTER(OdometryResult), vp]
    L.lfx_odometry_update.argtypes = [vp, vp, vp, u32, vp, u32, C.POINTER(OdometryResult), vp]
    L.lfx_odometry_update_host.argtypes = [vp, vp, vp, u32, vp, u32, C.POINTER(OdometryResult), vp]
    L.lfx_odometry_add.argtypes = [vp, vp, pd, vp, u32, vp, u32, vp]
    L.lfx_odometry_pose.argtypes = [vp, pd]
    L.lfx_odometry_view.argtypes = [vp, C.POINTER(OdometryStoreView)]
    L.lfx_odometry_save.argtypes = [vp, vp, C.c_char_p, C.POINTER(i32), vp]
    u64, p64 = C.c_uint64, C.POINTER(C.c_uint64)
    L.lfx_pcd_read.argtypes = [C.c_char_p, vp, u64, i32, p64, p64, C.c_char_p, C.c_size_t]
    L.lfx_pcd_write.argtypes = [C.c_char_p, vp, u64, C.c_char_p, C.c_size_t]
    L.lfx_pose_diff.argtypes = [pd, pd, pd, pd]
    L.lfx_mapper_default_config.argtypes = [C.POINTER(MapperConfig)]
    L.lfx_mapper_default_config.restype = None
    L.lfx_mapper_create.argtypes = [vp, C.POINTER(MapperConfig), C.POINTER(vp)]
    L.lfx_mapper_destroy.argtypes = [vp]
    L.lfx_mapper_destroy.restype = None
    L.lfx_mapper_add.argtypes = [vp, vp, vp, vp, vp, u32, u32, C.c_size_t, pd, vp, vp]
    L.lfx_mapper_add_host.argtypes = [vp, vp, vp, u32, pd, vp, vp]
    L.lfx_mapper_view.argtypes = [vp, C.POINTER(MapperStoreView)]
    L.lfx_mapper_save.argtypes = [vp, vp, C.c_char_p, C.POINTER(i32), vp]
    L.lfx_rolling_map_default_config.argtypes = [C.POINTER(RollingMapConfig)]
    L.lfx_rolling_map_default_config.restype = None
    L.lfx_rolling_map_create.argtypes = [vp, C.POINTER(RollingMapConfig), C.POINTER(vp)]
    L.lfx_rolling_map_destroy.argtypes = [vp]
    L.lfx_rolling_map_destroy.restype = None
    L.lfx_rolling_map_recenter.argtypes = [vp, pd]
    L.lfx_rolling_map_insert.argtypes = [vp, vp, i32, vp, vp, vp, u32, u32, C.c_size_t, pd, vp]
    L.lfx_rolling_map_insert_host.argtypes = [vp, vp, i32, vp, u32, pd, vp]
    L.lfx_rolling_map_extract.argtypes = [vp, vp, i32, pd, pd, vp, u64, p64, vp]
    L.lfx_rolling_map_view.argtypes = [vp, vp, C.POINTER(RollingMapView), vp]
    L.lfx_rolling_map_save.argtypes = [vp, vp, C.c_char_p, C.POINTER(i32), vp]
    L.lfx_rolling_map_update_batch.argtypes = [vp, vp, u32, pd, C.POINTER(RollingMapResult), vp]
    L.lfx_rolling_map_pose.argtypes = [vp, pd]
    L.lfx_gather.argtypes = [vp, vp, i32, vp, vp, vp, u32, u32, vp, vp, vp, C.c_size_t, vp, vp]
    L.lfx_layout_from_fields.argtypes = [C.POINTER(PointField), C.c_uint32, C.c_uint32, C.c_int, C.POINTER(Layout)]
    L.lfx_time_field_from_fields.argtypes = [C.POINTER(PointField), C.c_uint32, C.c_uint32, C.c_int, C.POINTER(TimeField)]
    L.lfx_motion_between.argtypes = [pd, pd, pd]
    L.lfx_motion_twist.argtypes = [pd, pd, pd]
    L.lfx_motion_scale.argtypes = [pd, C.c_double, pd]
    L.lfx_deskew_batch.argtypes = [vp, C.POINTER(TimeField), C.POINTER(Sweep), u32, i32, vp, vp, vp]
    L.lfx_odometry_update_batch_deskewed.argtypes = [vp, vp, C.POINTER(TimeField), pd, C.c_double, i32, u32,
                                                     C.POINTER(OdometryResult), vp]
    L.lfx_trajectory_segments.argtypes = [C.POINTER(Trajectory), pd]
    L.lfx_trajectory_from_gyro.argtypes = [pd, pd, u32, pd, pd, pd]
    L.lfx_deskew_batch_trajectory.argtypes = [vp, C.POINTER(TimeField), C.POINTER(Trajectory), u32, vp, vp, vp]
    L.lfx_odometry_update_batch_trajectory.argtypes = [vp, vp, C.POINTER(TimeField), C.POINTER(Trajectory), u32,
                                                       C.POINTER(OdometryResult), vp]
    psc = C.POINTER(ScanContextConfig)
    L.lfx_scan_context_default_config.argtypes = [psc]
    L.lfx_scan_context_default_config.restype = None
    L.lfx_scan_context_tables.argtypes = [psc, pd, pd, pd]
    L.lfx_scan_context_batch.argtypes = [vp, psc, u32, vp, vp]
    L.lfx_place_db_create.argtypes = [vp, psc, u32, C.POINTER(vp)]
    L.lfx_place_db_destroy.argtypes = [vp]
    L.lfx_place_db_destroy.restype = None
    L.lfx_place_db_add.argtypes = [vp, vp, vp, u32, vp]
    L.lfx_place_db_add_host.argtypes = [vp, vp, vp, u32, vp]
    L.lfx_place_db_size.argtypes = [vp, C.POINTER(u32)]
    L.lfx_place_db_download.argtypes = [vp, vp, u32, u32, vp, vp]
    L.lfx_place_db_query.argtypes = [vp, vp, vp, u32, u32, u32, u32, C.POINTER(PlaceMatch), vp]
    pseg = C.POINTER(SegmentConfig)
    L.lfx_segment_default_config.argtypes = [pseg]
    L.lfx_segment_default_config.restype = None
    L.lfx_segment_tables.argtypes = [pseg, pd, pd, pd]
    L.lfx_segment_batch.argtypes = [vp, pseg, u32, vp, vp, vp, vp]
    L.lfx_pack_features_segmented.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp, C.c_size_t, vp]
    L.lfx_pack_xyz.argtypes = [vp, vp, vp, vp, C.c_size_t, vp]
    L.lfx_pack_xyz12.argtypes = [vp, vp, vp, vp, C.c_size_t, vp]
    L.lfx_pack_colored.argtypes = [vp, vp, vp, C.c_size_t, vp]
    L.lfx_pack_features.argtypes = [vp, vp, vp, vp, C.c_size_t, vp]
    L.lfx_download_scan.argtypes = [vp, u32, vp, C.POINTER(ScanResult)]
    L.lfx_stage_ring.argtypes = [vp, C.POINTER(Params), u32, u32] + [vp] * 10
    L.lfx_stage_convolution1d.argtypes = [vp, vp, u32, vp, u32, vp]
    L.lfx_stage_ring_projection.argtypes = [vp, vp, C.c_size_t, vp, C.POINTER(u32), vp, vp]
    L.lfx_label_to_color.argtypes = [C.c_uint8, C.POINTER(C.c_uint8)]
    L.lfx_color_points_by_label.argtypes = [vp, vp, C.c_size_t, vp, vp]
    L.lfx_set_profiling.argtypes = [vp, i32]
    L.lfx_set_profiling_interval.argtypes = [vp, C.c_uint32]
    ppg = C.POINTER(PoseGraphConfig)
    L.lfx_pose_graph_default_config.argtypes = [ppg]
    L.lfx_pose_graph_default_config.restype = None
    L.lfx_pose_graph_create.argtypes = [vp, ppg, C.POINTER(vp)]
    L.lfx_pose_graph_destroy.argtypes = [vp]
    L.lfx_pose_graph_destroy.restype = None
    L.lfx_pose_graph_info.argtypes = [vp, C.POINTER(PoseGraphInfo)]
    L.lfx_pose_graph_add_nodes.argtypes = [vp, vp, vp, u32, C.POINTER(u32), vp]
    L.lfx_pose_graph_set_fixed.argtypes = [vp, vp, u32, i32, vp]
    L.lfx_pose_graph_add_edges.argtypes = [vp, vp, vp, u32, vp]
    L.lfx_pose_graph_optimize.argtypes = [vp, vp, C.POINTER(PoseGraphResult), vp]
    L.lfx_pose_graph_poses.argtypes = [vp, vp, u32, u32, vp, vp]
    L.lfx_pose_graph_set_poses.argtypes = [vp, vp, u32, u32, vp, vp]
    L.lfx_pose_graph_view.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(u32), vp]
    L.lfx_pose_graph_edge_chi2.argtypes = [vp, vp, u32, u32, vp, vp, vp]
    L.lfx_pose_graph_edge_information.argtypes = [vp, vp, vp]
    L.lfx_pose_graph_reserve_priors.argtypes = [vp, vp, u32]
    L.lfx_pose_graph_add_priors.argtypes = [vp, vp, vp, u32, vp]
    L.lfx_pose_graph_release_first.argtypes = [vp, vp, i32, vp]
    L.lfx_pose_graph_prior_chi2.argtypes = [vp, vp, u32, u32, vp, vp, vp]
    L.lfx_pose_graph_prior_info.argtypes = [vp, C.POINTER(PoseGraphPriorInfo)]
    L.lfx_pose_graph_reserve_marginals.argtypes = [vp, vp]
    L.lfx_pose_graph_marginals.argtypes = [vp, vp, u32, u32, vp, C.POINTER(i32), vp]
    L.lfx_pose_graph_joint_covariances.argtypes = [vp, vp, vp, u32, vp, C.POINTER(i32), vp]
    L.lfx_pose_graph_relative_covariance.argtypes = [vp, vp, vp, vp]
    pkf, pkc = C.POINTER(KeyframesConfig), C.POINTER(KeyframesClouds)
    L.lfx_keyframes_default_config.argtypes = [pkf]
    L.lfx_keyframes_default_config.restype = None
    L.lfx_keyframes_create.argtypes = [vp, pkf, C.POINTER(vp)]
    L.lfx_keyframes_destroy.argtypes = [vp]
    L.lfx_keyframes_destroy.restype = None
    L.lfx_keyframes_info.argtypes = [vp, C.POINTER(KeyframesInfo)]
    L.lfx_keyframes_view.argtypes = [vp, vp, C.POINTER(KeyframesStoreView), vp]
    L.lfx_keyframes_add.argtypes = [vp, vp, pkc, pkc, u32, vp, C.POINTER(u32), vp]
    L.lfx_keyframes_add_host.argtypes = [vp, vp, vp, u32, vp, u32, vp, C.POINTER(u32), vp]
    L.lfx_keyframes_set_poses.argtypes = [vp, vp, u32, u32, vp, vp]
    L.lfx_keyframes_poses.argtypes = [vp, vp, u32, u32, vp, vp]
    L.lfx_keyframes_follow.argtypes = [vp, vp, vp, u32, u32, vp]
    L.lfx_keyframes_build.argtypes = [vp, vp, i32, u32, u32, vp, u64, p64, vp]
    L.lfx_keyframes_submap.argtypes = [vp, vp, i32, vp, C.c_double, u32, u32, vp, u64, C.POINTER(KeyframesSubmapResult), vp]
    L.lfx_keyframes_save.argtypes = [vp, vp, C.c_char_p, C.POINTER(i32), vp]
    L.lfx_keyframes_build_masked.argtypes = [vp, vp, i32, u32, u32, vp, vp, u64, vp, p64, vp]
    L.lfx_keyframes_reserve_flags.argtypes = [vp, vp, vp]
    L.lfx_keyframes_flags.argtypes = [vp, vp, C.POINTER(vp), vp]
    L.lfx_keyframes_set_flags.argtypes = [vp, vp, i32, u32, u32, vp, vp]
    L.lfx_keyframes_clear_flags.argtypes = [vp, vp, i32, u32, u32, vp]
    L.lfx_keyframes_flags_info.argtypes = [vp, vp, C.POINTER(KeyframesFlagsInfo), vp]
    L.lfx_keyframes_submap_masked.argtypes = L.lfx_keyframes_submap.argtypes
    L.lfx_keyframes_save_masked.argtypes = L.lfx_keyframes_save.argtypes
    pvc = C.POINTER(VisibilityConfig)
    L.lfx_visibility_default_config.argtypes = [pvc]
    L.lfx_visibility_default_config.restype = None
    L.lfx_visibility_tables.argtypes = [pvc, vp, vp, vp]
    L.lfx_visibility_create.argtypes = [vp, pvc, u32, u32, C.POINTER(vp)]
    L.lfx_visibility_destroy.argtypes = [vp]
    L.lfx_visibility_destroy.restype = None
    L.lfx_visibility_info.argtypes = [vp, C.POINTER(VisibilityInfo)]
    L.lfx_visibility_run.argtypes = [vp, vp, vp, u32, u32, C.POINTER(vp), C.POINTER(vp), C.POINTER(VisibilityResult), vp]
    pvf = C.POINTER(VoxelFilterConfig)
    L.lfx_voxel_filter_default_config.argtypes = [pvf]
    L.lfx_voxel_filter_default_config.restype = None
    L.lfx_voxel_filter_create.argtypes = [vp, pvf, C.POINTER(vp)]
    L.lfx_voxel_filter_destroy.argtypes = [vp]
    L.lfx_voxel_filter_destroy.restype = None
    L.lfx_voxel_filter_info.argtypes = [vp, C.POINTER(VoxelFilterInfo)]
    L.lfx_voxel_filter_reset.argtypes = [vp, vp, C.c_float, vp]
    L.lfx_voxel_filter_add.argtypes = [vp, vp, vp, u64, vp]
    L.lfx_voxel_filter_add_host.argtypes = [vp, vp, vp, u64, vp]
    L.lfx_voxel_filter_emit.argtypes = [vp, vp, u32, vp, u64, vp, C.POINTER(VoxelFilterResult), vp]
    L.lfx_voxel_filter_add_keyframes.argtypes = [vp, vp, vp, i32, u32, u32, i32, vp]
    L.lfx_keyframes_save_filtered.argtypes = [vp, vp, vp, C.POINTER(C.c_float), u32, i32, C.c_char_p, C.POINTER(i32), vp]
    poc, poe = C.POINTER(OccupancyConfig), C.POINTER(OccupancyEmitConfig)
    L.lfx_occupancy_default_config.argtypes = [poc]
    L.lfx_occupancy_default_config.restype = None
    L.lfx_occupancy_tables.argtypes = [poc, vp, vp]
    L.lfx_occupancy_emit_default_config.argtypes = [poe]
    L.lfx_occupancy_emit_default_config.restype = None
    L.lfx_occupancy_emit_table.argtypes = [poe, vp]
    L.lfx_occupancy_create.argtypes = [vp, poc, C.POINTER(vp)]
    L.lfx_occupancy_destroy.argtypes = [vp]
    L.lfx_occupancy_destroy.restype = None
    L.lfx_occupancy_info.argtypes = [vp, C.POINTER(OccupancyInfo)]
    L.lfx_occupancy_view.argtypes = [vp, vp, C.POINTER(OccupancyView), vp]
    L.lfx_occupancy_add_batch.argtypes = [vp, vp, u32, vp, vp, vp, u32, u32, C.POINTER(u32), vp]
    L.lfx_occupancy_set_poses.argtypes = [vp, vp, u32, u32, vp, vp]
    L.lfx_occupancy_poses.argtypes = [vp, vp, u32, u32, vp, vp]
    L.lfx_occupancy_follow.argtypes = [vp, vp, vp, u32, u32, vp]
    L.lfx_occupancy_truncate.argtypes = [vp, vp, u32, vp]
    L.lfx_occupancy_clear.argtypes = [vp, vp, vp]
    L.lfx_occupancy_render.argtypes = [vp, vp, u32, u32, vp]
    L.lfx_occupancy_counters.argtypes = [vp, vp, C.POINTER(OccupancyCounters), vp]
    L.lfx_occupancy_emit.argtypes = [vp, vp, poe, vp, vp]
    L.lfx_occupancy_write_map.argtypes = [C.c_char_p, vp, u32, u32, C.c_float, C.c_double, C.c_double, i32, i32]
    L.lfx_occupancy_save.argtypes = [vp, vp, poe, C.c_char_p, i32, i32, vp]
    pdc, pdk = C.POINTER(DistanceConfig), C.POINTER(DistanceCostConfig)
    L.lfx_distance_default_config.argtypes = [pdc]
    L.lfx_distance_default_config.restype = None
    L.lfx_distance_cost_default_config.argtypes = [pdk]
    L.lfx_distance_cost_default_config.restype = None
    L.lfx_distance_cost_table_size.argtypes = [pdk, C.c_float, C.POINTER(u32)]
    L.lfx_distance_cost_table.argtypes = [pdk, C.c_float, vp, u32]
    L.lfx_distance_create.argtypes = [vp, u32, u32, C.POINTER(vp)]
    L.lfx_distance_destroy.argtypes = [vp]
    L.lfx_distance_destroy.restype = None
    L.lfx_distance_info.argtypes = [vp, C.POINTER(DistanceInfo)]
    L.lfx_distance_from_grid.argtypes = [vp, vp, vp, pdc, vp]
    L.lfx_distance_from_occupancy.argtypes = [vp, vp, vp, poe, pdc, vp]
    L.lfx_distance_view.argtypes = [vp, vp, C.POINTER(DistanceView), vp]
    L.lfx_distance_metres.argtypes = [vp, vp, C.c_float, vp, vp]
    L.lfx_distance_costmap.argtypes = [vp, vp, pdk, C.c_float, vp, vp]
    L.lfx_distance_stats.argtypes = [vp, vp, C.POINTER(DistanceStats), vp]
    pgc, pgt, pgs = C.POINTER(GridMatchConfig), C.POINTER(GridMatchTableConfig), C.POINTER(GridMatchSearchConfig)
    for name, ptr in (("lfx_grid_match_default_config", pgc), ("lfx_grid_match_table_default_config", pgt), ("lfx_grid_match_search_default_config", pgs)):
        getattr(L, name).argtypes = [ptr]
        getattr(L, name).restype = None
    L.lfx_grid_match_table_size.argtypes = [pgt, C.c_float, C.POINTER(u32)]
    L.lfx_grid_match_table.argtypes = [pgt, C.c_float, vp, u32]
    L.lfx_grid_match_search_size.argtypes = [pgs, C.POINTER(u32)]
    L.lfx_grid_match_rotations.argtypes = [C.c_double, u32, C.c_double, vp]
    L.lfx_grid_match_candidate.argtypes = [pgs, C.c_float, vp, u32, vp]
    L.lfx_grid_match_pose3.argtypes = [vp, vp, C.c_double, vp]
    L.lfx_grid_match_create.argtypes = [vp, pgc, C.POINTER(vp)]
    L.lfx_grid_match_destroy.argtypes = [vp]
    L.lfx_grid_match_destroy.restype = None
    L.lfx_grid_match_info.argtypes = [vp, C.POINTER(GridMatchInfo)]
    L.lfx_grid_match_view.argtypes = [vp, vp, C.POINTER(GridMatchView), vp]
    L.lfx_grid_match_set_field.argtypes = [vp, vp, vp, vp, u32, vp]
    L.lfx_grid_match_set_scans.argtypes = [vp, vp, vp, u32, u32, vp, vp]
    L.lfx_grid_match_set_scans_occupancy.argtypes = [vp, vp, vp, u32, u32, i32, vp]
    L.lfx_grid_match_score.argtypes = [vp, vp, u32, vp, u32, vp, vp, vp]
    L.lfx_grid_match_search.argtypes = [vp, vp, u32, u32, vp, pgs, vp, vp, vp, vp]
    L.lfx_place_db_query_gated.argtypes = [vp, vp, vp, u32, C.POINTER(PlaceGate), vp, C.c_double, u32, C.POINTER(PlaceMatch), C.POINTER(u32), vp]
    plc = C.POINTER(LoopCloserConfig)
    L.lfx_loop_closer_default_config.argtypes = [plc]
    L.lfx_loop_closer_default_config.restype = None
    L.lfx_loop_closer_create.argtypes = [vp, plc, vp, vp, vp, C.POINTER(vp)]
    L.lfx_loop_closer_destroy.argtypes = [vp]
    L.lfx_loop_closer_destroy.restype = None
    L.lfx_loop_closer_info.argtypes = [vp, C.POINTER(LoopCloserInfo)]
    L.lfx_loop_closer_set_masked.argtypes = [vp, i32]
    L.lfx_loop_closer_get_masked.argtypes = [vp, C.POINTER(i32)]
    L.lfx_loop_closer_detect.argtypes = [vp, vp, u32, u32, C.POINTER(PlaceMatch), C.POINTER(u32), vp]
    L.lfx_loop_closer_verify.argtypes = [vp, vp, u32, C.POINTER(PlaceMatch), C.POINTER(LoopClosure), vp]
    L.lfx_loop_closer_update.argtypes = [vp, vp, u32, u32, C.POINTER(LoopClosure), C.POINTER(LoopCloserResult), vp]
    L.lfx_kernel_times.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.lfx_kernel_name.argtypes = [i32]
    L.lfx_kernel_name.restype = C.c_char_p
    L.lfx_box_calibration.argtypes = [vp, C.c_size_t, vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    _libs[path] = L
    return L


def check(ctx, rc, lib=None):
    if rc != 0:
        raise LfxError(rc, ((lib or load()).lfx_last_error(ctx) or b"").decode())
