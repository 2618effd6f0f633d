"""MI355X-native lidar feature extraction (the extraction/ hot path of tier4/lidar_feature_extraction).

HIP kernels + C ABI live in csrc/ (built to _lib/liblfx.so); `FeatureExtraction` is the host-side
mirror of the reference node's operator.  Importing this package does not need a GPU; creating a
`FeatureExtraction` does, and raises if the library or the device is missing (no CPU fallback).
"""
from .extraction import FeatureExtraction, HyperParameters, Odometry, ScanFeatures, LABEL_NAMES, RING_STATUS_NAMES, layout_from_fields  # noqa: F401
from .extraction import RollingMap  # noqa: F401
from .extraction import Mapper, ScanMap, read_pcd, write_pcd, pose_diff, covariance_ros  # noqa: F401
from .extraction import time_field_from_fields, motion_between, motion_twist, motion_scale  # noqa: F401
from .extraction import trajectory_segments, trajectory_from_gyro  # noqa: F401
from .extraction import PlaceDb, scan_context_config, scan_context_tables  # noqa: F401
from .extraction import segment_config, segment_tables  # noqa: F401
from .extraction import PoseGraph, pose_graph_config, pose_graph_edges, pose_graph_priors, edge_information, relative_covariance  # noqa: F401
from .extraction import Keyframes  # noqa: F401
from .extraction import LoopCloser, loop_closer_config  # noqa: F401
from .extraction import Visibility, visibility_config, visibility_tables  # noqa: F401
from .extraction import VoxelFilter  # noqa: F401
from .extraction import OccupancyGrid, occupancy_config, occupancy_tables, occupancy_emit_config, occupancy_emit_table, write_occupancy_map  # noqa: F401
from .extraction import DistanceField, distance_config, distance_cost_config, distance_cost_table  # noqa: F401
from .extraction import GridMatcher, grid_match_config, grid_match_table_config, grid_match_search_config, grid_match_table  # noqa: F401
from .extraction import grid_match_search_size, grid_match_rotations, grid_match_candidate, grid_match_pose3  # noqa: F401
from .synth import POINT_DTYPE, SENSORS, make_scan, make_batch, make_sequence, make_sweep, make_sweep_trajectory, concat  # noqa: F401
