/*
 * lfx.h -- C ABI of the MI355X-native lidar feature extraction hot path.
 *
 * The reference (tier4/lidar_feature_extraction) has no plugin/FFI boundary: its per-scan
 * extraction is the C++ body of FeatureExtraction::Callback,
 *   /root/reference/extraction/app/feature_extraction.cpp:114-157
 * between GetPointCloud<PointXYZIR> (:94) and ToPointXYZ/ToRosMsg (:161-166).  This header is
 * the drop-in boundary for exactly those lines: PointXYZIR points in (32-byte AoS,
 * lib/include/lidar_feature_library/point_type.hpp:62-86), edge + surface clouds, per-point
 * labels and curvature out.  Plain pointers and sizes only; no C++ or torch types.
 * INTEGRATION.md shows the replacement of lines 114-157 that binds these entry points.
 *
 * Threading: a context is NOT thread-safe; use one context per GPU / per calling thread
 * (the reference's caller is a single-threaded executor, feature_extraction.cpp:185).
 * Every function returns LFX_OK (0) or a negative lfx_error; lfx_last_error() gives text.
 * No exception crosses this boundary: the reference's per-ring std::invalid_argument
 * (feature_extraction.cpp:154-156: warn, ring contributes nothing) becomes ring_status[].
 */
#ifndef LFX_H_
#define LFX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LFX_VERSION 1
#define LFX_MAX_PADDING 63          /* convolution_padding: up to 15 the window kernels (the fast routes); 16 .. 63 every ring takes the
                                    * workgroup-per-ring kernel, whose labelling then walks the positions in reach (slow, same results) */
#define LFX_MAX_RING_ID 65535       /* a ring id is the uint16 of PointXYZIR (point_type.hpp:62-86) */
#define LFX_MAX_RINGS 256           /* distinct ring ids a context takes (every spinning lidar fielded today has fewer) */
#define LFX_MAX_RING_POINTS 4608    /* the longest ring the LDS-resident kernels take (25 B per point in one workgroup's LDS; 6 blocks
                                     * of the unit kernels' long form), and the ring capacity of a context that names none */
#define LFX_MAX_LONG_RING_POINTS 262144  /* the largest max_points_per_ring (2^18).  A context above LFX_MAX_RING_POINTS takes
                                     * rings of up to its capacity, the longer ones in a kernel whose workspace is in HBM */

/* The nine node parameters: extraction/include/lidar_feature_extraction/hyper_parameter.hpp:32-65
 * (same names, same units; the neighbour threshold is in DEGREES, converted as
 * lib/include/lidar_feature_library/degree_to_radian.hpp:34-37 does). */
typedef struct lfx_params {
  int32_t padding;                        /* convolution_padding            default 5    */
  double neighbor_degree_threshold;       /*                                default 2.0  */
  double distance_diff_threshold;         /*                                default 0.3  */
  double parallel_beam_min_range_ratio;   /*                                default 0.02 */
  double edge_threshold;                  /*                                default 0.05 */
  double surface_threshold;               /*                                default 0.05 */
  double min_range;                       /*                                default 0.1  */
  double max_range;                       /*                                default 100  */
  int32_t n_blocks;                       /*                                default 6    */
} lfx_params;

/* sensor_msgs/msg/PointField datatype codes (the upstream converter's table,
 * point_type_converter/convert.py:41-53). */
enum lfx_field_type {
  LFX_FIELD_INT8 = 1, LFX_FIELD_UINT8 = 2, LFX_FIELD_INT16 = 3, LFX_FIELD_UINT16 = 4, LFX_FIELD_INT32 = 5,
  LFX_FIELD_UINT32 = 6, LFX_FIELD_FLOAT32 = 7, LFX_FIELD_FLOAT64 = 8
};

/* Where x, y, z (f32) and ring sit inside one point record, as a PointCloud2 describes it.
 * PointXYZIR is {32, 0, 4, 8, 20, LFX_FIELD_UINT16, 0} (point_type.hpp:62-86; convert.py:134-145 of
 * point_type_converter).  ring_datatype: any integer PointField type (0 = UINT16; an Ouster driver
 * publishes UINT8, test_convert.py:42-60); big_endian: the message's is_bigendian flag.  With these
 * the library reads a driver's cloud directly -- the repack the upstream converter node does on the
 * CPU (convert.py:183-212) is folded into the bucketing kernel's loads. */
typedef struct lfx_layout {
  uint32_t point_step, off_x, off_y, off_z, off_ring;
  uint32_t ring_datatype, big_endian;
} lfx_layout;

/* One entry of PointCloud2.fields */
typedef struct lfx_point_field {
  const char *name;
  uint32_t offset;
  uint8_t datatype;               /* lfx_field_type */
  uint32_t count;
} lfx_point_field;

typedef struct lfx_config {
  uint32_t struct_size;           /* sizeof(lfx_config) as the CALLER was compiled with it: fields beyond it (added to the end
                                   * of this struct by a later header) read as zero, so that a caller built against an
                                   * older header keeps working.  0 is refused (an uninitialised struct).               */
  uint32_t max_points_per_scan;   /* capacity of one scan                                   */
  uint32_t max_batch;             /* scans per lfx_extract_batch* call                      */
  uint32_t max_points_per_ring;   /* 0 = LFX_MAX_RING_POINTS; at most LFX_MAX_LONG_RING_POINTS and max_points_per_scan;
                                   * rounded up to a multiple of 64 (cap).  The sensor's real column count here lets the
                                   * ring kernel run its smallest (fastest) variant.  Above LFX_MAX_RING_POINTS (long rings:
                                   * line-based sensors, slow spinning ones) the ring-major arrays take
                                   * max_batch x max_rings x cap x 45 B (37 B without LFX_OUT_CURVATURE) -- set max_rings:
                                   * 0 reserves 256 rings of cap points each -- plus up to 512 MB of workspace for the
                                   * long-ring kernel; the context declines the holes form (grids with (0, 0, 0) records
                                   * are bucketed) */
  uint32_t max_rings;             /* ring ids are 0 .. max_rings-1 (a sensor's ring count); 0 = 256 */
  uint32_t drop_zero_points;      /* 1: points with x = y = z = 0 are not part of the scan -- the filter the
                                   * upstream converter applies (point_type_converter/convert.py:162-163,192) */
  lfx_layout layout;              /* all-zero = PointXYZIR                                  */
  uint32_t outputs;               /* LFX_OUT_* mask: what lfx_extract / lfx_extract_batch bring back to the host.
                                   * 0 = LFX_OUT_ALL.  The edge / surface clouds (with their index lists) and the ring
                                   * table always come back; labels, curvature and sorted_index are per-point arrays
                                   * (13 bytes per point over PCIe) that the node itself does not consume
                                   * (feature_extraction.cpp:161-170 publishes the two clouds; labels only feed the
                                   * colored_scan debug cloud): a caller that does not need them leaves them out.
                                   * Without LFX_OUT_CURVATURE the per-point curvature is not PRODUCED either (the
                                   * device view's curvature_sorted is NULL; the feature points still carry theirs as
                                   * intensity): 8 of the 9 bytes the kernels write per point, +5 % scans/s          */
  uint32_t stream_hint;           /* LFX_STREAM_*: what the caller knows about the order its driver publishes in.  The
                                   * library finds the route for a stream from what the first batches report (nothing to
                                   * configure); a hint only spares the FIRST batch of a stream the slower route         */
  const uint16_t *ring_ids;       /* the sensor's ring ids where they are not 0 .. max_rings-1 (the reference buckets by
                                   * whatever uint16 a point carries, ring.hpp:114-125): n_ring_ids distinct ids, at most
                                   * LFX_MAX_RINGS of them; results list rings by id ascending.  NULL: ids 0 .. max_rings-1 --
                                   * and the host entry points (lfx_extract*) look the ids of a scan up themselves when a
                                   * point carries another one (lfx_set_ring_ids does the same for the device path)       */
  uint32_t n_ring_ids;
} lfx_config;

#define LFX_STREAM_UNKNOWN 0u      /* start on the organised route, adapt                                               */
#define LFX_STREAM_TURNED_RINGS 1u /* a grid whose rings arrive rotated / reversed (scans not cut at -pi, a clockwise
                                    * sensor): find the rings' transforms from the first batch on                        */
#define LFX_STREAM_NO_GRID 2u      /* records missing or in arbitrary order: the bucketing route from the first batch on */
#define LFX_STREAM_GRID_WITH_HOLES 3u /* a grid whose invalid returns are (0, 0, 0) records, with drop_zero_points set (what the
                                    * reference's converter filters, convert.py:162-163,192): count the valid returns per ring
                                    * first and read the grid in place, from the first batch on.  Means nothing (and is
                                    * dropped) without drop_zero_points or on a context with long rings                  */

#define LFX_OUT_FEATURES 1u        /* always on */
#define LFX_OUT_LABELS 2u
#define LFX_OUT_CURVATURE 4u
#define LFX_OUT_SORTED_INDEX 8u
#define LFX_OUT_ALL 15u

/* PointLabel values: extraction/include/lidar_feature_extraction/point_label.hpp:32-42 */
enum lfx_label {
  LFX_LABEL_DEFAULT = 0, LFX_LABEL_EDGE = 1, LFX_LABEL_EDGE_NEIGHBOR = 2, LFX_LABEL_SURFACE = 3,
  LFX_LABEL_SURFACE_NEIGHBOR = 4, LFX_LABEL_OUT_OF_RANGE = 5, LFX_LABEL_OCCLUDED = 6,
  LFX_LABEL_PARALLEL_BEAM = 7
};

/* Per-ring outcome.  Non-zero = the ring contributes no label, curvature or feature point,
 * exactly as a ring the reference removes (RemoveSparseRings, ring.cpp:46-59) or abandons on
 * std::invalid_argument (feature_extraction.cpp:154-156). */
enum lfx_ring_status {
  LFX_RING_OK = 0,
  LFX_RING_SPARSE = 1,            /* N < padding+1                 ring.cpp:46-59             */
  LFX_RING_TOO_FEW_CONV = 2,      /* N < 2*padding+1               convolution.cpp:39-43      */
  LFX_RING_TOO_FEW_BLOCKS = 3,    /* N - 2*padding < n_blocks      index_range.cpp:35-40      */
  LFX_RING_BLOCK_TOO_SMALL = 4,   /* a block holds < 2 points      neighbor.hpp:71-75         */
  LFX_RING_ZERO_NORM_PAIR = 5,    /* adjacent points both (0,0)    math.cpp:40-42             */
  LFX_RING_TOO_LARGE = 7          /* N > max_points_per_ring (no reference counterpart)       */
};

enum lfx_error {
  LFX_OK = 0,
  LFX_ERR_INVALID_ARGUMENT = -1,
  LFX_ERR_NO_DEVICE = -2,         /* no HIP device / kernel image: the product has NO CPU fallback */
  LFX_ERR_HIP = -3,
  LFX_ERR_CAPACITY = -4,          /* more points / scans than the context was created for     */
  LFX_ERR_RING_ID = -5,           /* a point carries a ring id the context does not know (lfx_config.ring_ids,
                                   * lfx_set_ring_ids), or a scan more than LFX_MAX_RINGS distinct ones */
  LFX_ERR_OUT_OF_MEMORY = -6,
  LFX_ERR_NO_RING_FIELD = -7,     /* the cloud has no "ring" field: RingIsAvailable (ring.cpp:36-44) is false and the
                                   * node shuts down (feature_extraction.cpp:103-108)            */
  LFX_ERR_UNSUPPORTED_FIELD = -8, /* x / y / z missing or not FLOAT32, ring not an integer, field outside point_step */
  LFX_ERR_FILE = -9,              /* a file cannot be opened, read or written, or it is not a PCD file lfx_pcd_read takes */
  LFX_ERR_NO_TIME_FIELD = -10     /* the cloud has no per-point time field (lfx_time_field_from_fields) */
};

typedef struct lfx_ctx lfx_ctx;

/* One scan's results in host memory (pinned, owned by the context, valid until its next call). */
typedef struct lfx_scan_result {
  uint32_t n_points;
  const uint8_t *labels;          /* [n_points] lfx_label, addressed by ORIGINAL point index; NULL unless LFX_OUT_LABELS  */
  const double *curvature;        /* [n_points] f64, original index (curvature.cpp:44-50); NULL unless LFX_OUT_CURVATURE  */
  const uint32_t *sorted_index;   /* [n_sorted] rings ascending, angle ascending inside a ring (ring.hpp:141-147); NULL unless LFX_OUT_SORTED_INDEX */
  uint32_t n_sorted;              /* = n_points, less the points drop_zero_points removed                  */
  uint32_t n_rings;
  const uint16_t *ring_id;        /* [n_rings] ascending                                        */
  const uint32_t *ring_count;     /* [n_rings] points of the ring                               */
  const uint32_t *ring_offset;    /* [n_rings] start of the ring inside sorted_index            */
  const uint8_t *ring_status;     /* [n_rings] lfx_ring_status                                  */
  uint32_t n_edge;
  const float *edge_points;       /* [n_edge][4] x, y, z, (float)curvature  (label.hpp:166-179) */
  const uint32_t *edge_index;     /* [n_edge] original point index; ring asc, angle asc         */
  uint32_t n_surface;
  const float *surface_points;    /* [n_surface][4]                                             */
  const uint32_t *surface_index;
} lfx_scan_result;

/* Device-resident results of the last lfx_extract_batch_device call (device pointers owned by
 * the context).  Per-point outputs are RING-MAJOR with a fixed capacity per ring slot (the ring id; with lfx_config.ring_ids /
 * lfx_set_ring_ids the id's rank among the sensor's ids): ring r of
 * scan s owns positions [(s * max_rings + r) * ring_capacity, + ring_count[s][r]) of labels_sorted,
 * curvature_sorted and sorted_index, angle ascending.  The feature clouds are dense: scan s owns the
 * first n_edge / n_surface records from scan_begin[s] (scan_info[s][2], [3]).
 * scan_info[s][1] carries error bits (1: a ring id the context does not know, 4: bucketing timed out -- lfx_batch_status turns
 * them into a return code) and the route the scan took: (bits & LFX_SCAN_ROUTE_MASK) == LFX_SCAN_ORGANISED means the
 * scan arrived column-major with ring == index mod max_rings and was read in place: position k of ring r IS input
 * point k * max_rings + r and sorted_index holds nothing for that scan.  Any other value: sorted_index holds every ring
 * position's original index -- a bucketed scan, or (bit LFX_SCAN_GRID_WITH_HOLES, without LFX_SCAN_ORGANISED) a grid with
 * (0, 0, 0) records that the zero filter dropped, read in place (lfx_scan_routes: 3). */
#define LFX_SCAN_ROUTE_MASK 0x300u
#define LFX_SCAN_ORGANISED 0x100u
#define LFX_SCAN_GRID_WITH_HOLES 0x800u
typedef struct lfx_device_view {
  uint32_t batch;
  uint32_t max_rings;             /* ring ids the layout has room for                            */
  uint32_t ring_capacity;         /* positions per ring (max_points_per_ring rounded up to 64)   */
  const uint32_t *scan_begin;     /* device [batch+1] (in points)                                */
  const uint8_t *labels_sorted;   /* device: label of ring position k                            */
  const double *curvature_sorted; /* device; NULL in a context created without LFX_OUT_CURVATURE */
  const uint32_t *sorted_index;   /* device: original index (within its scan) of ring position k */
  const uint32_t *scan_info;      /* device [batch][4]: occupied rings, error bits, n_edge, n_surface */
  const uint32_t *ring_count;     /* device [batch][256] by ring slot                            */
  const uint8_t *ring_status;     /* device [batch][256] by ring slot (valid where ring_count > 0) */
  const float *edge_points;       /* device [total][4]                                           */
  const uint32_t *edge_index;
  const float *surface_points;
  const uint32_t *surface_index;
} lfx_device_view;

/* --- parameters ------------------------------------------------------------------------ */
void lfx_default_params(lfx_params *p);   /* code defaults, hyper_parameter.hpp:35-43 */
void lfx_launch_params(lfx_params *p);    /* lidar_feature_launch/config/lidar_feature_extraction.param.yaml:3-10 */

/* --- context --------------------------------------------------------------------------- */
/* Replaces the node's construction of HyperParameters / EdgeLabel / SurfaceLabel
 * (feature_extraction.cpp:68-72).  Fails with LFX_ERR_NO_DEVICE when no MI355X is present. */
int lfx_create(lfx_ctx **ctx, int device_id, const lfx_params *params, const lfx_config *config);
void lfx_destroy(lfx_ctx *ctx);
const char *lfx_last_error(const lfx_ctx *ctx);   /* ctx may be NULL: error of the last failed lfx_create */
const char *lfx_status_string(int ring_status);
/* The text the reference's exception carries when it abandons a ring of n_points points for `ring_status` -- what the
 * node logs with RCLCPP_WARN(e.what()), feature_extraction.cpp:154-156: convolution.cpp:40-41, index_range.cpp:36-38,
 * neighbor.hpp:72-73, math.cpp:41.  Empty for LFX_RING_OK, LFX_RING_SPARSE (RemoveSparseRings drops the ring silently,
 * ring.cpp:46-59) and LFX_RING_TOO_LARGE (no counterpart).  Returns the length written (snprintf semantics). */
int lfx_ring_message(int ring_status, uint32_t n_points, const lfx_params *params, char *buf, size_t len);
/* Optional log callback: where the node logs, the library calls back.  For every ring a host-API call (lfx_extract,
 * lfx_extract_batch, lfx_extract_wait) finds abandoned on std::invalid_argument it calls `cb(LFX_LOG_WARN, text, user)` with
 * the text of lfx_ring_message -- the node's RCLCPP_WARN(e.what()), feature_extraction.cpp:154-156, once per ring as there
 * (a ring RemoveSparseRings drops makes no sound, ring.cpp:46-59; LFX_RING_TOO_LARGE, which has no counterpart, is reported
 * with the library's own text).  Called on the caller's thread, inside the call that brought the results; cb = NULL
 * switches it off (the default).  Nothing is ever printed by the library itself. */
#define LFX_LOG_WARN 1
typedef void (*lfx_log_fn)(int level, const char *message, void *user);
int lfx_set_log_callback(lfx_ctx *ctx, lfx_log_fn cb, void *user);
/* RangeMessage* of range_message.hpp:37-83, the texts of the reference's bounds errors ("i (which is 39) >= max (which
 * is 30)"): kind 0 LargerThanOrEqualTo, 1 SmallerThanOrEqualTo, 2 LargerThan, 3 SmallerThan.  Returns the length, -1
 * for an unknown kind. */
int lfx_range_message(int kind, const char *value_name, const char *range_name, long long value, long long range,
                      char *buf, size_t len);

/* --- the operator: feature_extraction.cpp:114-157 ---------------------------------------- */
/* Host points in, host results out (synchronous; H2D + kernels + D2H). */
int lfx_extract(lfx_ctx *ctx, const void *points, size_t n_points, lfx_scan_result *out);
/* The same in two halves, for a caller that keeps the next scan coming while this one is on the device (the node's
 * callback, feature_extraction.cpp:92-171, called by a spinning executor, :185): lfx_extract_submit queues the upload of
 * `points` (on a stream of its own, so that it runs beside the kernels of the scan before), the kernels and the download,
 * and returns at once with a ticket; lfx_extract_wait(ticket) waits for that scan alone and fills `out`.  Two scans may
 * be in flight: a third lfx_extract_submit before the first lfx_extract_wait fails with LFX_ERR_INVALID_ARGUMENT.
 * Tickets are waited for in the order they were issued.  `points`: pageable memory is copied at once and may be reused
 * when lfx_extract_submit returns; pinned memory (lfx_host_alloc) is read by DMA and must stay untouched until that
 * ticket's lfx_extract_wait returns.  `out` and what it points to stay valid until the SECOND lfx_extract_submit after
 * this lfx_extract_wait (each of the two slots has a result block of its own).  Not to be mixed with lfx_extract /
 * lfx_extract_batch / lfx_extract_batch_device while a ticket is outstanding (LFX_ERR_INVALID_ARGUMENT). */
int lfx_extract_submit(lfx_ctx *ctx, const void *points, size_t n_points, uint64_t *ticket);
int lfx_extract_wait(lfx_ctx *ctx, uint64_t ticket, lfx_scan_result *out);
int lfx_extract_batch(lfx_ctx *ctx, const void *const *points, const size_t *n_points, uint32_t batch,
                      lfx_scan_result *out /* [batch] */);

/* Device points in, results stay on the device (asynchronous on `stream`, a hipStream_t or NULL).
 * d_points: the scans' point records back to back; n_points: host array [batch]. */
int lfx_extract_batch_device(lfx_ctx *ctx, const void *d_points, const uint32_t *n_points, uint32_t batch,
                             void *stream);
int lfx_device_results(const lfx_ctx *ctx, lfx_device_view *view);
/* Input records of the last batch the context ran, whichever entry point ran it (lfx_extract, lfx_extract_submit,
 * lfx_extract_batch, lfx_extract_batch_device): the view's scan_begin[batch] as the device holds it, from the host's copy --
 * no device work, no wait.  What a caller sizes per-record outputs by (lfx_segment_batch).  0 before the first batch. */
int lfx_batch_points(const lfx_ctx *ctx, uint64_t *n_points);
/* What lfx_extract reports through its return code, for callers of the device-resident path: waits for `stream`,
 * reads the last batch's scan_info and returns LFX_ERR_RING_ID / LFX_ERR_HIP if any scan carries an error bit
 * (the clouds of such a scan are not to be used), else LFX_OK.  first_bad (may be NULL): index of the first such scan. */
int lfx_batch_status(lfx_ctx *ctx, void *stream, uint32_t *first_bad);
/* The sensor's ring ids for a context created without lfx_config.ring_ids (n distinct ids, n <= the context's max_rings;
 * any order: results list rings by id ascending).  ids = NULL: back to 0 .. max_rings-1.  Takes effect with the next
 * batch; ids other than 0 .. n-1 go through the bucketing route (the organised-scan kernel reads ring r at column
 * offset r).  Waits for the context's stream. */
int lfx_set_ring_ids(lfx_ctx *ctx, const uint16_t *ids, uint32_t n);
/* Which route each scan of the last batch took (diagnostics; waits for `stream`): routes[s] = 1 read in place by the
 * organised-scan kernel, 2 the same through per-ring transforms (rings rotated / reversed in the stream), 3 read in place
 * as a grid with (0, 0, 0) records that the zero filter dropped (sorted_index holds its points' indices), 0 bucketed. */
int lfx_scan_routes(lfx_ctx *ctx, void *stream, uint8_t *routes /* [batch] */);

/* Pinned host memory for the caller's point buffers: lfx_extract reads a buffer allocated here by DMA (3.7 MB in
 * ~70 us for a 64 x 1800 scan); any other host pointer is first copied, chunk by chunk, through the context's own
 * pinned staging buffer (CPU memcpy speed).  Free with lfx_host_free before or after lfx_destroy. */
int lfx_host_alloc(lfx_ctx *ctx, size_t bytes, void **out);
void lfx_host_free(lfx_ctx *ctx, void *ptr);

/* --- PointCloud2 on either side of the operator ---------------------------- */
/* The record layout for lfx_config from a message's field list: what pcl::fromROSMsg<PointXYZIR>
 * (ros_msg.hpp:72-78) needs from it -- x, y, z as FLOAT32 -- plus the ring channel the node insists on.
 * Other fields (intensity, time, reflectivity ...) are skipped, as the upstream converter's field filter
 * does (convert.py:113-121).  Returns LFX_ERR_NO_RING_FIELD / LFX_ERR_UNSUPPORTED_FIELD. */
int lfx_layout_from_fields(const lfx_point_field *fields, uint32_t n_fields, uint32_t point_step, int is_bigendian,
                           lfx_layout *out);
/* The last device batch's edge and surface clouds as pcl::PointXYZ wire records (point_step 16:
 * x, y, z, 1.0f -- what ToPointXYZ + toROSMsg publish as scan_edge / scan_surface,
 * feature_extraction.cpp:163-170), packed back to back in scan order exactly as lfx_pack_features
 * does (same offsets table).
 * A short capacity_points (all four lfx_pack_* calls): records at or past capacity_points are not written -- nothing is
 * stored beyond [capacity_points] records of any output buffer -- while the offsets table is complete, the counts of every
 * scan and the totals as if everything had fitted.  A caller compares entry [batch] (for the surface cloud [2*batch+1])
 * with its capacity: a larger entry means the payload was cut there, and a second call with room for it gets all of it.
 * capacity_points above 2^32 - 1 counts as 2^32 - 1 (a batch holds fewer records than that). */
int lfx_pack_xyz(lfx_ctx *ctx, float *d_edge_out, float *d_surface_out, uint32_t *d_offsets_out,
                 size_t capacity_points, void *stream);
/* The same clouds as tight x, y, z triples (12 bytes per point, [capacity_points][3] floats): the least that has
 * to cross xGMI when the clouds of several GPUs are gathered to one (gather.py, bench.py).  A short capacity_points: as
 * lfx_pack_xyz -- no float at or past 3 * capacity_points is written, the table is complete. */
int lfx_pack_xyz12(lfx_ctx *ctx, float *d_edge_out, float *d_surface_out, uint32_t *d_offsets_out,
                   size_t capacity_points, void *stream);
/* colored_scan (feature_extraction.cpp:153,161) of the last device batch as pcl::PointXYZRGB wire records
 * (point_step 32: x, y, z, 1.0f | rgb bit-cast to float, 0, 0, 0; rgb = 0xFF<<24 | r<<16 | g<<8 | b with the
 * table of color_points.cpp:39-68): for every scan the points of each ring that was labelled (status
 * LFX_RING_OK), rings ascending, angle ascending -- the reference appends ring by ring and skips a ring it
 * abandons.  d_offsets_out u32 [batch+1]: exclusive prefix of the per-scan point counts (entry [batch] = total).
 * d_colored_out [capacity_points][8] floats.  A short capacity_points: as lfx_pack_xyz -- no record at or past it is
 * written, the table is complete, the caller compares entry [batch] with its capacity. */
int lfx_pack_colored(lfx_ctx *ctx, float *d_colored_out, uint32_t *d_offsets_out, size_t capacity_points,
                     void *stream);
/* Pack the last device batch's edge and surface clouds back to back, in scan order, into
 * caller-provided DEVICE buffers (what one rank hands to the multi-GPU gather):
 * d_edge_out / d_surface_out [capacity_points][4] floats (16-byte aligned); d_offsets_out u32
 * [2][batch+1]: exclusive prefix of the per-scan edge counts, then of the surface counts
 * (entry [batch] = total).  Asynchronous on `stream`.  A short capacity_points: as lfx_pack_xyz -- records at or past it
 * are not written (each cloud against its own offsets), the table is complete, the caller compares entries [batch] and
 * [2*batch+1] with its capacity. */
int lfx_pack_features(lfx_ctx *ctx, float *d_edge_out, float *d_surface_out, uint32_t *d_offsets_out,
                      size_t capacity_points, void *stream);
/* Copy scan `scan` of the last device batch to host memory (synchronises the stream). */
int lfx_download_scan(lfx_ctx *ctx, uint32_t scan, void *stream, lfx_scan_result *out);

/* --- multi-GPU: one process per GPU, scans sharded scan i -> rank i mod N, clouds gathered to one rank ------------- */
/* The reference node is stateless per message (feature_extraction.cpp:173-179), so scans are independent units and the
 * only exchange is the gather of the variable-length edge / surface clouds.  It runs over RCCL directly (librccl is
 * opened at the first call; point-to-point send / recv over the direct xGMI links, no ring, no reduction).
 * Bootstrap as with NCCL: rank 0 makes an id (lfx_comm_unique_id), the caller hands it to every rank by whatever means
 * it has (MPI, a socket, torch.distributed ...), every rank calls lfx_comm_create with it. */
#define LFX_COMM_ID_BYTES 128
typedef struct lfx_comm lfx_comm;
int lfx_comm_unique_id(uint8_t id[LFX_COMM_ID_BYTES]);
int lfx_comm_create(lfx_ctx *ctx, const uint8_t id[LFX_COMM_ID_BYTES], int rank, int world, lfx_comm **out);
void lfx_comm_destroy(lfx_comm *comm);
/* Gather of one step, in two halves so that a caller can run it one step behind the extraction (bench.py, gather.py):
 *   lfx_gather_counts   queues on `stream`: the all-gather of this rank's two totals (from d_offsets as written by
 *                       lfx_pack_xyz12 / lfx_pack_xyz / lfx_pack_features: entries [batch] and [2*batch+1]) and their copy
 *                       to pinned host memory.  Returns at once.
 *   lfx_gather_payload  waits (host) for those totals, then queues on `stream` one grouped send / recv: every rank
 *                       sends its first n_edge and n_surface records (floats_per_point floats each: 3 for xyz12, 4
 *                       for xyz / features) and its offsets table to `dst`; dst receives them rank after rank into
 *                       d_edge_all / d_surface_all (capacity_points records each; its own part is a device copy) and
 *                       d_offsets_all [world][2][batch+1].  counts_out (host, [world][2], may be NULL) receives the
 *                       totals of every rank on every rank; rank r's clouds start at the sum of the counts before it.
 *                       capacity_points is the destination's, given by EVERY rank (the same value): if the gathered
 *                       clouds do not fit, every rank returns LFX_ERR_CAPACITY and nothing is sent.
 * lfx_gather = both, one after the other.  Every rank must make the same sequence of calls. */
int lfx_gather_counts(lfx_ctx *ctx, lfx_comm *comm, const uint32_t *d_offsets, uint32_t batch, void *stream);
/* What this rank has posted on the communicator so far: [0] sends, [1] receives, [2] bytes sent, [3] bytes received,
 * [4] all-gathers of totals.  `dst` of lfx_gather_payload may change from call to call (every rank gives the same). */
#define LFX_COMM_STATS 5
int lfx_comm_stats(const lfx_comm *comm, uint64_t out[LFX_COMM_STATS]);
/* Two steps' exchanges as ONE group on ONE communicator: step A's clouds travel to steps[0].dst, step B's to steps[1].dst,
 * every rank posting its sends and receives of both between one ncclGroupStart / ncclGroupEnd -- two of a rank's xGMI links
 * carry data at once (a sender reaches a destination over one link), with no second communicator whose kernels could
 * start in another order on another rank.  Each step's totals come from the slot its lfx_gather_counts_slot call named
 * (LFX_GATHER_SLOTS = 2 may be out at once; lfx_gather_counts = slot 0).  n_steps = 1 or 2; batch, floats_per_point and
 * capacity_points are common to the steps; if either step's clouds do not fit, every rank returns LFX_ERR_CAPACITY and
 * nothing of either is sent.  Every rank must make the same sequence of calls with the same dst and slot values. */
#define LFX_GATHER_SLOTS 2
typedef struct lfx_gather_step
{
  int dst;                          /* destination rank of this step                                              */
  uint32_t slot;                    /* which lfx_gather_counts_slot call carries its totals                        */
  const float *d_edge, *d_surface;  /* this rank's packed clouds of the step (lfx_pack_xyz12 / _xyz / _features)   */
  const uint32_t *d_offsets;
  float *d_edge_all, *d_surface_all;    /* where this rank is dst: capacity_points records each; else may be NULL  */
  uint32_t *d_offsets_all;              /* [world][2][batch+1]                                                      */
  uint64_t *counts_out;                 /* host [world][2] or NULL: every rank's totals of the step                 */
} lfx_gather_step;
int lfx_gather_counts_slot(lfx_ctx *ctx, lfx_comm *comm, uint32_t slot, const uint32_t *d_offsets, uint32_t batch, void *stream);
int lfx_gather_payload2(lfx_ctx *ctx, lfx_comm *comm, const lfx_gather_step *steps, uint32_t n_steps, uint32_t batch,
                        uint32_t floats_per_point, size_t capacity_points, void *stream);
int lfx_gather_payload(lfx_ctx *ctx, lfx_comm *comm, int dst, const float *d_edge, const float *d_surface,
                       const uint32_t *d_offsets, uint32_t batch, uint32_t floats_per_point, float *d_edge_all,
                       float *d_surface_all, uint32_t *d_offsets_all, size_t capacity_points, uint64_t *counts_out,
                       void *stream);
int lfx_gather(lfx_ctx *ctx, lfx_comm *comm, int dst, const float *d_edge, const float *d_surface,
               const uint32_t *d_offsets, uint32_t batch, uint32_t floats_per_point, float *d_edge_all,
               float *d_surface_all, uint32_t *d_offsets_all, size_t capacity_points, uint64_t *counts_out, void *stream);

/* --- voxel-grid Downsample ------------------------------------------------------------------------- */
/* Downsample<T>(cloud, leaf) of lib/include/lidar_feature_library/downsample.hpp:37-51 (pcl::VoxelGrid with one leaf
 * size), which the localizer applies to scan_surface before it builds residuals (localization/.../surface.hpp:111),
 * for a batch of clouds that are already on the device.  Cloud s = d_count[s * count_stride] records of 4 floats
 * (x, y, z, -) from record d_begin[s] of d_points; its downsampled cloud (x, y, z, 1: pcl::PointXYZ) is written from
 * record d_begin[s] of d_out, cells in ascending cell index, d_out_count[s] records; d_status[s] = 1 where PCL gives
 * the cloud back unfiltered because the leaf is too small for its extent (nothing is written then).  PARITY UNPINNED:
 * VoxelGrid's arithmetic is PCL's, a third-party library that is neither under the reference tree nor in this image;
 * implemented from its published algorithm (PCL 1.12.1), points of a cell summed in input order.  Asynchronous.
 * Where PCL's arithmetic is undefined, these rules hold:
 *   - a point whose x, y or z is not finite is skipped, as VoxelGrid does for a cloud not marked dense: it takes no part
 *     in the bounds, the cells or the centroids; a cloud of such points only gives 0 cells and status 0;
 *   - status 1 ("leaf too small") where, with inv = 1.0f / leaf, an axis's (max - min) * inv is not finite or does not
 *     fit int64; where PCL's dx * dy * dz > INT_MAX (d = (int64)((max - min) * inv) + 1); where floor(min * inv) or
 *     floor(max * inv) of an axis lies outside int32; or where the product of the div_b (floor(max * inv) -
 *     floor(min * inv) + 1) exceeds 2^32.  The last is a deviation: PCL's index would wrap there and merge distinct
 *     cells, and PCL filters the cloud;
 *   - the cell index i0 + i1 * div_b[0] + i2 * div_b[0] * div_b[1] (i = floor(x * inv) - (float)min_b, in float as
 *     PCL) is computed in unsigned 32-bit arithmetic: PCL's static_cast<unsigned>(int idx) without its signed overflow. */
int lfx_voxel_downsample(lfx_ctx *ctx, const float *d_points, const uint32_t *d_begin, const uint32_t *d_count,
                         uint32_t count_stride, uint32_t n_clouds, size_t total_points, float leaf, float *d_out,
                         uint32_t *d_out_count, uint32_t *d_status, void *stream);
/* The same for the surface clouds of the last device batch (scan s: the scan's n_surface points): d_out laid out like
 * lfx_device_view::surface_points, d_out_count / d_status [batch]. */
int lfx_downsample_surface(lfx_ctx *ctx, float leaf, float *d_out, uint32_t *d_out_count, uint32_t *d_status, void *stream);

/* --- the map a scan is matched against ---------------------------------------------------------------- */
/* KDTreeEigen (localization/include/lidar_feature_localization/kdtree.hpp:50-63, src/kdtree.cpp:37-68; MakeKDTree :66-71):
 * built once per map, answers exact k-nearest queries.  lfx_map_create copies n_points records of 4 floats (x, y, z, -)
 * from the device into an index of its own: a uniform grid of cubic cells of cell_size (map units; grown if the map's
 * extent would need more than 2^25 cells), the points sorted by cell -- or, with cell_size 0, no grid: every query reads
 * the whole map (small maps; the check of the grid).  Both answer alike: neighbours by ascending squared distance,
 * equal distances by the lower index in the map as given (nanoflann leaves that order open).  Points must be finite.
 * Synchronous on `stream`.  A map belongs to the device of the context that made it and outlives nothing: destroy it
 * before the context's device is reset. */
typedef struct lfx_map lfx_map;
int lfx_map_create(lfx_ctx *ctx, const float *d_points, uint32_t n_points, float cell_size, lfx_map **out, void *stream);
/* The same from host memory (the points are staged through a temporary device buffer). */
int lfx_map_create_host(lfx_ctx *ctx, const float *points, uint32_t n_points, float cell_size, lfx_map **out, void *stream);
void lfx_map_destroy(lfx_map *map);
int lfx_map_info(const lfx_map *map, uint32_t *n_points, float *cell_size /* 0: no grid */, int32_t dims[3]);
/* KDTreeEigen::NearestKSearch (src/kdtree.cpp:44-68) for n_queries queries of 3 doubles on the device: per query the k
 * nearest points of the map -- d_neighbours [n][k][3] doubles (GetRows of the map), d_squared_distances [n][k],
 * d_indices [n][k] into the map as given; any of the three may be NULL.  k <= 16.  Asynchronous. */
int lfx_map_nearest(lfx_ctx *ctx, const lfx_map *map, const double *d_queries, uint32_t n_queries, uint32_t k,
                    double *d_neighbours, double *d_squared_distances, uint32_t *d_indices, void *stream);

/* --- scan-to-map residual build (first slice) --------------------------------------------------------- */
/* What the reference's localizer does first with scan_edge / scan_surface, on clouds that are already on the device:
 *   LFX_RESIDUAL_EDGE     Edge::Make (localization/include/lidar_feature_localization/edge.hpp:86-124): per point the k
 *                         nearest points of the edge map, their mean and principal direction, residual[3] =
 *                         (p - p1) x (p - p2) and the 3 x 7 row [Hat(p2 - p1) DRpDq(q, p0), Hat(p2 - p1)];
 *   LFX_RESIDUAL_SURFACE  Surface::MakeFromDownsampled (surface.hpp:116-139; downsample first: lfx_downsample_surface):
 *                         the plane X w = -1 through the k nearest points of the surface map, residual[1] = signed
 *                         point-plane distance and the 1 x 7 row [u^T DRpDq(q, p), u^T], u = w / |w|.
 * pose: point_to_map as [R | t], row-major 3 x 4 doubles (host); clouds as in lfx_voxel_downsample; outputs addressed
 * like the points (record d_begin[s] + i): d_residual 3 (edge) or 1 (surface) doubles per point, d_jacobian 21 or 7
 * doubles per point, row-major.  n_neighbors <= 16 (the localizer uses 15).  Exact nearest-neighbour search (the
 * reference's nanoflann KD-tree is exact too).  PARITY UNPINNED: Eigen's and nanoflann's arithmetic is not available
 * here; tolerance-level agreement with the CPU restatement, edge rows up to the sign of the principal direction (see
 * DESIGN.md).  Asynchronous.
 * The principal direction u is found in closed form; with l1 >= l2 >= l3 the covariance's eigenvalues and kappa =
 * l1 / (l1 - l2), |sin(u, the true direction)| <= 2^-53 (8 kappa + 4 kappa^2) (linear for line-like neighbourhoods,
 * quadratic for nearly round discs: below what half a float32 spacing of the map's coordinates moves the direction for
 * kappa < 1e8), |u| = 1 to 4 x 2^-53, and the row's Hat block is Hat(2 u) exactly, wherever the map lies.  An isotropic
 * neighbourhood (l1 = l3: one point, +-e_i, a cube's corners) gives the row of u = (0, 0, 1).
 * The quaternion q of the pose is Eigen::Quaterniond(Matrix3d)'s: trace > 0 -> w > 0; otherwise the component of the
 * largest diagonal entry is the positive one (the first of equal entries) -- that fixes q's sign and with it the sign of
 * the four quaternion columns of every row.  (tests/test_rows_gpu.py holds all of this against a 50-digit reference.) */
#define LFX_RESIDUAL_EDGE 0
#define LFX_RESIDUAL_SURFACE 1
int lfx_scan_to_map_residuals(lfx_ctx *ctx, int kind, const lfx_map *map, const double pose[12], uint32_t n_neighbors,
                              const float *d_points, const uint32_t *d_begin, const uint32_t *d_count,
                              uint32_t count_stride, uint32_t n_clouds, uint32_t max_points_per_cloud,
                              double *d_residual, double *d_jacobian, void *stream);
/* The same for the edge clouds of the last device batch (outputs laid out like lfx_device_view::edge_points). */
int lfx_edge_residuals(lfx_ctx *ctx, const lfx_map *map, const double pose[12], uint32_t n_neighbors,
                       double *d_residual, double *d_jacobian, void *stream);

/* --- the optimizer around those rows (second slice) ---------------------------------------------------- */
/* Optimizer<LOAMOptimizationProblem, EdgeSurfaceScan>::Run (localization/include/lidar_feature_localization/
 * optimizer.hpp:79-123, as Localizer::Update calls it, localizer.hpp:76) for a batch of scans against one pair of maps
 * (lfx_map_create: the reference builds its two KD-trees in the problem's constructor, loam_optimization_problem.hpp:54-60),
 * every scan from its own initial pose, all iterations on the device: per iteration Problem::Make (the two row builds
 * above, edge rows first: loam_optimization_problem.hpp:62-84), ComputeErrors, NormalizeErrorScale (Scale = 1.4826 *
 * median absolute deviation, robust.cpp:36-50), ComputeWeights (HuberDerivative, k = 1.345), WeightedUpdate (sums of
 * J^T J, w J^T J, w J^T r; IsDegenerate(D, 0.1) -> no step; -(M^T A M).llt().solve(M^T b), optimizer.cpp:40-71),
 * q <- q * AngleAxisToQuaternion(dx[0:3]), t <- t + dx[3:6], and the stopping tests in the reference's order (error
 * larger than before, scale larger than before, |dq.vec| and |dt| < 1e-3, max_iter).  A scan that has stopped costs no
 * further work.  The surface clouds are the ones AFTER Downsample (surface.hpp:111; lfx_downsample_surface, leaf 1.0).
 * max_*_points_per_cloud must be at least the longest cloud's count (they size the launches; lfx_localize_batch reads the
 * counts back itself), total_*_points the extent of the point arrays in records (rows are addressed like the points).
 * initial_poses: [n_clouds][12] host doubles ([R | t] row-major); results: [n_clouds], host.  Synchronous on `stream`.
 * PARITY UNPINNED (Eigen / nanoflann / PCL arithmetic underneath; see lfx_scan_to_map_residuals): results agree with the
 * CPU restatement to tolerance, and the restatement passes the reference's own optimizer tests. */
#define LFX_ALIGN_CONVERGED 0      /* "Optimization successfully converged"           success */
#define LFX_ALIGN_LARGER_ERROR 1   /* "The error is larger than previous iteration"   success */
#define LFX_ALIGN_LARGER_SCALE 2   /* "The scale is larger than previous iteration"   success */
#define LFX_ALIGN_MAX_ITERATION 3  /* "The iteration reached the maximum value"       failure */
#define LFX_ALIGN_EMPTY_INPUT 4    /* "The input data is empty"                       failure */
#define LFX_ALIGN_NO_PLANE 5       /* "No surface neighbourhood spans a plane"        failure: not a status of the reference --
                                    * every surface row of the scan was a zero row (its k nearest map points coincide, lie on
                                    * one line or on a plane through the origin: surface.hpp:78-83 has a zero pivot there and
                                    * Eigen's solve() hands back NaN, with which the reference runs to its iteration limit) */
#define LFX_ALIGN_SUCCESS(code) ((code) <= LFX_ALIGN_LARGER_SCALE)
typedef struct lfx_align_result {   /* OptimizationResult, optimization_result.hpp:35-43 */
  double pose[12];                  /* [R | t] row-major 3 x 4 */
  double error;                     /* sum of squared residuals at the last Problem::Make */
  double error_scale;
  int32_t iteration;
  int32_t code;                     /* LFX_ALIGN_*; text: lfx_align_message */
} lfx_align_result;
const char *lfx_align_message(int code);
int lfx_scan_to_map_align(lfx_ctx *ctx, const lfx_map *edge_map, const lfx_map *surface_map, uint32_t n_neighbors, int max_iter,
                          const float *d_edge_points, const uint32_t *d_edge_begin, const uint32_t *d_edge_count,
                          uint32_t edge_count_stride, uint32_t max_edge_points_per_cloud, size_t total_edge_points,
                          const float *d_surface_points, const uint32_t *d_surface_begin, const uint32_t *d_surface_count,
                          uint32_t surface_count_stride, uint32_t max_surface_points_per_cloud, size_t total_surface_points,
                          uint32_t n_clouds, const double *initial_poses, lfx_align_result *results, void *stream);
/* The same loop on AlignmentProblem (localization/src/alignment.cpp:33-78: rows [DRpDq(q, x), I], residual pose * x - y),
 * the problem the reference's optimizer tests run (localization/test/test_optimizer.cpp).  d_source / d_target: records
 * of 3 doubles on the device, cloud s = d_count[s] records from record d_begin[s]. */
int lfx_align_point_pairs(lfx_ctx *ctx, const double *d_source, const double *d_target, const uint32_t *d_begin,
                          const uint32_t *d_count, uint32_t max_points_per_cloud, size_t total_points, uint32_t n_clouds,
                          int max_iter, const double *initial_poses, lfx_align_result *results, void *stream);
/* Localizer::Update (localizer.hpp:71-80) for every scan of the last device batch: Downsample(scan_surface, surface_leaf)
 * (the reference uses 1.0), then lfx_scan_to_map_align on scan_edge and the downsampled cloud; nothing leaves the device
 * but the results. */
int lfx_localize_batch(lfx_ctx *ctx, const lfx_map *edge_map, const lfx_map *surface_map, uint32_t n_neighbors, int max_iter,
                       float surface_leaf, uint32_t n_scans /* = scans of the last batch: sizes initial_poses[n][12], results[n] */,
                       const double *initial_poses, lfx_align_result *results, void *stream);

/* Localizer::Update for one scan whose two clouds are on the host -- the consumer in a process of its own, handed
 * scan_edge / scan_surface as published (records of 4 floats: x, y, z, -; pcl::PointXYZ on the wire): upload, Downsample
 * of the surface cloud, lfx_scan_to_map_align.  Synchronous. */
int lfx_localize_host(lfx_ctx *ctx, const lfx_map *edge_map, const lfx_map *surface_map, uint32_t n_neighbors, int max_iter,
                      float surface_leaf, const float *edge_points, uint32_t n_edge, const float *surface_points,
                      uint32_t n_surface, const double initial_pose[12], lfx_align_result *result, void *stream);

/* --- how good a pose is: the report of an alignment --------------------------------------------------------------------- */
/* The reference's optimizer computes D = sum J^T J and A = sum w J^T J in every iteration (optimizer.cpp:40-72), asks D one
 * yes / no question (IsDegenerate(D, 0.1), degenerate.cpp:32-37) and throws both away; its node publishes a constant
 * covariance (subscriber.hpp:158-169).  The *_report calls below run the plain call (the results are the same bits) and then
 * fill one record per scan AT THE POSE THE ALIGNMENT RETURNED (result.pose): one more Problem::Make there -- search and rows,
 * the kernels the iterations use, the pose handed over as lfx_scan_to_map_residuals hands it over, so that entry point
 * gives the rows the report was made from -- and one reduction.  The pose does not move.  Scans whose code is a success or
 * LFX_ALIGN_MAX_ITERATION get a report; for the others (and where H holds a NaN or an eigen-solve does not settle) valid is
 * 0 and every other byte of the record is 0.  w_i are the weights the optimizer would use at this pose:
 * HuberDerivative(e_i / (Scale(e) + 1e-16)), k = 1.345, e_i = r_i . r_i, the three rows of an edge residual sharing one
 * weight (ComputeErrors / NormalizeErrorScale / ComputeWeights, optimizer.cpp:100-128).  The residuals mix units (an edge
 * residual is a cross product, a surface one a distance), as they do in the reference's cost: sigma2 is the variance of that
 * mixture.  The covariance is the Gauss-Newton one: it knows nothing of the map's own noise, of wrong associations or of
 * the robust scale's variance (DESIGN.md section 7 has the calibration measured on the synthetic room).  Sums are taken in a
 * fixed order: the same inputs give the same bytes. */
typedef struct lfx_align_report {
  double information[36];   /* H = M^T (sum_i w_i J_i^T J_i) M, 6 x 6 row-major, in the optimizer's own coordinates dx
                               (optimizer.cpp:87-98): dx[0:3] the rotation increment applied as q <- q * AngleAxis(dx[0:3])
                               (the scan's frame), dx[3:6] the translation increment in the map frame; M = MakeM(q) */
  double eigenvalues[6];    /* of H, ascending */
  double eigenvectors[36];  /* row k: the unit eigenvector of eigenvalues[k]; sign: its largest-magnitude component > 0 */
  double covariance[36];    /* sigma2 * sum_k v_k v_k^T / max(eigenvalues[k], floor),  floor = 1e-9 * eigenvalues[5]: finite,
                               and LARGE along a direction the scan does not constrain.  "Finite" holds where sigma2 is:
                               where sigma2 is NaN every entry is NaN, valid stays 1 and every other field is as defined */
  double sigma2;            /* sum_i w_i e_i / (sum_i w_i dim_i - 6): weighted residual variance; dim_i = 3 for an edge
                               residual and 1 for a surface one; NaN where the denominator is <= 0 */
  double min_eigenvalue_d;  /* smallest eigenvalue of the 7 x 7 D = sum_i J_i^T J_i: what IsDegenerate compares with 0.1 */
  double error, error_scale;/* sum_i e_i and Scale(e) (robust.cpp:37-51) at this pose */
  double rms_edge, rms_surface;          /* sqrt(mean e_i) per kind; 0 where the kind has no row */
  uint32_t n_edge, n_surface;            /* residuals of each kind */
  uint32_t n_edge_inliers, n_surface_inliers;   /* those with w_i == 1 (HuberDerivative's first branch) */
  uint32_t n_surface_no_plane;           /* surface rows that are zero rows (see LFX_ALIGN_NO_PLANE) */
  int32_t rank;                          /* number of eigenvalues[k] > floor */
  int32_t degenerate;                    /* IsDegenerate(D, 0.1): the update the optimizer would refuse here */
  int32_t valid;                         /* 0: no report (empty input, LFX_ALIGN_EMPTY_INPUT / NO_PLANE / NOT_RUN, a NaN in H) */
} lfx_align_report;
/* The three calls above with one more argument: reports, host, [n_clouds] ([n_scans]; one record for lfx_localize_host). */
int lfx_scan_to_map_align_report(lfx_ctx *ctx, const lfx_map *edge_map, const lfx_map *surface_map, uint32_t n_neighbors, int max_iter,
                                 const float *d_edge_points, const uint32_t *d_edge_begin, const uint32_t *d_edge_count,
                                 uint32_t edge_count_stride, uint32_t max_edge_points_per_cloud, size_t total_edge_points,
                                 const float *d_surface_points, const uint32_t *d_surface_begin, const uint32_t *d_surface_count,
                                 uint32_t surface_count_stride, uint32_t max_surface_points_per_cloud, size_t total_surface_points,
                                 uint32_t n_clouds, const double *initial_poses, lfx_align_result *results,
                                 lfx_align_report *reports, void *stream);
int lfx_localize_batch_report(lfx_ctx *ctx, const lfx_map *edge_map, const lfx_map *surface_map, uint32_t n_neighbors, int max_iter,
                              float surface_leaf, uint32_t n_scans, const double *initial_poses, lfx_align_result *results,
                              lfx_align_report *reports, void *stream);
int lfx_localize_host_report(lfx_ctx *ctx, const lfx_map *edge_map, const lfx_map *surface_map, uint32_t n_neighbors, int max_iter,
                             float surface_leaf, const float *edge_points, uint32_t n_edge, const float *surface_points,
                             uint32_t n_surface, const double initial_pose[12], lfx_align_result *result,
                             lfx_align_report *report, void *stream);
/* A report's covariance as geometry_msgs/PoseWithCovariance orders it (x, y, z, rotation about the fixed X, Y, Z axes):
 * out = T C T^T with T = [[0, I], [R, 0]], R the rotation of `pose` (a rotation increment d in the scan's frame is R d in the
 * map frame).  Host only, no context; every sum of three terms is (a0 b0 + a1 b1) + a2 b2, unfused; out may be covariance. */
int lfx_align_covariance_ros(const double pose[12], const double covariance[36], double out[36]);

/* --- scan-to-local-map odometry (the odometry row) -------------------------------------------------------- */
/* Odometry<PoseUpdater, EdgeSurfaceMap, EdgeSurfaceScan> (localization/include/lidar_feature_localization/odometry.hpp:52-63)
 * over EdgeSurfaceMap (edge_surface_map.hpp:38-76: two RecentScans, recent_scans.hpp:56-88), every cloud on the device.
 * Update(scan): no scan added yet -> add the scan at the current pose; else align it against the merged last n_local_scans
 * scans (GetRecent) from the current pose and take result.pose whatever the code, then add it transformed by that pose.
 * The alignment is the problem Localizer::Update runs (lfx_localize_batch): edge rows against the window's edge map,
 * surface rows of Downsample(scan_surface, surface_leaf) against the window's surface map, Optimizer::Run with
 * n_neighbors / max_iter.  DEFINED DEVIATION: where a window map holds fewer than n_neighbors points (the reference reads
 * nanoflann's uninitialised output there) the scan is not aligned: aligned = 0, the pose is carried over, the scan is added.
 * The store: one linear device buffer per cloud, scans in insertion order, the window a contiguous suffix (so the map's
 * "lower index" tie order is MergeClouds order); everything is kept while the capacity allows (GetAll); when the next scan
 * would not fit, the scans older than the window are discarded (the window moved to the front); a scan that does not fit
 * even then fails the call with pose, store and counts unchanged.  Added clouds hold the raw scan (not downsampled),
 * transformed as pcl::transformPointCloud with an Affine3d does: each coordinate ((r0*x + r1*y) + r2*z) + t in double,
 * rounded once to float, the 4th float of a record copied.  An odometry belongs to the device of the context that made it;
 * it leaves the context's batch results as they were.  Poses: [R | t] row-major 3 x 4 doubles (point_to_map).
 * Waits: the results and the pose are final when a call returns (the alignment waits for itself); the scan's addition to
 * the store may still be queued on `stream` -- read the store after `stream`, and keep a caller's device clouds until
 * `stream` has passed the call.  The next call, or the next window rebuild, waits for it where nothing has since. */
#define LFX_ALIGN_NOT_RUN 6        /* odometry: the scan was not aligned (first scan, or a window map under n_neighbors points) */
typedef struct lfx_odometry lfx_odometry;
typedef struct lfx_odometry_config {
  uint32_t n_local_scans;          /* GetRecent(n): 7 in app/odometry.cpp; >= 1 */
  uint32_t n_neighbors;            /* N_NEIGHBORS: 15; in [3, 16] */
  int32_t max_iter;                /* Optimizer's default: 20; >= 1 */
  float surface_leaf;              /* Downsample leaf of the surface rows: 1.0 */
  float edge_cell, surface_cell;   /* grid cell of the window maps (0: no grid), as lfx_map_create */
  uint64_t edge_capacity_points, surface_capacity_points;   /* the device store, records of 4 floats; >= 1 */
  double initial_pose[12];         /* Odometry's pose_ before the first scan: identity */
} lfx_odometry_config;
/* n_local_scans 7, n_neighbors 15, max_iter 20, surface_leaf 1.0, cells 1.0, capacities 2^22 points, identity */
void lfx_odometry_default_config(lfx_odometry_config *config);
typedef struct lfx_odometry_result {
  lfx_align_result align;          /* what Optimizer::Run gave; not aligned: the carried pose, iteration 0, LFX_ALIGN_NOT_RUN */
  uint32_t n_edge_map, n_surface_map;   /* window sizes the scan was aligned against (0, 0 for the first scan) */
  int32_t aligned;                 /* 0: first scan, or a window map with fewer than n_neighbors points */
} lfx_odometry_result;
typedef struct lfx_odometry_store_view {
  uint32_t n_scans;                /* scans retained in the store (GetAll) */
  uint32_t n_window_scans;         /* the last min(n_local_scans, n_scans) of them (GetRecent) */
  uint64_t n_added;                /* scans added since create */
  uint64_t dropped_scans;          /* scans discarded to make room */
  uint64_t compactions;            /* times the window was moved to the front of the store */
  const float *edge_points;        /* device: the retained transformed edge clouds, n_edge records of 4 floats */
  const float *surface_points;     /* device: the same for the surface clouds */
  uint64_t n_edge, n_surface;
  const float *edge_window;        /* device: the suffix the next scan is aligned against (GetRecent) */
  const float *surface_window;
  uint32_t n_edge_window, n_surface_window;
  const uint32_t *edge_offsets;    /* host [n_scans + 1]: first record of every retained scan; valid until the next call */
  const uint32_t *surface_offsets;
  double pose[12];                 /* CurrentPose */
} lfx_odometry_store_view;
/* Allocates the store and the window maps' first buffers; synchronous. */
int lfx_odometry_create(lfx_ctx *ctx, const lfx_odometry_config *config, lfx_odometry **out);
void lfx_odometry_destroy(lfx_odometry *odometry);
/* Odometry::Update for every scan of the last device batch, in batch order (n_scans = scans of the last batch, sizes
 * results[n]).  The batch's surface clouds are downsampled once up front, and their counts read in one wait. */
int lfx_odometry_update_batch(lfx_ctx *ctx, lfx_odometry *odometry, uint32_t n_scans, lfx_odometry_result *results, void *stream);
/* Odometry::Update for one scan whose clouds (records of 4 floats) are on the device. */
int lfx_odometry_update(lfx_ctx *ctx, lfx_odometry *odometry, const float *d_edge, uint32_t n_edge, const float *d_surface,
                        uint32_t n_surface, lfx_odometry_result *result, void *stream);
/* The same for clouds on the host (scan_edge / scan_surface as a subscriber receives them): staged through a device buffer
 * of the odometry's own, grown when a scan needs more. */
int lfx_odometry_update_host(lfx_ctx *ctx, lfx_odometry *odometry, const float *edge, uint32_t n_edge, const float *surface,
                             uint32_t n_surface, lfx_odometry_result *result, void *stream);
/* EdgeSurfaceMap::Add with a caller-given pose (poses from elsewhere); the current pose is left as it is.  Queued on `stream`. */
int lfx_odometry_add(lfx_ctx *ctx, lfx_odometry *odometry, const double pose[12], const float *d_edge, uint32_t n_edge,
                     const float *d_surface, uint32_t n_surface, void *stream);
int lfx_odometry_pose(const lfx_odometry *odometry, double pose[12]);   /* CurrentPose */
/* Reports (lfx_align_report) of the scans the update* calls align: off by default.  lfx_odometry_reports copies those of the
 * LAST update* call, one per scan in its order (valid 0 for a scan that was not aligned), at most `capacity` of them, and
 * sets *n to how many there are (0 while reports are off). */
int lfx_odometry_set_reports(lfx_odometry *odometry, int on);
int lfx_odometry_reports(const lfx_odometry *odometry, lfx_align_report *out, uint32_t capacity, uint32_t *n);
/* The store (GetAll), the window (GetRecent), per-scan offsets and what was dropped. */
int lfx_odometry_view(const lfx_odometry *odometry, lfx_odometry_store_view *view);
/* EdgeSurfaceMap::Save(dirname) (edge_surface_map.hpp:66-70, through SaveMapIfNotEmpty, map_io.hpp:40-56): the store (GetAll)
 * written as dirname/edge.pcd and dirname/surface.pcd with lfx_pcd_write, each only if that cloud is non-empty;
 * written[0] / [1] = 1 where a file was written.  A store that has dropped scans (dropped_scans > 0) saves only the scans it
 * kept.  Reads the store on `stream` (after the odometry's queued appends there); synchronous. */
int lfx_odometry_save(lfx_ctx *ctx, const lfx_odometry *odometry, const char *dirname, int written[2], void *stream);

/* --- map files (PCD) and the keyframe map builder (the mapping row) ---------------------------------------- */
/* The mapping node (mapping/include/lidar_feature_mapping/map.hpp, mapping/src/mapping.cpp) builds a map from clouds and
 * poses and writes it with pcl::io::save; the localization node reads maps with pcl::io::loadPCDFile<pcl::PointXYZ>
 * (localization/app/localization.cpp:67-85).  These need no context and no device.
 *
 * lfx_pcd_read takes what loadPCDFile<pcl::PointXYZ> takes: v0.7 and v0.6 headers (# comment lines allowed; FIELDS, SIZE,
 * TYPE, COUNT (optional, 1 each), WIDTH, HEIGHT, VIEWPOINT (parsed, not applied: PCL does not apply it either), POINTS,
 * DATA; POINTS must be WIDTH x HEIGHT, an organised cloud is read in file order); DATA ascii (one point per line, values
 * separated by white space; nan, inf and exponents), binary (records back to back, little-endian) and binary_compressed
 * (uint32 compressed size, uint32 uncompressed size, one LZF block in liblzf's format holding one field after another).
 * Fields are found by name; every field but x, y and z is skipped whatever its type and count (intensity, ring, curvature,
 * rgb, normals, _ padding).  DEFINED DEVIATION: x, y and z must each be TYPE F, SIZE 4, COUNT 1, else
 * LFX_ERR_UNSUPPORTED_FIELD (PCL loads zeros there with a warning).  An ascii line with the wrong number of values is
 * LFX_ERR_FILE (PCL skips it with a warning).
 * Output: records of 4 floats in file order, x, y, z and 1.0f (the 4th float of a pcl::PointXYZ).  points NULL: only the
 * header is read, n_points = POINTS.  n_nonfinite (may be NULL) counts records with a non-finite coordinate; with
 * drop_nonfinite set they are left out (lfx_map_create requires finite points), else kept.  capacity too small:
 * LFX_ERR_CAPACITY with n_points = the records needed.  A file that cannot be read, or is not such a PCD file (truncated
 * data, sizes that do not match, an LZF reference before the start of the output or a run past either end), is
 * LFX_ERR_FILE; nothing is read or written out of bounds.  msg (may be NULL) gets one line naming the header line or the
 * byte offset at fault. */
int lfx_pcd_read(const char *path, float *points /* host [capacity][4] or NULL */, uint64_t capacity, int drop_nonfinite,
                 uint64_t *n_points, uint64_t *n_nonfinite, char *msg, size_t msg_len);
/* pcl::io::save(name, pcl::PointCloud<pcl::PointXYZ>): DATA binary, the header
 *   # .PCD v0.7 - Point Cloud Data file format / VERSION 0.7 / FIELDS x y z / SIZE 4 4 4 / TYPE F F F / COUNT 1 1 1 /
 *   WIDTH n / HEIGHT 1 / VIEWPOINT 0 0 0 1 0 0 0 / POINTS n / DATA binary
 * (one line each, '\n'), then n x 12 bytes: x, y, z of every record (the 4th float is not written).  The header is this
 * project's reading of PCL 1.12's PCDWriter::generateHeader; byte equality with a file PCL writes is UNPINNED (PCL is
 * not available to build against).  The mapping node's own files carry extra curvature and ring columns (its PointType
 * is PointXYZCR, mapping.cpp:56; zero for clouds taken from scan_edge); this writes x y z only, and lfx_pcd_read and
 * loadPCDFile<PointXYZ> read either form.  n_points 0 is LFX_ERR_INVALID_ARGUMENT (PCL refuses an empty cloud; the
 * reference's savers skip empty maps). */
int lfx_pcd_write(const char *path, const float *points /* host [n][4] */, uint64_t n_points, char *msg, size_t msg_len);
/* The two quantities PoseDiffIsSufficientlySmall (map.hpp:49-60) compares, with d = pose0.inverse() * pose1:
 * translation = |d.translation()|, rotation = |Quaterniond(d.rotation()).vec()| (|sin(angle / 2)| of the relative
 * rotation).  The test is translation < t_thr && rotation < r_thr.  Poses [R | t] row-major.  Eigen 3.4's arithmetic,
 * restated in this order: inverse R0^T and -(R0^T t0); product R0^T R1 and R0^T t1 + (-(R0^T t0)); every 3-term sum as
 * (a0 b0 + a1 b1) + a2 b2; rotation() of an Isometry is its linear part; the quaternion from the matrix as Eigen's
 * (trace = (m00 + m11) + m22 > 0: s = 0.5 / sqrt(trace + 1), vec = (m21 - m12, m02 - m20, m10 - m01) * s; else the branch
 * of the largest diagonal entry i, j = i+1, k = j+1 mod 3: t = sqrt(((mii - mjj) - mkk) + 1), q_i = 0.5 t, q_j = (mji +
 * mij) * (0.5 / t), q_k = (mki + mik) * (0.5 / t)); norms as sqrt((x^2 + y^2) + z^2).  The decisions are pinned by the
 * reference's vectors (test_map.cpp:34-65); bits against Eigen are UNPINNED (Eigen 3.3's rotation() ran a polar
 * decomposition, which moves the last bits). */
int lfx_pose_diff(const double pose0[12], const double pose1[12], double *translation, double *rotation);

/* MapBuilder<PointType> (map.hpp:95-153) with its Map on the device: one mapper per map (an edge mapper and a surface
 * mapper for the two files).  Per cloud, in order: empty -> LFX_KEYFRAME_EMPTY, nothing changes; else, where the map holds
 * a point and lfx_pose_diff to the last added pose is below both thresholds -> LFX_KEYFRAME_TOO_CLOSE; else
 * LFX_KEYFRAME_ADDED: the cloud, transformed by its pose, is appended to the map and becomes the last added pose.  The
 * transform is odometry's (each coordinate ((r0*x + r1*y) + r2*z) + t in double, rounded once to float; the 4th float
 * copied).  The map grows to max(need, 1.5 x capacity), capped at max_points; a call that would pass max_points returns
 * LFX_ERR_CAPACITY, a failed allocation LFX_ERR_OUT_OF_MEMORY -- map, last pose, counters and outcomes untouched.
 * Waits: outcomes and counters are final when a call returns; the append may still be queued on `stream` -- read the map
 * (lfx_mapper_store_view.points) after `stream` has passed it, and keep a caller's device clouds until then.  Successive
 * calls may use different streams: a growth copy and lfx_mapper_save are ordered behind the previous call's append. */
typedef struct lfx_mapper lfx_mapper;
typedef struct lfx_mapper_config {
  double translation_threshold;      /* 1.0 (map.hpp:89) */
  double rotation_threshold;         /* 0.1 (map.hpp:90): |sin(angle / 2)| of the relative rotation */
  uint64_t initial_capacity_points;  /* records of 4 floats allocated at create: 2^20 */
  uint64_t max_points;               /* the map never holds more: 2^32 - 1 (lfx_map_create takes uint32) */
} lfx_mapper_config;
void lfx_mapper_default_config(lfx_mapper_config *config);
int lfx_mapper_create(lfx_ctx *ctx, const lfx_mapper_config *config, lfx_mapper **out);
void lfx_mapper_destroy(lfx_mapper *mapper);
#define LFX_KEYFRAME_ADDED 0
#define LFX_KEYFRAME_EMPTY 1       /* "Empty cloud observed. Do nothing and continue" (map.hpp:118-121) */
#define LFX_KEYFRAME_TOO_CLOSE 2   /* PoseDiffIsSufficientlySmall to the last added pose (map.hpp:123-129) */
/* MapBuilder::Callback for n_clouds clouds on the device, in order.  Cloud s is d_count[s * count_stride] records of 4
 * floats starting at record d_begin[s] of d_points (lfx_voxel_downsample's addressing: the last device batch's edge clouds
 * are view.edge_points, view.scan_begin, view.scan_info + 2, 4; its surface clouds the same with + 3); total_points = the
 * extent of d_points in records.  poses: host [n_clouds][12] ([R | t] row-major, finite); outcomes: host [n_clouds].  One
 * wait (the counts and begins), then one kernel for every added cloud.  NULL pointers, n_clouds 0, count_stride 0,
 * non-finite poses and clouds past total_points are LFX_ERR_INVALID_ARGUMENT. */
int lfx_mapper_add(lfx_ctx *ctx, lfx_mapper *mapper, const float *d_points, const uint32_t *d_begin, const uint32_t *d_count,
                   uint32_t count_stride, uint32_t n_clouds, size_t total_points, const double *poses /* host [n][12] */,
                   uint8_t *outcomes /* host [n] */, void *stream);
/* The same for one cloud on the host (the mapping node's subscriber), staged through a device buffer of the mapper's own. */
int lfx_mapper_add_host(lfx_ctx *ctx, lfx_mapper *mapper, const float *points, uint32_t n_points, const double pose[12],
                        uint8_t *outcome, void *stream);
typedef struct lfx_mapper_store_view {
  const float *points;               /* device: n_points records of 4 floats; valid until the next add (growth moves it) */
  uint64_t n_points, capacity_points;
  uint64_t n_added, n_empty, n_too_close;
  int32_t has_pose;                  /* 0 until a cloud is added */
  double last_pose[12];              /* prev_transform_: the pose of the last added cloud */
} lfx_mapper_store_view;
/* (the type is named as lfx_odometry_store_view is: a typedef may not share the function's name) */
int lfx_mapper_view(const lfx_mapper *mapper, lfx_mapper_store_view *view);
/* SaveMap (map.hpp:135-149): an empty map writes nothing, *written = 0 (the reference warns); else lfx_pcd_write of the
 * map read on `stream`, *written = 1.  Synchronous. */
int lfx_mapper_save(lfx_ctx *ctx, const lfx_mapper *mapper, const char *path, int *written, void *stream);

/* --- the rolling voxel map: one point per voxel in a window that follows the vehicle ------------------------------------- */
/* The map LOAM's mapping stage keeps (no reference counterpart): bounded in memory, cheap to insert into and to cut a local
 * map from.  Two stores, LFX_ROLLING_EDGE and LFX_ROLLING_SURFACE, each a direct-mapped, tagged voxel array with a leaf size
 * and a window of dims[3] voxels (any positive sizes; their product at most 2^31); 32 bytes per voxel (key, stamp, point).
 *   voxel    v_a = (int32)floorf(p_a * inv), inv = 1.0f / leaf in float (as lfx_voxel_downsample).  A point with a coordinate
 *            that is not finite or with |floorf(..)| >= 2^20 on an axis is dropped and counted as nonfinite.
 *   key      1 << 63 | (vx & 0x1FFFFF) | (vy & 0x1FFFFF) << 21 | (vz & 0x1FFFFF) << 42; 0 = never written.
 *   slot     s_a = v_a mod dims_a (non-negative); slot = (s_z * dims_y + s_y) * dims_x + s_x.
 *   window   origin o[3] in voxels, o_a <= v_a < o_a + dims_a; o_a = -(dims_a / 2) at create.  Moving it is host arithmetic:
 *            nothing on the device is touched.
 *   live     voxel v is live iff it lies in the window and keys[slot(v)] == key(v).  A slot that holds another voxel's key
 *            reads as empty and is overwritten by an insert.  A voxel that left the window and comes back is live again
 *            unless another voxel has taken its slot meanwhile.  Inside the window voxel -> slot is injective.
 *   insert   every record transformed by its cloud's pose (the odometry's and the mapper's transform: same bits).  Outside
 *            the window: dropped, counted as outside.  In a live voxel: counted as merged, the stored point stays.  Among the
 *            records of one call in the same voxel that is not live the one of the lowest rank is stored, all four floats
 *            (inserted), and the others count as merged; rank is (cloud index, index in the cloud), whatever order d_begin
 *            is in and however the device schedules the call.  inserted + merged + outside + nonfinite = records given.
 *   extract  the box lo .. hi (metres) is the voxels voxel(lo) .. voxel(hi) inclusive per axis ((float)lo_a through the voxel
 *            rule, clamped to [-2^20, 2^20 - 1]), clipped to the window; its live voxels' points in ascending (vz, vy, vx),
 *            x fastest.  hi < lo on an axis: no points.
 * Calls on one map are ordered behind its last insert whichever streams they use; an insert behind an extraction on another
 * stream is the caller's to order.  The map must be used with a context of the device it was created on. */
typedef struct lfx_rolling_map lfx_rolling_map;
#define LFX_ROLLING_EDGE 0
#define LFX_ROLLING_SURFACE 1
typedef struct lfx_rolling_map_config {
  float edge_leaf, surface_leaf;           /* metres: 0.2, 0.4 */
  uint32_t edge_dims[3], surface_dims[3];  /* voxels: 512, 512, 128 and 256, 256, 64 (102.4 x 102.4 x 25.6 m each; 1.2 GB) */
  /* lfx_rolling_map_update_batch: */
  float match_half_extent[3];              /* metres: the box around a scan's pose it is aligned against: 50, 50, 12.8 */
  uint32_t n_neighbors;                    /* 15; in [3, 16] */
  int32_t max_iter;                        /* 20 */
  float scan_surface_leaf;                 /* Downsample of a scan's surface cloud before its rows: 1.0 */
  float edge_cell, surface_cell;           /* grids of the two box maps, as lfx_map_create: 1.0 (0: no grid) */
  double initial_pose[12];                 /* identity */
} lfx_rolling_map_config;
void lfx_rolling_map_default_config(lfx_rolling_map_config *config);
/* A leaf <= 0 or not finite, a dimension of 0, a window of more than 2^31 voxels, n_neighbors outside [3, 16], max_iter < 1, a
 * negative extent or cell and an initial pose that is not finite are LFX_ERR_INVALID_ARGUMENT; a failed allocation is
 * LFX_ERR_OUT_OF_MEMORY with nothing left allocated. */
int lfx_rolling_map_create(lfx_ctx *ctx, const lfx_rolling_map_config *config, lfx_rolling_map **out);
void lfx_rolling_map_destroy(lfx_rolling_map *map);
/* Both windows centred on `center` (metres): o_a = voxel((float)center_a) - dims_a / 2 per kind.  O(1), no device work.  A
 * centre that is not finite or has no voxel is LFX_ERR_INVALID_ARGUMENT. */
int lfx_rolling_map_recenter(lfx_rolling_map *map, const double center[3]);
/* n_clouds device clouds into the store of `kind`, addressed as lfx_mapper_add's (cloud s: d_count[s * count_stride] records
 * from record d_begin[s] of d_points; total_points the extent of d_points in records); poses: host [n_clouds][12], finite.
 * One wait (the counts and begins), then two launches; they may still be queued on `stream` when the call returns.  A call
 * of more than 2^32 - 2 records is LFX_ERR_CAPACITY. */
int lfx_rolling_map_insert(lfx_ctx *ctx, lfx_rolling_map *map, int kind, const float *d_points, const uint32_t *d_begin,
                           const uint32_t *d_count, uint32_t count_stride, uint32_t n_clouds, size_t total_points,
                           const double *poses /* host [n][12] */, void *stream);
/* The same for one cloud on the host, staged through a device buffer of the map's own; the cloud has been read on return. */
int lfx_rolling_map_insert_host(lfx_ctx *ctx, lfx_rolling_map *map, int kind, const float *points, uint32_t n_points,
                                const double pose[12], void *stream);
/* The live voxels of a box as records of 4 floats to d_out (the lfx_pack_* convention: nothing is written at or past
 * capacity_points, *n_points is the full need; d_out may be NULL with capacity 0).  Waits: *n_points is final on return. */
int lfx_rolling_map_extract(lfx_ctx *ctx, const lfx_rolling_map *map, int kind, const double lo[3], const double hi[3],
                            float *d_out, uint64_t capacity_points, uint64_t *n_points /* host */, void *stream);
typedef struct lfx_rolling_map_view_t {    /* [0] the edge store, [1] the surface store */
  float leaf[2];
  uint32_t dims[2][3];
  int32_t origin[2][3];
  uint64_t n_inserted[2], n_merged[2], n_outside[2], n_nonfinite[2];   /* records, summed since create */
  uint64_t n_live[2];                      /* live voxels in the window now (a count pass over the window) */
  double pose[12], correction[12];         /* lfx_rolling_map_update_batch's current pose and C (map <- odometry frame) */
} lfx_rolling_map_view_t;
/* (the type is named apart from the function, as lfx_mapper_store_view is)  Waits for the counters and the count passes. */
int lfx_rolling_map_view(lfx_ctx *ctx, const lfx_rolling_map *map, lfx_rolling_map_view_t *view, void *stream);
/* edge.pcd and surface.pcd of the whole windows under dirname through lfx_pcd_write, as lfx_odometry_save: an empty store
 * writes no file (written[k] = 0).  With lfx_pcd_read and lfx_rolling_map_insert_host at the identity pose this seeds a map
 * of the same leaves from disk: a stored point is its own voxel's representative (the 4th float comes back as 1).
 * Synchronous. */
int lfx_rolling_map_save(lfx_ctx *ctx, const lfx_rolling_map *map, const char *dirname, int written[2], void *stream);
/* LOAM's mapping stage for every scan k of the last device batch, in order (n_scans = the batch's size).  odometry_poses:
 * host [n_scans][12], the scans' poses in an odometry's frame (lfx_odometry_update_batch's results), or NULL.
 *   1  initial = C x odom_k; C (map <- odometry frame) is the identity at create.  With NULL the initial pose is the current
 *      pose (config.initial_pose at create).  Poses compose in double, every 3-term sum as (a0 b0 + a1 b1) + a2 b2, the
 *      translation's as that sum + t; the inverse of a pose is [R^T | -(R^T t)] with the same sums.
 *   2  with t the initial translation: if for either kind on any axis |voxel(t_a) - (o_a + dims_a / 2)| > dims_a / 4, both
 *      windows are recentred at t (recentered 1).
 *   3  the boxes t -+ match_half_extent are extracted from both stores and indexed as lfx_map_create does (cells edge_cell /
 *      surface_cell); the scan's surface cloud is downsampled by scan_surface_leaf, once per batch up front.
 *   4  a box under n_neighbors points: the scan is not aligned (aligned 0, LFX_ALIGN_NOT_RUN), pose = initial, both raw
 *      clouds inserted at it (inserted 1).
 *   5  else the alignment of lfx_scan_to_map_align from the initial pose (aligned 1).  LFX_ALIGN_SUCCESS(code): pose = the
 *      result's, C = pose x odom_k^-1, both raw clouds inserted at the pose (inserted 1).
 *   6  otherwise the current pose becomes the initial pose, C stays and nothing is inserted (inserted 0).
 * The context's batch results stay as they were.  Results are final on return; the last insert may still be queued on
 * `stream`.  An initial pose that is not finite or whose translation has no voxel is LFX_ERR_INVALID_ARGUMENT. */
typedef struct lfx_rolling_map_result {
  lfx_align_result align;
  double initial_pose[12];
  uint32_t n_edge_map, n_surface_map;      /* points of the two boxes the scan was aligned against */
  int32_t aligned, inserted, recentered;
} lfx_rolling_map_result;
int lfx_rolling_map_update_batch(lfx_ctx *ctx, lfx_rolling_map *map, uint32_t n_scans, const double *odometry_poses /* host [n][12] or NULL */,
                                 lfx_rolling_map_result *results, void *stream);
/* The current pose: the pose of the last scan lfx_rolling_map_update_batch went through. */
int lfx_rolling_map_pose(const lfx_rolling_map *map, double pose[12]);

/* --- de-skew: the sensor's motion during a sweep taken out of the feature clouds ------------------------------------------ */
/* A spinning lidar reports every point in the sensor frame of its own firing time; everything above treats a scan as one
 * instant.  No reference counterpart (the reference has an unused imu_integration package beside its pipeline); the model
 * is LOAM's.  A sweep has a start time t0, an end time t1 != t0 and a MOTION D = [R_D | t_D] (3 x 4 row-major doubles): the
 * sensor frame at t1 expressed in the sensor frame at t0 (D = P0^-1 P1 for world poses P0, P1).  A point measured at time t
 * has alpha = (t - t0) * (1 / (t1 - t0)), not clamped; the sensor frame at alpha, in the frame at t0, is
 * M(alpha) = [Exp(alpha w) | alpha v], w = Log(R_D) (angle-axis vector), v = t_D: the rotation along the geodesic, the
 * translation linear.  M(1) = D.
 *   LFX_DESKEW_TO_START  p' = Exp(alpha w) p + alpha v
 *   LFX_DESKEW_TO_END    p' = R_D^T (Exp(alpha w) p + alpha v - t_D)
 * Arithmetic: double from the float record, unfused; theta and w as lfx_motion_twist gives them, k = w / theta,
 * a = alpha * theta, c = cos a, s = sin a, kxp = k x p, kdp = (kx px + ky py) + kz pz,
 * r = (p c + kxp s) + k (kdp (1 - c)); where theta < 1e-8 (zero included) r = p + alpha (w x p); m = r + alpha v; TO_START
 * rounds m once to float; TO_END takes u = m - t_D and rounds (R_D[0][i] u0 + R_D[1][i] u1) + R_D[2][i] u2 once to float.
 * The record's 4th float (the curvature) is copied.  A record whose alpha is not finite is copied unchanged. */
#define LFX_TIME_FROM_INDEX 0u   /* alpha = index / n_points of the scan: the records arrive in firing order */
#define LFX_TIME_FROM_FIELD 1u   /* t = (double)value * scale, read from the point record */
typedef struct lfx_time_field {
  uint32_t source;                 /* LFX_TIME_FROM_* */
  uint32_t offset;                 /* of the field inside a point record (FROM_FIELD) */
  uint32_t datatype;               /* LFX_FIELD_FLOAT32, LFX_FIELD_FLOAT64 or LFX_FIELD_UINT32 (FROM_FIELD) */
  uint32_t big_endian;
  double scale;                    /* seconds per unit of the field */
} lfx_time_field;
typedef struct lfx_sweep { double t0, t1; double motion[12]; } lfx_sweep;   /* t0, t1 unused with LFX_TIME_FROM_INDEX */
#define LFX_DESKEW_TO_START 0
#define LFX_DESKEW_TO_END 1
/* The time channel of a message's field list: the first field named t, time, timestamp, time_stamp or offset_time with
 * count 1.  FLOAT32 / FLOAT64 get scale 1.0 (seconds), UINT32 gets 1e-9 (nanoseconds: Ouster's t, Livox's offset_time).
 * LFX_ERR_NO_TIME_FIELD where there is none; LFX_ERR_UNSUPPORTED_FIELD for another datatype or a field past point_step.
 * Host only. */
int lfx_time_field_from_fields(const lfx_point_field *fields, uint32_t n_fields, uint32_t point_step, int is_bigendian,
                               lfx_time_field *out);
/* Motions, host only, no context, in lfx_pose_diff's arithmetic (every 3-term sum (a0 b0 + a1 b1) + a2 b2, unfused):
 *   lfx_motion_between  motion = pose0^-1 pose1 (the product lfx_pose_diff forms); two poses of equal values give the
 *                       identity itself (R^T R as it rounds is not), so that a sensor at rest changes no bit of a cloud
 *   lfx_motion_twist    w = Log(R_D) and theta = |w| as the de-skew kernel is given them: the quaternion of the matrix as
 *                       lfx_pose_diff states it (q_w = 0.5 sqrt(trace + 1) in the first branch, (m_kj - m_jk) * (0.5 / t) in
 *                       the second), n = |vec|, theta = 2 atan2(n, q_w), w = vec * (theta / n); n == 0: w = 0, theta = 0
 *   lfx_motion_scale    out = [Exp(ratio w) | ratio t_D] (a sweep shorter than the scan period), the rotation as the kernel
 *                       forms it: R = c I + s [k]x + (1 - c) k k^T with a = ratio * theta; theta < 1e-8: I + ratio [w]x */
int lfx_motion_between(const double pose0[12], const double pose1[12], double motion[12]);
int lfx_motion_twist(const double motion[12], double w[3], double *theta);
int lfx_motion_scale(const double motion[12], double ratio, double out[12]);
/* De-skew every edge and surface record of the last device batch, scan s by sweeps[s] (host, [n_scans]).  Outputs laid out
 * like lfx_device_view::edge_points / surface_points; BOTH NULL: in place, so that lfx_localize_batch,
 * lfx_odometry_update_batch, lfx_mapper_add, the lfx_pack_* calls and lfx_download_scan see de-skewed clouds.  The firing time
 * of a feature record comes from its edge_index / surface_index entry (the original index within the scan):
 * LFX_TIME_FROM_INDEX divides it by the scan's point count; LFX_TIME_FROM_FIELD reads the field from that record of the
 * batch's input points, which must still be alive (as for lfx_pack_colored).  Asynchronous on `stream`, one launch for the
 * batch, the counts read on the device.  LFX_ERR_INVALID_ARGUMENT: no batch yet, n_scans not the last batch's, NULL time /
 * sweeps, an unknown source / datatype / to, a field past the context's point_step, non-finite motion or times, t1 == t0
 * with LFX_TIME_FROM_FIELD, exactly one output NULL, outputs that are the context's own clouds (lfx_device_view::edge_points /
 * surface_points: NULL, NULL is the way to de-skew in place), and any de-skew of a batch that has already been de-skewed in
 * place (the next extraction lifts that). */
int lfx_deskew_batch(lfx_ctx *ctx, const lfx_time_field *time, const lfx_sweep *sweeps, uint32_t n_scans, int to,
                     float *d_edge_out, float *d_surface_out, void *stream);
/* lfx_odometry_update_batch with every scan corrected by its own constant-velocity prediction.  The odometry remembers the
 * poses of the last two scans its update* calls processed (lfx_odometry_add does not count).  Per scan of the last device
 * batch, in order: D = Pa^-1 Pb (lfx_motion_between; identity while fewer than two exist), the sweep's motion
 * lfx_motion_scale(D, sweep_ratio), the scan's two clouds de-skewed (as lfx_deskew_batch, out of place) into a buffer of
 * the odometry's own, then exactly lfx_odometry_update on those clouds (downsample after de-skew, align from the current
 * pose, append the de-skewed raw clouds).  sweep_times: host [n_scans][2] = t0, t1 per scan; NULL with LFX_TIME_FROM_INDEX.
 * The batch's clouds in the context stay raw.  Refused with LFX_ERR_INVALID_ARGUMENT: what lfx_odometry_update_batch and
 * lfx_deskew_batch refuse, a batch that has already been de-skewed in place (its clouds would be corrected twice), a
 * non-finite sweep_ratio, NULL sweep_times with LFX_TIME_FROM_FIELD. */
int lfx_odometry_update_batch_deskewed(lfx_ctx *ctx, lfx_odometry *odometry, const lfx_time_field *time,
                                       const double *sweep_times, double sweep_ratio, int to, uint32_t n_scans,
                                       lfx_odometry_result *results, void *stream);

/* De-skew along a TRAJECTORY: the sensor's poses within the sweep, as an IMU, a wheel odometer or a fused pose stream gives
 * them (10 - 40 per 0.1 s sweep), in place of one constant motion.
 * Model: between knots j and j + 1 the rotation runs along the geodesic and the position along the straight line.  With
 * beta = (t - times[j]) * (1 / (times[j+1] - times[j])) the pose is
 *   P(t) = [R_j Exp(beta Log(R_j^T R_{j+1})) | p_j + beta (p_{j+1} - p_j)].
 * The segment of a time t is j = clamp(#{knots with times[k] <= t} - 1, 0, n_knots - 2): a time on a knot belongs to the
 * segment that starts there; a time before the first knot extrapolates the first segment, one after the last knot the last
 * segment; beta is not clamped (as alpha is not).  A record measured at t becomes P(t_ref)^-1 P(t) p.
 * Arithmetic, host (lfx_trajectory_segments; the motion helpers' arithmetic, every 3-term sum (a0 b0 + a1 b1) + a2 b2,
 * unfused): P_ref is the knot's pose itself where t_ref equals a knot time, else with j, beta of t_ref
 *   P_ref = [R_j * rot(lfx_motion_scale(lfx_motion_between(P_j, P_{j+1}), beta)) | p_j + beta (p_{j+1} - p_j)];
 * Q_j = lfx_motion_between(P_ref, P_j) for every knot; per segment D_j = lfx_motion_between(Q_j, Q_{j+1}),
 * (w_j, theta_j) = lfx_motion_twist(D_j), k_j = w_j / theta_j (0 where theta_j < 1e-8), A_j the rotation of Q_j, q_j its
 * translation, dq_j = q_{j+1} - q_j.  A segment's row of the table, 24 doubles:
 *   [0..2] k_j   [3] theta_j   [4..6] w_j   [7..15] A_j row-major   [16..18] q_j   [19..21] dq_j   [22] times[j]
 *   [23] 1 / (times[j+1] - times[j])
 * Arithmetic, device, per record: double from the float record, unfused; r is the rotation step of the constant-motion
 * de-skew above with beta, k_j, theta_j, w_j (a = beta * theta_j, r = (p c + kxp s) + k (kdp (1 - c)); where
 * theta_j < 1e-8, r = p + beta (w_j x p));
 *   out_i = ((A_j[i][0] r0 + A_j[i][1] r1) + A_j[i][2] r2) + (q_j[i] + beta * dq_j[i]), rounded once to float.
 * The 4th float is copied.  A record whose time is not finite (its beta is not) is copied unchanged; with
 * LFX_TIME_FROM_FIELD and an index outside the scan nothing is read and the record is copied.
 * Consequence: with two knots and t_ref = times[0], Q_0 is the identity itself and the result equals
 * lfx_deskew_batch(..., LFX_DESKEW_TO_START) with motion = lfx_motion_between(P_0, P_1), t0 = times[0], t1 = times[1]
 * (times 0, 1 with LFX_TIME_FROM_INDEX), value for value. */
#define LFX_MAX_TRAJECTORY_KNOTS 64
#define LFX_TRAJECTORY_SEGMENT_DOUBLES 24
typedef struct lfx_trajectory {
  uint32_t n_knots;        /* 2 .. LFX_MAX_TRAJECTORY_KNOTS */
  const double *times;     /* host [n_knots], finite, strictly ascending: seconds with LFX_TIME_FROM_FIELD, fractions of
                              the sweep (index / n_points of the scan) with LFX_TIME_FROM_INDEX */
  const double *poses;     /* host [n_knots][12]: the sensor's pose at times[j], [R | t] row-major, all in ONE fixed frame */
  double t_ref;            /* the records are brought to the sensor frame at this time (same unit; may lie outside the knots) */
} lfx_trajectory;
/* Host only, no context: the table the kernel is given, [n_knots - 1][24] doubles in the order above.
 * LFX_ERR_INVALID_ARGUMENT: NULL arguments, n_knots outside 2 .. 64, NULL times / poses, times that are not finite or not
 * strictly ascending, a non-finite pose entry or t_ref. */
int lfx_trajectory_segments(const lfx_trajectory *trajectory, double *segments_out);
/* Host only: knots from gyro samples.  P_0 = identity; R_{j+1} = R_j E_j (3-term sums as above), E_j the rotation
 * lfx_motion_scale forms for the angle-axis vector phi = (0.5 * ((rate_j - bias) + (rate_{j+1} - bias))) * (t_{j+1} - t_j)
 * (theta = |phi| < 1e-8: I + [phi]x); p_j = velocity * (t_j - t_0) (constant, in the frame of the first sample).  bias and
 * velocity may be NULL (0).  LFX_ERR_INVALID_ARGUMENT: n < 2, NULL times / rates / poses_out, times that are not finite or
 * not strictly ascending, a non-finite rate, bias or velocity. */
int lfx_trajectory_from_gyro(const double *times, const double *rates /* [n][3] rad/s, sensor frame */, uint32_t n,
                             const double bias[3], const double velocity[3], double *poses_out /* [n][12] */);
/* lfx_deskew_batch along trajectories[s] (host, [n_scans]; the scans of one batch may have different knot counts): its
 * contract in every respect not named here.  Asynchronous on `stream`, one launch for the batch, the counts read on the
 * device; outputs laid out like the view's clouds, BOTH NULL: in place, which sets the same "already de-skewed in place"
 * mark (either de-skew call, lfx_odometry_update_batch_deskewed and lfx_odometry_update_batch_trajectory then refuse the
 * batch until the next extraction); the outputs may not be the context's own clouds.  Refused as well, with
 * LFX_ERR_INVALID_ARGUMENT and before anything is queued: what lfx_trajectory_segments refuses. */
int lfx_deskew_batch_trajectory(lfx_ctx *ctx, const lfx_time_field *time, const lfx_trajectory *trajectories /* host [n_scans] */,
                                uint32_t n_scans, float *d_edge_out, float *d_surface_out, void *stream);
/* lfx_odometry_update_batch_deskewed with the caller's trajectories in place of the prediction (a caller with a pose source
 * needs no seeding).  Per scan, in order: that scan alone de-skewed out of place (as lfx_deskew_batch_trajectory) into the
 * odometry's own de-skew buffers, then exactly lfx_odometry_update on those clouds.  The batch's clouds in the context stay
 * raw.  Refused: what lfx_odometry_update_batch and lfx_deskew_batch_trajectory refuse, and a batch that has already been
 * de-skewed in place.  Every trajectory of the batch is checked before the first scan is touched: a call refused for
 * trajectories[s], whichever s, has aligned and added nothing. */
int lfx_odometry_update_batch_trajectory(lfx_ctx *ctx, lfx_odometry *odometry, const lfx_time_field *time,
                                         const lfx_trajectory *trajectories, uint32_t n_scans,
                                         lfx_odometry_result *results, void *stream);

/* --- place recognition: scan-context descriptors and a place index ----------------------------------------------------- */
/* "Where am I in this map?"  No reference counterpart; the model is Scan Context (Kim and Kim, IROS 2018): a scan gives one
 * R x S matrix, the largest height in every polar cell around the sensor; two matrices are compared under every column
 * shift, and the best shift is the yaw between the two visits.  The index below compares a query with EVERY entry (no
 * KD-tree prefilter).
 *
 * Tables (lfx_scan_context_tables, host only, the ONLY source: the device is given exactly these values):
 *   sector_cos[m], sector_sin[m] = cos, sin of -pi + (2 pi) * m / S in double, the angle formed as
 *                                  -M_PI + ((2.0 * M_PI) * (double)m) / (double)S;
 *   ring_r2[j] = e * e with e = ((double)max_radius * (double)j) / (double)R, j = 0 .. R.
 * Per record (x, y, z read as floats through the context's lfx_layout: any point_step, offsets, byte order), in double,
 * unfused:
 *   - a record with a non-finite x, y or z is skipped;
 *   - r2 = x*x + y*y (the products of two floats are exact in double); a record with r2 < min_radius^2 (the square of the
 *     float in double, exact) or r2 >= ring_r2[R] is skipped -- with min_radius > 0 that leaves the (0, 0, 0) records out;
 *   - ring = #{ j in 1 .. R-1 : r2 >= ring_r2[j] };
 *   - cross_m = sector_cos[m]*y - sector_sin[m]*x: two rounded products and one subtraction (a fused form gives other bits);
 *     where y >= 0 (-0.0 included): sector = S/2 + #{ m in S/2+1 .. S-1 : cross_m >= 0 },
 *     otherwise:                    sector = #{ m in 1 .. S/2-1 : cross_m >= 0 }.
 *     The counts are the definition; no atan2 is involved (sector m covers the azimuths [-pi + 2 pi m / S, -pi + 2 pi (m+1) / S)).
 * Cell [ring][sector] holds zmax, the largest z of its records (float order; -0.0 and +0.0 give the same cell value); the
 * value written is v = zmax + sensor_height in float where v > 0, else +0.0f; a cell without a record is +0.0f. */
typedef struct lfx_scan_context_config {
  uint32_t n_rings;      /* R, radial cells: 20;  1 .. 40            */
  uint32_t n_sectors;    /* S, azimuth cells: 60; even, 4 .. 120     */
  float max_radius;      /* 80.0  */
  float min_radius;      /* 0.1; >= 0, < max_radius */
  float sensor_height;   /* 2.0: added to z so that the ground is near 0 */
} lfx_scan_context_config;
#define LFX_SCAN_CONTEXT_MAX_RINGS 40
#define LFX_SCAN_CONTEXT_MAX_SECTORS 120
void lfx_scan_context_default_config(lfx_scan_context_config *config);
/* host only, no context: the tables the kernel is given.  LFX_ERR_INVALID_ARGUMENT: NULL arguments, R or S out of range, S
 * odd, radii that are not finite, negative or not min_radius < max_radius, a non-finite sensor_height. */
int lfx_scan_context_tables(const lfx_scan_context_config *config, double *sector_cos /*[S]*/, double *sector_sin /*[S]*/,
                            double *ring_r2 /*[R+1]*/);
/* Descriptors of every scan of the last device batch, from the batch's INPUT records (which must still be alive, as for
 * lfx_pack_colored): d_desc_out [n_scans][R][S] floats, row = ring.  Every cell is written on every call.  Asynchronous on
 * `stream`, the counts read on the device.  LFX_ERR_INVALID_ARGUMENT: NULL arguments, what lfx_scan_context_tables refuses,
 * no batch yet, n_scans not the last batch's, the batch's input records not known. */
int lfx_scan_context_batch(lfx_ctx *ctx, const lfx_scan_context_config *config, uint32_t n_scans, float *d_desc_out, void *stream);

/* The place index: descriptors of one config on the device, in insertion order, each with its column norms (computed once,
 * at the add).  Distance of a query q and an entry c under the column shift s, in double:
 *   nq[j] = sqrt(sum_i q[i][j]^2), summed in the order i = 0 .. R-1 (nc the same for the entry);
 *   g(j, s) = sum_i q[i][j] * c[i][(j + s) mod S], in the same order (the products are exact in double);
 *   a column pair j counts where nq[j] > 0 and nc[(j + s) mod S] > 0;
 *   d(s) = 1 - (sum_j g(j, s) / (nq[j] * nc[(j + s) mod S])) / n_valid, j ascending over the pairs that count; no pair: 1.
 * The entry's distance is the least d(s), its shift the lowest s that reaches it; yaw = shift * (2 pi / S) for
 * shift <= S / 2, (shift - S) * (2 pi / S) above: in (-pi, pi].  CONVENTION: a sensor that revisits the entry's place turned
 * by +yaw about z (counter-clockwise seen from above) gives this shift; the initial pose of the revisit is the entry's pose
 * times Rz(yaw).  Matches come in ascending distance, equal distances by the lower entry: the same inputs give the same
 * bytes.  Descriptors must be finite (what lfx_scan_context_batch writes is); an entry whose distance to a query is NaN is
 * never a match.  An index belongs to the device of the context that made it. */
typedef struct lfx_place_db lfx_place_db;
typedef struct lfx_place_match { uint32_t entry; uint32_t shift; double distance; double yaw; } lfx_place_match;
#define LFX_PLACE_MAX_MATCHES 16
int lfx_place_db_create(lfx_ctx *ctx, const lfx_scan_context_config *config, uint32_t capacity, lfx_place_db **out);
void lfx_place_db_destroy(lfx_place_db *db);
/* Appends n descriptors ([n][R][S] floats) from the device / from the host; entry = insertion order.  Beyond the capacity:
 * LFX_ERR_CAPACITY, the index unchanged.  Queued on `stream`; a query on another stream is ordered behind the last add. */
int lfx_place_db_add(lfx_ctx *ctx, lfx_place_db *db, const float *d_desc, uint32_t n, void *stream);
int lfx_place_db_add_host(lfx_ctx *ctx, lfx_place_db *db, const float *desc, uint32_t n, void *stream);
int lfx_place_db_size(const lfx_place_db *db, uint32_t *n);
/* Entries first .. first + count - 1 to host memory ([count][R][S] floats).  Synchronous. */
int lfx_place_db_download(lfx_ctx *ctx, const lfx_place_db *db, uint32_t first, uint32_t count, float *desc_out /*host*/, void *stream);
/* For each of n_queries descriptors on the device, the k (1 .. 16) best of entries [first, first + count): matches host
 * [n_queries][k].  first / count let a loop-closure caller leave out its most recent keyframes; count may be 0.  With fewer
 * than k entries in the range the remaining matches are entry = UINT32_MAX, shift = 0, distance = +inf, yaw = 0.
 * Synchronous.  LFX_ERR_INVALID_ARGUMENT: NULL arguments, n_queries 0, k outside 1 .. 16, a range past the index's size. */
int lfx_place_db_query(lfx_ctx *ctx, const lfx_place_db *db, const float *d_desc, uint32_t n_queries, uint32_t first,
                       uint32_t count, uint32_t k, lfx_place_match *matches, void *stream);
/* The same query with a gate of its own per query, decided on the device: entry e is ELIGIBLE for query q iff
 * e < gates[q].limit and it passes the position test (dx*dx + dy*dy) + dz*dz <= radius*radius, d = the translation of
 * d_poses[e] minus the translation of d_poses[gates[q].pose], all in double, unfused, in that order -- the rule and the
 * arithmetic of lfx_keyframes_submap's selection.  The test is skipped (every e < limit is eligible) where d_poses is NULL or
 * gates[q].pose == LFX_PLACE_NO_POSE; a radius of +inf passes every finite pose.  d_poses: device, [.][12] doubles as the
 * keyframe store and the pose graph keep them, entry e's pose at d_poses[e]; it must hold every entry below the largest
 * limit and every gates[q].pose, and is read on `stream`.  matches [n_queries][k]: the k best ELIGIBLE entries, each with
 * exactly the (entry, shift, distance, yaw) lfx_place_db_query gives for that pair, ascending distance, equal distances by
 * the lower entry; slots beyond the eligible entries are UINT32_MAX, 0, +inf, 0.  n_eligible (may be NULL) [n_queries]: the
 * eligible entries of each query.  Distance work is done for eligible pairs only: a gate pass writes each query's eligible
 * entries in ascending order (a fixed order: the same inputs give the same list), the comparison and the selection run
 * over those lists, whose lengths stay on the device and nothing waits before the final copy.  The comparison's launch is
 * sized from the largest limit: without poses a workgroup to each tile of it, as lfx_place_db_query's; with poses at most
 * about 8 192 workgroups in all, each walking every n-th tile of one pass up to its list's end.  Synchronous; ordered behind the index's last add.  LFX_ERR_INVALID_ARGUMENT, before anything is queued:
 * NULL ctx, db, d_desc, gates or matches, n_queries outside 1 .. 65535, k outside 1 .. 16, a limit above the index's size, a
 * radius that is NaN or negative. */
#define LFX_PLACE_NO_POSE 0xFFFFFFFFu
typedef struct lfx_place_gate { uint32_t limit; uint32_t pose; } lfx_place_gate;
int lfx_place_db_query_gated(lfx_ctx *ctx, const lfx_place_db *db, const float *d_desc, uint32_t n_queries,
                             const lfx_place_gate *gates /* host [n_queries] */,
                             const double *d_poses /* device [.][12]; entry e's pose is d_poses[e]; may be NULL */,
                             double radius, uint32_t k, lfx_place_match *matches /* host [n_queries][k] */,
                             uint32_t *n_eligible /* host [n_queries], may be NULL */, void *stream);

/* --- segmentation: ground, clusters and clutter from a range image; feature clouds filtered by it ----------------------- */
/* "Is this feature on the road, on an object, or on a leaf?"  No reference counterpart; the model is LeGO-LOAM's image
 * projection (Shan and Englot, IROS 2018): the sweep becomes an H x W range image, the ground is found by the slope between
 * vertically adjacent cells, the rest is clustered by connected components under an angle test, and clusters too small to be
 * objects are clutter.  Edge features are then taken from clusters only, surface features from the ground and from clusters
 * (lfx_pack_features_segmented).
 *
 * Tables (lfx_segment_tables, host only, the ONLY source: the device is given exactly these values):
 *   col_cos[m], col_sin[m] = cos, sin of -M_PI + ((2.0 * M_PI) * (double)m) / (double)W, m = 0 .. W-1;
 *   consts = sin, cos of (2.0 * M_PI) / (double)W (the angle between adjacent columns), then sin, cos of (double)row_step.
 * All arithmetic below is in double, unfused, on the floats read through the context's lfx_layout.
 *
 * Projection.  Record i of a scan (i: its index in the scan's input):
 *   - skipped if x, y or z is not finite, or if its row -- its ring slot as the extraction defines it: the ring id, with
 *     lfx_config.ring_ids / lfx_set_ring_ids the id's rank -- is >= H or unknown to the context;
 *   - skipped if x*x + y*y == 0;
 *   - r = sqrt((x*x + y*y) + z*z); skipped if r < (double)min_range or r >= (double)max_range (the (0, 0, 0) records go here
 *     at the latest);
 *   - column: m0 = y >= 0.0f ? W/2 : 0;  cross(m) = col_cos[m]*y - col_sin[m]*x (two rounded products, one subtraction);
 *       lo = 0, hi = W/2 - 1; while (lo < hi) { mid = (lo + hi + 1) >> 1; if (cross(m0 + mid) >= 0) lo = mid; else hi = mid - 1; }
 *     column = m0 + lo.  The bisection is the definition; no atan2 is involved.
 *   Cell (row, column) is won by the record with the least (float)r, equal floats by the lower i; the cell has that record's
 *   x, y, z and r.  A cell without a record is empty.
 * Ground.  For a column c and a row i, ground_first_row <= i < ground_last_row, with (i, c) and (i+1, c) both occupied:
 *   dx, dy, dz the differences of the floats in double; if dz*dz <= g2 * (dx*dx + dy*dy), g2 = (double)ground_tan *
 *   (double)ground_tan, both cells are ground.  (A sensor whose ring 0 is the top beam gives the upper slots.)
 * Clusters.  Nodes: the occupied cells that are not ground.  Edges: (row, c) - (row, (c+1) mod W) with the column step's sin
 *   and cos -- the seam pair (W-1, 0) counts once -- and (row, c) - (row+1, c) with the row step's.  An edge joins its cells
 *   iff d2 * sin_a > (double)segment_tan * (d1 - d2 * cos_a), d1 = max(r_a, r_b), d2 = min(r_a, r_b).  A cell's LABEL is the
 *   least cell index row * W + column of its connected component.  A component is a SEGMENT if its size is >=
 *   segment_min_points, or if its size is >= small_min_points and row_max - row_min + 1 >= small_min_rows; otherwise CLUTTER.
 * Per record: a skipped record is LFX_SEG_NONE; every other record takes the class of its cell, whether or not it won the
 *   cell; its id is the cell's label for LFX_SEG_SEGMENT and LFX_SEG_CLUTTER, 0xFFFFFFFF for LFX_SEG_NONE and LFX_SEG_GROUND.
 * Every output byte is the same whatever the schedule. */
#define LFX_SEG_NONE 0
#define LFX_SEG_GROUND 1
#define LFX_SEG_SEGMENT 2
#define LFX_SEG_CLUTTER 3
#define LFX_SEG_EDGE_MASK_DEFAULT (1u << LFX_SEG_SEGMENT)
#define LFX_SEG_SURFACE_MASK_DEFAULT ((1u << LFX_SEG_GROUND) | (1u << LFX_SEG_SEGMENT))
#define LFX_SEGMENT_MAX_ROWS 128
#define LFX_SEGMENT_MAX_COLUMNS 4096
typedef struct lfx_segment_config {
  uint32_t n_rows;              /* H: 16; 1 .. 128, at most the context's max_rings */
  uint32_t n_columns;           /* W: 1800; even, 4 .. 4096 */
  float row_step;               /* 0.034906585 (2 degrees): radians between adjacent rows; > 0, finite */
  float min_range, max_range;   /* 1.0, 100.0; 0 < min_range < max_range, finite */
  uint32_t ground_first_row, ground_last_row;   /* 0, 7; first <= last < H: the pairs (i, i+1), first <= i < last, are tested */
  float ground_tan;             /* 0.17632698 (tan 10 degrees); >= 0, finite */
  float segment_tan;            /* 1.7320508 (tan 60 degrees); > 0, finite */
  uint32_t segment_min_points;  /* 30; >= 1 */
  uint32_t small_min_points, small_min_rows;    /* 5, 3; >= 1 */
} lfx_segment_config;
void lfx_segment_default_config(lfx_segment_config *config);
/* host only, no context: the tables the kernels are given.  LFX_ERR_INVALID_ARGUMENT: NULL arguments and every field outside
 * the ranges above. */
int lfx_segment_tables(const lfx_segment_config *config, double *col_cos /*[W]*/, double *col_sin /*[W]*/, double consts[4]);
/* Class and id of every input record of every scan of the last device batch, from the batch's INPUT records (which must
 * still be alive, as for lfx_scan_context_batch).  d_class_out (u8) and d_id_out (u32, may be NULL) are addressed by
 * scan_begin[s] + i with the view's scan_begin; d_counts_out (may be NULL) u32 [n_scans][4], the scan's records by class.
 * Every element of every scan is written on every call.  Asynchronous on `stream`, the counts read on the device.  The
 * images live in a workspace of the context that grows on demand up to LFX_SEGMENT_BUDGET_CELLS cells; a batch whose images
 * exceed that is processed in chunks of whole scans, in stream order (calls on different streams are ordered one behind the
 * other: they share the workspace).  LFX_ERR_INVALID_ARGUMENT, before anything is queued: NULL ctx, config or d_class_out,
 * what lfx_segment_tables refuses, n_rows above the context's max_rings, no batch yet, n_scans not the last batch's, the
 * batch's input records not known (a defensive check: every entry point that runs a batch records where its records lie, so
 * no sequence of calls reaches it today).  The call never waits for `stream`: the tables of the configs seen last are kept
 * on the device, and a new config's go up from a pinned block of their own. */
#define LFX_SEGMENT_BUDGET_CELLS (1u << 24)
int lfx_segment_batch(lfx_ctx *ctx, const lfx_segment_config *config, uint32_t n_scans, uint8_t *d_class_out,
                      uint32_t *d_id_out, uint32_t *d_counts_out, void *stream);
/* lfx_pack_features with a filter: a feature record is kept iff bit (1 << class) of its ORIGINAL point (the view's
 * edge_index / surface_index into d_class, which lfx_segment_batch wrote for this batch) is set in its cloud's mask; the order
 * is kept.  The same [2][batch+1] offsets table (of what is kept), the same rule for a short capacity_points, the same cap at
 * 2^32 - 1.  d_counts_out (may be NULL) u32 [2][batch]: the kept records per scan, so that (d_offsets_out, d_counts_out,
 * count_stride 1) -- for the surface cloud (d_offsets_out + batch + 1, d_counts_out + batch, 1) -- are the (d_begin, d_count)
 * of lfx_mapper_add and lfx_rolling_map_insert.  LFX_ERR_INVALID_ARGUMENT: NULL arguments, no batch yet, a mask with a bit
 * above 3. */
int lfx_pack_features_segmented(lfx_ctx *ctx, const uint8_t *d_class, uint32_t edge_mask, uint32_t surface_mask,
                                float *d_edge_out, float *d_surface_out, uint32_t *d_offsets_out, uint32_t *d_counts_out,
                                size_t capacity_points, void *stream);

/* --- pose graph: past poses corrected by loop closures, optimised on the device ------------------------------------------ */
/* The problem.  NODE k: a pose [R | t], 12 doubles row-major.  Its increment is delta = (a, b), ordered as
 * lfx_align_report.information orders it: R <- R Exp(a), t <- t + b -- the rotation first and in the node's own frame, the
 * translation in the world frame.  Node 0 is fixed unless lfx_pose_graph_release_first frees it (PRIORS, below); others may
 * be flagged fixed (lfx_pose_graph_set_fixed).
 * EDGE (i, j, Z = [R_Z | t_Z], Omega 6 x 6 row-major symmetric positive definite, flags): Z measures T_i^-1 T_j.  Its residual
 * r = (phi, t_E):
 *   R_E = R_Z^T R_i^T R_j,  d = R_i^T (t_j - t_i),  t_E = R_Z^T (d - t_Z),  phi = Log(R_E)
 *   Log: v = (R21 - R12, R02 - R20, R10 - R01) / 2, theta = atan2(|v|, (trace - 1) / 2), phi = v theta / |v|, and phi = v
 *   where |v| < 1e-10.  Valid for theta < 3 rad; phi's rounding error grows as 1 / sin theta beyond a right angle (against a
 *   50-digit reference, in spacings of the largest term summed on the way to r: 0.8 up to 2.5 rad, 3 at 2.9, 1.8 at 2.99).
 * Its Jacobians dr / d delta_i and dr / d delta_j, with Jri = J_r^-1(phi) = I + [phi]x / 2 + c [phi]x^2,
 * c = 1 / theta^2 - (1 + cos theta) / (2 theta sin theta), c = 1 / 12 + theta^2 / 720 for theta < 1e-4:
 *   A_j = [[Jri, 0], [0, R_Z^T R_i^T]]      A_i = [[-Jri R_j^T R_i, 0], [R_Z^T [d]x, -R_Z^T R_i^T]]
 * COST chi^2 = sum of rho_e.  An edge without LFX_EDGE_ROBUST has rho = r^T Omega r and weight w = 1.  With the flag, Huber
 * on s = sqrt(r^T Omega r) with the config's huber_delta: s <= delta has rho = s^2, w = 1; beyond it rho = 2 delta s -
 * delta^2, w = delta / s.  Omega enters the normal equations as w Omega.
 * ITERATION: Gauss-Newton, (H + lambda I) delta = -g over the free nodes (H = sum A^T w Omega A, g = sum A^T w Omega r), then
 * the increment above; lambda = damping.  It stops when max |delta| < tolerance or after max_iter steps.  If the final chi^2
 * exceeds the initial one (by more than its rounding, 1e-12 max(1, chi^2): a consistent graph starts and ends at 1e-30),
 * or is not a number, the initial poses are restored: LFX_POSE_GRAPH_DIVERGED.  Rotations stay
 * orthonormal, |R^T R - I| <= 1e-12 after any number of iterations: every step re-orthonormalises the rotation it moved,
 * R <- R (3 I - R^T R) / 2 (one step of the polar iteration; no quaternion is kept).  A node whose increment is exactly 0
 * (no edge and no prior touches it) is not moved: its pose stays as it is, byte for byte.
 * THE SOLVER: the chain is the first edge with j == i + 1 for each i; every other edge is a loop edge --
 * backward edges, duplicates and edges between distant nodes among them.  P = lambda I + the chain edges' blocks is block-
 * tridiagonal in node order (a fixed node has the identity and no coupling); with J the loop edges' rows H = P + J^T W J, and
 * the step is exact: y0 = P^-1 (-g), Y = P^-1 J^T, S = W^-1 + J Y, delta = y0 - Y S^-1 (J y0), S formed and factored in the
 * rows whitened by the loop edges' information.  A missing chain edge leaves P block-diagonal there; lambda and the loops
 * hold it.  A pivot that is not positive (an information matrix that is not positive definite) refuses the call:
 * LFX_POSE_GRAPH_NOT_POSITIVE_DEFINITE, the poses untouched.  No floating-point atomic is used: the same graph gives the
 * same bytes, however its edges were split over calls of lfx_pose_graph_add_edges. */
#define LFX_EDGE_ROBUST 1u
#define LFX_POSE_GRAPH_CONVERGED 0              /* max |delta| < tolerance                                   */
#define LFX_POSE_GRAPH_MAX_ITERATIONS 1         /* max_iter steps taken, the last one not below the tolerance */
#define LFX_POSE_GRAPH_DIVERGED 2               /* the initial poses were restored                           */
#define LFX_POSE_GRAPH_NOT_POSITIVE_DEFINITE 3  /* the poses are untouched                                   */
#define LFX_POSE_GRAPH_MAX_LOOP_EDGES 10000u
typedef struct lfx_pose_graph lfx_pose_graph;
typedef struct lfx_pose_graph_config {
  uint32_t max_nodes;        /* >= 1 */
  uint32_t max_edges;        /* >= 1 */
  uint32_t max_loop_edges;   /* 512; <= LFX_POSE_GRAPH_MAX_LOOP_EDGES.  The workspace holds 6 max_nodes (6 max_loop_edges + 1) doubles */
  uint32_t max_iter;         /* 10; 1 .. 1000 */
  double damping;            /* 1e-6; >= 0, finite */
  double tolerance;          /* 1e-9; >= 0, finite */
  double huber_delta;        /* 3.0; > 0, finite */
} lfx_pose_graph_config;
typedef struct lfx_pose_graph_edge {
  uint32_t i, j;             /* i != j, both nodes of the graph */
  uint32_t flags;            /* 0 or LFX_EDGE_ROBUST */
  uint32_t reserved;         /* 0 */
  double z[12];              /* Z = T_i^-1 T_j (lfx_motion_between(pose_i, pose_j)) */
  double information[36];    /* Omega, symmetric to 1e-9 of its largest entry */
} lfx_pose_graph_edge;
typedef struct lfx_pose_graph_result {
  int32_t code;              /* LFX_POSE_GRAPH_* */
  int32_t iterations;        /* steps taken */
  double chi2_initial, chi2_final, max_step;   /* max_step: max |delta| of the last step */
  uint32_t n_chain, n_loop, n_robust_downweighted;   /* edges with w < 1 at the final poses */
  uint32_t reserved;
} lfx_pose_graph_result;
typedef struct lfx_pose_graph_info_t {
  uint32_t n_nodes, n_edges, n_chain, n_loop;   /* n_chain / n_loop: of the edges added so far */
  uint64_t device_bytes;                        /* everything lfx_pose_graph_create allocated on the device */
} lfx_pose_graph_info_t;
/* max_nodes = max_edges = 0 (the caller sets both), max_loop_edges 512, max_iter 10, damping 1e-6, tolerance 1e-9, huber_delta 3 */
void lfx_pose_graph_default_config(lfx_pose_graph_config *config);
/* Allocates everything the graph will ever use; no later call allocates device memory.  A config outside the ranges above is
 * LFX_ERR_INVALID_ARGUMENT, a failed allocation LFX_ERR_OUT_OF_MEMORY with nothing left allocated. */
int lfx_pose_graph_create(lfx_ctx *ctx, const lfx_pose_graph_config *config, lfx_pose_graph **out);
void lfx_pose_graph_destroy(lfx_pose_graph *graph);
int lfx_pose_graph_info(const lfx_pose_graph *graph, lfx_pose_graph_info_t *info);
/* n poses on the host ([n][12]) appended as nodes; *first_id (may be NULL) = the id of the first.  A pose that is not finite is
 * LFX_ERR_INVALID_ARGUMENT, more nodes than max_nodes LFX_ERR_CAPACITY: nothing changed, nothing queued. */
int lfx_pose_graph_add_nodes(lfx_ctx *ctx, lfx_pose_graph *graph, const double *poses, uint32_t n, uint32_t *first_id, void *stream);
/* Node `node` held where it is (fixed != 0) or free again.  Node 0 stays fixed whatever is asked, unless
 * lfx_pose_graph_release_first released it: then it is held or free as asked here. */
int lfx_pose_graph_set_fixed(lfx_ctx *ctx, lfx_pose_graph *graph, uint32_t node, int fixed, void *stream);
/* n edges on the host appended.  Checked before anything is touched: i == j, an id that is not a node, flags beyond
 * LFX_EDGE_ROBUST, Z or Omega not finite, Omega not symmetric are LFX_ERR_INVALID_ARGUMENT; more edges than max_edges, or more
 * loop edges than max_loop_edges, LFX_ERR_CAPACITY. */
int lfx_pose_graph_add_edges(lfx_ctx *ctx, lfx_pose_graph *graph, const lfx_pose_graph_edge *edges, uint32_t n, void *stream);
/* Gauss-Newton to the config's tolerance; synchronous (the host reads one small record per iteration).  Returns LFX_OK
 * whenever the optimiser ran, whatever result->code says; a graph with neither edges nor priors is LFX_ERR_INVALID_ARGUMENT
 * (priors alone are enough).  Ordered behind
 * every earlier call on this graph, whichever streams they used. */
int lfx_pose_graph_optimize(lfx_ctx *ctx, lfx_pose_graph *graph, lfx_pose_graph_result *result, void *stream);
/* Nodes first .. first + count - 1 copied to the host ([count][12]); synchronous. */
int lfx_pose_graph_poses(lfx_ctx *ctx, const lfx_pose_graph *graph, uint32_t first, uint32_t count, double *poses_out, void *stream);
/* The same range overwritten from the host (a new initial guess; poses that are not finite are refused). */
int lfx_pose_graph_set_poses(lfx_ctx *ctx, lfx_pose_graph *graph, uint32_t first, uint32_t count, const double *poses, void *stream);
/* The poses where they live: *d_poses = [n_nodes][12] doubles on the device.  The ADDRESS is valid until the graph is
 * destroyed.  The CONTENTS are current behind `stream` once the graph's earlier calls have passed (the call queues that wait
 * on `stream`), and stay so until the next call that writes the graph (add_nodes, set_poses, optimize): nothing orders that
 * call behind the caller's reads, so the reader must have finished, or must order the writing call's stream behind its own
 * work itself, before the graph is written again.  What a map rebuild from corrected poses reads. */
int lfx_pose_graph_view(lfx_ctx *ctx, const lfx_pose_graph *graph, const double **d_poses, uint32_t *n_nodes, void *stream);
/* Per edge, at the poses the last lfx_pose_graph_optimize left: rho[e] and w[e] (either may be NULL), first .. first + count - 1.
 * A false loop closure under LFX_EDGE_ROBUST shows as the smallest w.  LFX_ERR_INVALID_ARGUMENT before the first optimise or
 * when nodes, edges or poses were written since. */
int lfx_pose_graph_edge_chi2(lfx_ctx *ctx, const lfx_pose_graph *graph, uint32_t first, uint32_t count, double *rho, double *w, void *stream);
/* An alignment report's information (lfx_align_report.information: a in the scan's frame, b in the map frame) in an edge's
 * residual coordinates: Omega = B H B^T, B = blkdiag(I, R_j^T), pose_j the scan's pose the report was made at.  Host only;
 * every sum of three terms is (a0 b0 + a1 b1) + a2 b2.  out may be report_information. */
int lfx_pose_graph_edge_information(const double pose_j[12], const double report_information[36], double out[36]);

/* PRIORS: unary terms, each on one node -- an absolute fix (GNSS, a surveyed marker, a pose from lfx_localize_batch against an
 * older map).  A prior adds A^T w Omega A to its node's diagonal block of P and A^T w Omega r to its gradient, nothing else:
 * the chain factor, the chain solve, S and the step are as above, the cost is O(priors) and does not grow with the loop edges.
 * POSE PRIOR (Z = [R_Z | t_Z], Omega 6 x 6): Z measures T_node.  By definition the edge (i, node, Z, Omega) with T_i the
 * identity, through the same device routine as an edge's r and A_j:
 *   R_E = R_Z^T R_k,  t_E = R_Z^T (t_k - t_Z),  phi = Log(R_E),  r = (phi, t_E),  A = [[Jri, 0], [0, R_Z^T]]
 * POSITION PRIOR (LFX_PRIOR_POSITION; t_Z, Omega_t 3 x 3 symmetric positive semi-definite, lever l): t_Z measures the world
 * position of the point l of the node's frame (an antenna metres from the lidar; with l != 0, positions alone make the heading
 * observable):
 *   r = (0, 0, 0, t_k + R_k l - t_Z)  in the world frame,  A = [[0, 0], [-R_k [l]x, I]]
 * every sum of three terms (a0 b0 + a1 b1) + a2 b2.  Omega_t is the lower right 3 x 3 of `information`.
 * COST AND WEIGHTS as an edge's: rho = r^T Omega r; with LFX_PRIOR_ROBUST Huber on s = sqrt(r^T Omega r) with the config's
 * huber_delta, Omega entering as w Omega.  chi2_initial and chi2_final are the sum over edges and priors.  A prior on a fixed
 * node counts in chi^2 and in nothing else.  A prior whose Omega is indefinite shows as a chain pivot that is not positive:
 * LFX_POSE_GRAPH_NOT_POSITIVE_DEFINITE, the poses untouched.  A node that no edge touches but a prior does moves to its prior.
 * lfx_pose_graph_result and lfx_pose_graph_info_t do not know priors: n_robust_downweighted counts edges only
 * (lfx_pose_graph_prior_info has the priors').  A graph without priors computes, byte for byte, what it computed before priors
 * existed; a graph with priors gives the same bytes however its priors and edges were split and interleaved over calls. */
#define LFX_PRIOR_ROBUST   1u   /* Huber with the graph's huber_delta, as LFX_EDGE_ROBUST */
#define LFX_PRIOR_POSITION 2u   /* a position fix; without it a full pose */
typedef struct lfx_pose_graph_prior {
  uint32_t node, flags;
  double z[12];              /* pose: Z = [R_Z | t_Z] measures T_node.  position: only t_Z (z[3], z[7], z[11]) is read */
  double information[36];    /* pose: Omega 6 x 6, checked as an edge's.  position: its lower right 3 x 3, the rest must be 0 */
  double lever[3];           /* position: the antenna in the node's frame; pose: must be 0 */
} lfx_pose_graph_prior;      /* 416 bytes */
typedef struct lfx_pose_graph_prior_info_t {
  uint32_t n_priors, max_priors;   /* added so far; reserved by lfx_pose_graph_reserve_priors (0: nothing reserved) */
  uint32_t n_downweighted;         /* priors with w < 1 at the poses the last lfx_pose_graph_optimize left */
  uint32_t reserved;               /* 0 */
  double chi2;                     /* the priors' share of that optimise's chi2_final */
} lfx_pose_graph_prior_info_t;
/* Room for max_priors priors: the priors, their linearisation and the per-node lists.  Called once, before the first prior.
 * lfx_pose_graph_config cannot grow (lfx_loop_closer_result embeds the graph's structs), so the capacity comes through this
 * call: the one exception to "no later call allocates"; lfx_pose_graph_info's device_bytes grows by what was allocated.  A
 * second call, or max_priors == 0, is LFX_ERR_INVALID_ARGUMENT; a failed allocation LFX_ERR_OUT_OF_MEMORY, the graph as it was. */
int lfx_pose_graph_reserve_priors(lfx_ctx *ctx, lfx_pose_graph *graph, uint32_t max_priors);
/* n priors on the host appended.  Checked before anything is touched: a node that is not in the graph, unknown flags, a value
 * that is not finite, Omega not symmetric (an edge's rule: 1e-9 of its largest entry), a position prior with information outside
 * its block, a pose prior with a lever are LFX_ERR_INVALID_ARGUMENT; more priors than reserved LFX_ERR_CAPACITY (nothing
 * reserved: a capacity of 0). */
int lfx_pose_graph_add_priors(lfx_ctx *ctx, lfx_pose_graph *graph, const lfx_pose_graph_prior *priors, uint32_t n, void *stream);
/* released != 0: node 0 is free from now on, unless lfx_pose_graph_set_fixed(0, 1) says otherwise; released == 0: fixed again
 * whatever is asked.  A graph that never calls this behaves as described above, set_fixed(0, 0) included.  A free first node
 * lets measurements turn and shift the trajectory as a whole; without a prior (or a loop to a fixed node) nothing but lambda
 * holds it, and what the optimiser then returns is the caller's affair. */
int lfx_pose_graph_release_first(lfx_ctx *ctx, lfx_pose_graph *graph, int released, void *stream);
/* Per prior, as lfx_pose_graph_edge_chi2 per edge, with the same refusals (before the first optimise; after nodes, edges,
 * priors or poses were written since).  An outlier fix under LFX_PRIOR_ROBUST shows as the smallest w. */
int lfx_pose_graph_prior_chi2(lfx_ctx *ctx, const lfx_pose_graph *graph, uint32_t first, uint32_t count, double *rho, double *w, void *stream);
int lfx_pose_graph_prior_info(const lfx_pose_graph *graph, lfx_pose_graph_prior_info_t *info);

/* COVARIANCES: how well the optimised nodes are known.  H is the matrix of the solver's last linearisation, sum A^T w Omega A
 * over edges and priors with the Huber weights at the poses the last lfx_pose_graph_optimize left, and
 *   Sigma = (H + lambda I)^-1  over the free nodes, lambda the config's damping:
 * the matrix the solver factors, nothing else.  It is over the node increments (a, b) as ordered above -- a the rotation in
 * the node's own frame, b the translation in the world frame, lfx_align_report.information's ordering -- so
 * lfx_align_covariance_ros(pose_k, Sigma_kk, out) applies to a node's marginal unchanged.  A node nothing constrains has
 * Sigma_kk = I / lambda.  A fixed node has no increment: every block of Sigma in its row or column is exactly 0.0 (not the
 * identity P carries there).  Sigma is as good as the Omega that were fed: nothing is rescaled by chi^2 / dof.
 * HOW: with H + lambda I = P + Jt^T Jt as in THE SOLVER, Sigma = P^-1 - V V^T, V = Y L_S^-T, S = I + Jt Y = L_S L_S^T;
 * (P^-1)(k, k) and the blocks beside it come from the selected inverse of the chain factor.  All FP64, no floating-point
 * atomic, every sum in a fixed order: the same graph gives the same bytes, however its edges were split over calls, whichever
 * stream is used, whatever range or pairs are asked for.  Cost: the solve for V is (6 L)^2 / 2 * 6 N multiply-adds. */
/* Allocates what the two calls below need: three [max_nodes][36] blocks of doubles (Sigma_kk, the chain factor's inverse
 * diagonal, its transfer blocks), a status word, and the ids and cross blocks of the 64 pairs one launch takes
 * (64 x (36 doubles + 2 ids)); Y is solved in place.  lfx_pose_graph_info's device_bytes grows by that amount.  As
 * lfx_pose_graph_reserve_priors, an exception to "no later call allocates", for the same reason: the config cannot grow.  A
 * second call is LFX_ERR_INVALID_ARGUMENT; a failed allocation LFX_ERR_OUT_OF_MEMORY, the graph as it was.  A graph that never
 * reserves holds the memory it always did and computes the bytes it always did. */
int lfx_pose_graph_reserve_marginals(lfx_ctx *ctx, lfx_pose_graph *graph);
/* Sigma_kk of nodes first .. first + count - 1 ([count][36], row-major, exactly symmetric: the lower triangle is computed and
 * mirrored).  Synchronous.  The first call after an optimise does the whole graph's work once and keeps all blocks on the
 * device; later calls only copy, until the graph is next written (add_nodes, add_edges, add_priors, set_poses, set_fixed,
 * release_first, optimize).  The poses are never touched, and the next optimise computes what it would have computed.
 * *code: LFX_POSE_GRAPH_CONVERGED (0), or LFX_POSE_GRAPH_NOT_POSITIVE_DEFINITE where a pivot was not positive (damping 0 and a
 * node nothing holds): cov_out is then untouched.  LFX_ERR_INVALID_ARGUMENT: before lfx_pose_graph_reserve_marginals; wherever
 * lfx_pose_graph_edge_chi2 refuses (before the first optimise; nodes, edges, priors or poses written since) and after
 * set_fixed or release_first since (H holds the flags of the optimise); a range outside the nodes. */
int lfx_pose_graph_marginals(lfx_ctx *ctx, lfx_pose_graph *graph, uint32_t first, uint32_t count, double *cov_out, int32_t *code,
                             void *stream);
/* For each pair (i, j) of pairs[n][2], i != j in either order: out[p] = [[Sigma_ii, Sigma_ij], [Sigma_ji, Sigma_jj]], 12 x 12
 * row-major, Sigma_ji = Sigma_ij^T exactly, the diagonal blocks byte for byte those of lfx_pose_graph_marginals.  The same
 * refusals, code and caching (the marginals are computed if they are not there yet).  i == j or an id that is not a node is
 * LFX_ERR_INVALID_ARGUMENT with nothing written.  Between nodes a chain apart the chain part of Sigma_ij is a product of
 * j - i 6 x 6 blocks, one wave per pair: the cost grows with the distance. */
int lfx_pose_graph_joint_covariances(lfx_ctx *ctx, lfx_pose_graph *graph, const uint32_t *pairs, uint32_t n, double *out,
                                     int32_t *code, void *stream);
/* The covariance of the residual r of an edge (i, j, Z = T_i^-1 T_j) at the current poses, from lfx_pose_graph_joint_covariances'
 * block of (i, j): r changes by A_i delta_i + A_j delta_j, so out = [A_i A_j] joint [A_i A_j]^T, with A_i, A_j those above at
 * phi = 0: Jri = I, R_Z^T R_i^T = R_j^T, R_Z^T = R_j^T R_i, d = R_i^T (t_j - t_i).  Its inverse is in the coordinates of an
 * edge's Omega: a loop candidate Z' passes a gate when r(Z')^T out^-1 r(Z') <= chi^2.  Host only, as
 * lfx_pose_graph_edge_information; every sum of three terms is (a0 b0 + a1 b1) + a2 b2; exactly symmetric. */
int lfx_pose_graph_relative_covariance(const double pose_i[12], const double pose_j[12], const double joint[144], double out[36]);

/* --- the keyframe store: sensor-frame clouds on the device, world maps written from them at the poses of the moment ------ */
/* What lets a map follow a pose graph.  lfx_mapper and lfx_odometry keep their clouds already in the world, so a corrected
 * pose cannot reach them; the store keeps every keyframe's records as the sensor saw them and one pose per keyframe, and a
 * world cloud is a pure function of the two: each coordinate ((r0*x + r1*y) + r2*z) + t in double, rounded once to float, the
 * 4th float copied -- lfx_mapper_add's arithmetic, so a build equals, byte for byte, a fresh mapper (thresholds 0) fed the
 * same clouds and poses.
 *   RECORDS  per kind (LFX_KEYFRAMES_EDGE, LFX_KEYFRAMES_SURFACE) records of 4 floats in the sensor frame, packed back to back
 *            in keyframe order; copied in as they are (16 bytes moved, no arithmetic: -0.0 and NaN payloads stay).
 *   BEGINS   per kind begin[max_keyframes + 1], 64-bit, the exclusive prefix of the counts: keyframe k is records begin[k] ..
 *            begin[k + 1] - 1.  The host keeps a mirror, so no call waits to learn a size.
 *   POSES    [max_keyframes][12] doubles, [R | t] row-major: lfx_pose_graph_view's layout.
 * Keyframe ids are 0, 1, 2 .. in order of addition; a caller that adds graph nodes in step has id == node id.  An empty cloud
 * is a keyframe with count 0.  lfx_keyframes_create allocates everything on the device (the records at max_points[kind], the
 * tables, the submap's workspace and a scratch of min(2^20, max(max_points)) records for lfx_keyframes_save); no later call
 * allocates device memory (pinned host blocks grow with the largest call) but lfx_keyframes_reserve_flags, once.
 * ORDER: every call is ordered behind the store's earlier calls, whichever streams they used (one event, waited for on the
 * call's stream and recorded behind the call).  The caller keeps alive, until `stream` has passed the call: the device
 * clouds given to lfx_keyframes_add, the pose array given to lfx_keyframes_follow, and d_out of lfx_keyframes_build (which
 * returns before the cloud is written).  d_out is device memory or a pinned block (lfx_host_alloc), which the host reads once
 * `stream` has passed.  Host arrays are copied before a call returns.  Nothing orders a LATER write of the
 * caller's own to those buffers behind the call: that is the caller's. */
#define LFX_KEYFRAMES_EDGE 0
#define LFX_KEYFRAMES_SURFACE 1
#define LFX_KEYFRAMES_NO_ID 0xFFFFFFFFu
typedef struct lfx_keyframes lfx_keyframes;
typedef struct lfx_keyframes_config {
  uint32_t max_keyframes;    /* 1 .. 2^30 */
  uint32_t reserved;         /* 0 */
  uint64_t max_points[2];    /* records per kind, 1 .. 2^40 */
} lfx_keyframes_config;
typedef struct lfx_keyframes_info_t {
  uint32_t n_keyframes, max_keyframes;
  uint64_t n_points[2], max_points[2];
  uint64_t device_bytes;     /* everything lfx_keyframes_create allocated on the device */
} lfx_keyframes_info_t;
typedef struct lfx_keyframes_store_view {
  const float *points[2];    /* device: the sensor-frame records of each kind */
  const uint64_t *begin[2];  /* device: [n_keyframes + 1] */
  const double *poses;       /* device: [n_keyframes][12] */
  uint32_t n_keyframes, reserved;
  uint64_t n_points[2];      /* the host's counts: begin[kind][n_keyframes] */
} lfx_keyframes_store_view;
/* n device clouds of one kind, addressed as lfx_mapper_add addresses its clouds: cloud s is d_count[s * count_stride] records
 * from record d_begin[s] of d_points; total_points the extent of d_points in records.  The last device batch's edge clouds
 * are {view.edge_points, view.scan_begin, view.scan_info + 2, 4, capacity}; its surface clouds the same with + 3. */
typedef struct lfx_keyframes_clouds {
  const float *d_points;
  const uint32_t *d_begin, *d_count;
  uint32_t count_stride, reserved;
  uint64_t total_points;
} lfx_keyframes_clouds;
typedef struct lfx_keyframes_submap_result {
  uint32_t n_selected;            /* keyframes of the window within the radius */
  uint32_t n_written_keyframes;   /* of those, the ones written: all of them unless truncated */
  uint64_t n_points;              /* records written to d_out */
  uint32_t first_id, last_id;     /* the first and the last keyframe written; LFX_KEYFRAMES_NO_ID where none was */
  int32_t truncated;              /* 1: a selected keyframe did not fit capacity_points; it and every later one is left out */
  uint32_t reserved;
} lfx_keyframes_submap_result;
/* all zero: the caller sets every field */
void lfx_keyframes_default_config(lfx_keyframes_config *config);
/* A config outside the ranges above is LFX_ERR_INVALID_ARGUMENT, a failed allocation LFX_ERR_OUT_OF_MEMORY with nothing left
 * allocated. */
int lfx_keyframes_create(lfx_ctx *ctx, const lfx_keyframes_config *config, lfx_keyframes **out);
void lfx_keyframes_destroy(lfx_keyframes *keyframes);
int lfx_keyframes_info(const lfx_keyframes *keyframes, lfx_keyframes_info_t *info);
/* The store where it lives.  The addresses are valid until the store is destroyed; the contents are current behind `stream`
 * once the store's earlier calls have passed (the call queues that wait), as lfx_pose_graph_view's are. */
int lfx_keyframes_view(lfx_ctx *ctx, const lfx_keyframes *keyframes, lfx_keyframes_store_view *view, void *stream);
/* n keyframes: keyframe first_id + s is edge cloud s and surface cloud s at poses[s] (host, [n][12], finite); *first_id (may
 * be NULL) the id of the first.  One wait (both kinds' counts and begins), then one copy launch per kind.  Checked before
 * anything is changed: NULL pointers, n 0, count_stride 0, a pose that is not finite and a cloud past total_points are
 * LFX_ERR_INVALID_ARGUMENT; more keyframes than max_keyframes or more records than max_points[kind] LFX_ERR_CAPACITY --
 * the store is as it was and nothing is left queued. */
int lfx_keyframes_add(lfx_ctx *ctx, lfx_keyframes *keyframes, const lfx_keyframes_clouds *edge, const lfx_keyframes_clouds *surface,
                      uint32_t n, const double *poses, uint32_t *first_id, void *stream);
/* One keyframe from host memory (either cloud may be empty), staged through the store's pinned block and copied from there
 * straight into place; *id (may be NULL) its id.  No wait unless the store's previous call still reads that block. */
int lfx_keyframes_add_host(lfx_ctx *ctx, lfx_keyframes *keyframes, const float *edge, uint32_t n_edge, const float *surface,
                           uint32_t n_surface, const double pose[12], uint32_t *id, void *stream);
/* Keyframes first .. first + count - 1: their poses overwritten from the host (finite), or copied to the host (synchronous). */
int lfx_keyframes_set_poses(lfx_ctx *ctx, lfx_keyframes *keyframes, uint32_t first, uint32_t count, const double *poses, void *stream);
int lfx_keyframes_poses(lfx_ctx *ctx, const lfx_keyframes *keyframes, uint32_t first, uint32_t count, double *poses_out, void *stream);
/* The call that makes the maps follow the graph: d_poses[k] -> keyframe k for k in [first, first + count), device to device
 * from a [.][12] double array such as the one lfx_pose_graph_view returns (taken on the same `stream`, it is current).
 * Asynchronous, no host copy; the poses are not inspected. */
int lfx_keyframes_follow(lfx_ctx *ctx, lfx_keyframes *keyframes, const double *d_poses, uint32_t first, uint32_t count, void *stream);
/* The world cloud of keyframes [first, first + count) of `kind` at the store's current poses to d_out, in keyframe order then
 * record order; *n_out, from the host's mirror, its records.  No wait; asynchronous.  More records than capacity_points is
 * LFX_ERR_CAPACITY with *n_out = the records needed, nothing queued.  count 0, or keyframes that are all empty: LFX_OK,
 * *n_out = 0, no launch (d_out may be NULL). */
int lfx_keyframes_build(lfx_ctx *ctx, const lfx_keyframes *keyframes, int kind, uint32_t first, uint32_t count, float *d_out,
                        uint64_t capacity_points, uint64_t *n_out, void *stream);
/* The local map around a point, selected on the device (the poses live there): keyframe k of [first, first + count) is
 * selected iff (dx^2 + dy^2) + dz^2 <= radius^2, the sums in double in that order, d = t_k - center.  The selected keyframes
 * are written to d_out in ascending id, each whole, as lfx_keyframes_build writes them; writing stops before the first that
 * would pass capacity_points.  One wait, for *result.  Nothing selected (or only empty keyframes): n_points 0 and no launch.
 * The window [first, first + count) is how a loop closer leaves the recent keyframes out.  A centre or radius that is not
 * finite, or a negative radius, is LFX_ERR_INVALID_ARGUMENT. */
int lfx_keyframes_submap(lfx_ctx *ctx, const lfx_keyframes *keyframes, int kind, const double center[3], double radius, uint32_t first,
                         uint32_t count, float *d_out, uint64_t capacity_points, lfx_keyframes_submap_result *result, void *stream);
/* dirname/edge.pcd and dirname/surface.pcd of the whole store at the current poses through lfx_pcd_write, named and written
 * as lfx_odometry_save's; an empty kind writes nothing (written[kind] = 0).  CHUNKED: the world cloud is built into the
 * store's scratch min(2^20, max(max_points)) records at a time (a chunk may begin and end inside a keyframe) and copied down
 * chunk by chunk, so a save needs no second copy of the records on the device.  Synchronous. */
int lfx_keyframes_save(lfx_ctx *ctx, const lfx_keyframes *keyframes, const char *dirname, int written[2], void *stream);

/* --- visibility votes: records that moved while the map was recorded, found from the keyframes that looked through them --- */
/* "Was this record still there when the sensor came by again?"  No reference counterpart; the model is Removert (Kim and Kim,
 * IROS 2020) and the visibility checks of ERASOR-style cleaners, over what the keyframe store already holds: sensor-frame
 * records and one pose per keyframe (best after lfx_loop_closer_update).  If keyframe v looked through the place where
 * keyframe k left a record and saw something clearly farther away, the record was not there when v looked.
 * THE DEFAULTS are Removert's or a numpy prototype's on a synthetic room; NONE IS MEASURED on real data, and neither is the
 * occupancy of images built from real feature clouds (lfx_visibility_result.occupied_cells is there so a caller sees it).
 * LIMITS: feature records only (the store holds nothing else); a viewer whose centre cell is empty gives no evidence; an
 * object that never moves while it is observed stays.
 *
 * Tables (lfx_visibility_tables, host only, the ONLY source: the device is given exactly these values):
 *   col_cos[m], col_sin[m]: lfx_segment_tables' values for W columns;
 *   row_tan[j] = tan((double)elev_min + (double)j * (double)elev_step), j = 0 .. H.
 * All arithmetic below is in double, unfused, on floats.
 *
 * Cell of a point (x, y, z), doubles:
 *   - skipped if a coordinate is not finite, or if x*x + y*y == 0;
 *   - rho = sqrt(x*x + y*y), r = sqrt((x*x + y*y) + z*z); skipped if r < (double)min_range or r >= (double)max_range;
 *   - column: the segmentation's bisection: m0 = y >= 0 ? W/2 : 0;  cross(m) = col_cos[m]*y - col_sin[m]*x;
 *       lo = 0, hi = W/2 - 1; while (lo < hi) { mid = (lo + hi + 1) >> 1; if (cross(m0 + mid) >= 0) lo = mid; else hi = mid - 1; }
 *     column = m0 + lo;
 *   - row: skipped if z < row_tan[0]*rho or z >= row_tan[H]*rho (one rounded product, one comparison); otherwise the largest
 *     j < H with z >= row_tan[j]*rho: lo = 0, hi = H - 1; while (lo < hi) { mid = (lo + hi + 1) >> 1;
 *     if (z >= row_tan[mid]*rho) lo = mid; else hi = mid - 1; }  row = lo.  No atan2 and no asin anywhere.
 * Image of viewer v, from v's own stored records of both kinds in the sensor frame as stored: cell (row, column) holds the
 *   least (float)r of the records that fall into it; a cell without a record is empty.  A minimum over a set: whatever the
 *   schedule.
 * Vote of viewer v on record p of target keyframe k.  The pair qualifies when k != v, both lie in the call's window
 *   [first, first + count), and (dx^2 + dy^2) + dz^2 <= radius^2 between the two poses' translations (lfx_keyframes_submap's
 *   rule and order).  Then
 *     w = the float world record lfx_keyframes_build writes for p;  d = (double)w - t_v (three subtractions);
 *     q_x = (R00*dx + R10*dy) + R20*dz, q_y = (R01*dx + R11*dy) + R21*dz, q_z = (R02*dx + R12*dy) + R22*dz, R = R_v;
 *     the cell and r_q of q as above -- q skipped: no vote;  m = max((double)margin_abs, (double)margin_rel * r_q);
 *     centre cell empty: no vote;
 *     an occupied cell with value R of the window -- rows row-guard .. row+guard clipped to [0, H), columns col-guard ..
 *       col+guard taken mod W -- OBJECTS iff (double)R <= r_q + m; empty cells do not object;
 *     THROUGH: no cell of the window objects.   AGREE: r_q - m <= (double)R_centre && (double)R_centre <= r_q + m.
 *   The two exclude each other; a record that gets neither is occluded from v.
 * Per record: through and agree, the counts over all qualifying viewers; a window holds at most LFX_VISIBILITY_MAX_WINDOW
 *   keyframes, so both fit 16 bits.  The vote word is through | agree << 16.  DYNAMIC (flag byte 1, otherwise 0) iff
 *   through >= min_through && (uint64)agree * agree_weight < through.  A record of a keyframe without viewers has word 0 and
 *   flag 0.  Every count is an integer: the same store, poses and config give the same bytes whatever the schedule and
 *   however the viewers are chunked. */
#define LFX_VISIBILITY_MAX_WINDOW 65536u
#define LFX_VISIBILITY_SCRATCH_WORDS (1u << 22)
typedef struct lfx_visibility lfx_visibility;
typedef struct lfx_visibility_config {
  uint32_t n_rows;              /* H: 32; 1 .. 128 */
  uint32_t n_columns;           /* W: 360; even, 4 .. 4096 */
  float elev_min, elev_step;    /* -0.43633232 (-25 degrees), 0.027270770 (50 degrees / 32); elev_step > 0, elev_min > -pi/2,
                                   elev_min + H * elev_step < pi/2 (in double) */
  float min_range, max_range;   /* 1.0, 100.0; 0 < min_range < max_range, finite */
  float radius;                 /* 15.0; finite, >= 0: a viewer lies within it of the target keyframe */
  float margin_abs, margin_rel; /* 0.3, 0.02; finite, >= 0 */
  uint32_t guard;               /* 1; 0 .. 2: the window is (2 guard + 1)^2 cells */
  uint32_t min_through;         /* 2; >= 1 */
  uint32_t agree_weight;        /* 1; >= 0 */
  uint32_t reserved;            /* 0 */
} lfx_visibility_config;
typedef struct lfx_visibility_info_t {
  lfx_visibility_config config;
  uint32_t max_window, max_resident_images;
  uint64_t device_bytes;        /* everything lfx_visibility_create allocated on the device */
} lfx_visibility_info_t;
typedef struct lfx_visibility_result {
  uint64_t n_pairs;             /* ordered pairs (k, v) of non-empty keyframes of the window that qualify */
  uint64_t n_records[2];        /* per kind: the window's records, */
  uint64_t n_voted[2];          /*   those with a vote word != 0, */
  uint64_t n_dynamic[2];        /*   those flagged; all counted on the device */
  uint64_t occupied_cells;      /* of the viewers' images (the window's non-empty keyframes), */
  uint64_t total_cells;         /*   of their H * W cells each */
  uint32_t n_viewer_chunks;     /* ceil(non-empty keyframes of the window / max_resident_images) */
  uint32_t reserved;
} lfx_visibility_result;
void lfx_visibility_default_config(lfx_visibility_config *config);
/* host only, no context.  LFX_ERR_INVALID_ARGUMENT: NULL arguments, every field outside the ranges above, reserved != 0. */
int lfx_visibility_tables(const lfx_visibility_config *config, double *col_cos /*[W]*/, double *col_sin /*[W]*/, double *row_tan /*[H+1]*/);
/* Everything on the device is allocated here: the images (max_resident_images x H x W words), the tables, the viewer list,
 * the counters, LFX_VISIBILITY_SCRATCH_WORDS vote words for callers that pass no d_votes, and a pinned block; no later call
 * allocates device memory.  1 <= max_resident_images <= max_window <= LFX_VISIBILITY_MAX_WINDOW.  A window with more non-
 * empty keyframes than max_resident_images is processed in chunks of that many viewers, in ascending id and in stream order.
 * LFX_ERR_INVALID_ARGUMENT: what lfx_visibility_tables refuses and capacities outside that; LFX_ERR_OUT_OF_MEMORY with nothing
 * left allocated. */
int lfx_visibility_create(lfx_ctx *ctx, const lfx_visibility_config *config, uint32_t max_window, uint32_t max_resident_images,
                          lfx_visibility **out);
void lfx_visibility_destroy(lfx_visibility *visibility);
int lfx_visibility_info(const lfx_visibility *visibility, lfx_visibility_info_t *info);
/* The votes of keyframes [first, first + count) on each other.  d_votes[kind][i] (u32, an entry may be NULL) and
 * d_flags[kind][i] (u8, required) are addressed by the STORE's record index of the kind, begin[kind][first] <= i <
 * begin[kind][first + count]; nothing outside that is touched.  Ordered behind the store's earlier calls through the store's
 * event, as every store call is, and behind this object's earlier runs; recorded behind itself on both.  One wait, for
 * *result.  Between chunks of viewers a record's counts live in its own vote word -- no atomic touches a vote -- which is
 * d_votes[kind][i] or, where that is NULL, the object's own LFX_VISIBILITY_SCRATCH_WORDS words (edge records first): a run
 * that needs more than one chunk, passes a NULL d_votes entry and has more records of those kinds than that is
 * LFX_ERR_CAPACITY (pass d_votes, or keep more images resident).  LFX_ERR_INVALID_ARGUMENT, before anything is queued: NULL
 * pointers, a window past the store, count > max_window.  count 0, or only empty keyframes: LFX_OK, *result zero, no launch. */
int lfx_visibility_run(lfx_ctx *ctx, lfx_visibility *visibility, const lfx_keyframes *keyframes, uint32_t first, uint32_t count,
                       uint32_t *const d_votes[2], uint8_t *const d_flags[2], lfx_visibility_result *result, void *stream);
/* lfx_keyframes_build with the records whose flag byte is non-zero left out and the order kept: d_flags[i] (u8, device) is
 * addressed by the store's record index of `kind`, as lfx_visibility_run writes it; a kept record is byte for byte what
 * lfx_keyframes_build writes.  d_begin_out (device, [count + 1], may be NULL): the exclusive prefix of the kept counts per
 * keyframe -- narrowed to 32 bits, with its differences, what lfx_mapper_add and lfx_keyframes_add take.  One wait, for
 * *n_out (the kept records are counted on the device).  More kept records than capacity_points is LFX_ERR_CAPACITY with
 * *n_out = the records needed and no record written.  count 0, or keyframes that are all empty: LFX_OK, *n_out = 0,
 * d_begin_out zero.  The counts per 1 024 records live in a table lfx_keyframes_create allocates (8 bytes per 1 024 records
 * of the larger max_points). */
int lfx_keyframes_build_masked(lfx_ctx *ctx, const lfx_keyframes *keyframes, int kind, uint32_t first, uint32_t count,
                               const uint8_t *d_flags, float *d_out, uint64_t capacity_points, uint64_t *d_begin_out,
                               uint64_t *n_out, void *stream);

/* --- flags kept in the store: the masked submap and the masked save --------------------------------------------------------- */
/* One byte per record and kind that BELONGS to the store, so that lfx_keyframes_submap_masked, lfx_keyframes_save_masked and a
 * loop closer (lfx_loop_closer_set_masked) leave the flagged records out without a second store.  A NON-ZERO byte leaves the
 * record out: lfx_keyframes_build_masked's rule.  The bytes are addressed by the store's record index of the kind, exactly as
 * lfx_visibility_run and lfx_keyframes_build_masked address d_flags, so both take the pointers lfx_keyframes_flags returns:
 *   lfx_visibility_run(.., d_flags = the two pointers, ..) writes the store's flags in place;
 *   lfx_keyframes_build_masked(.., d_flags = the kind's pointer, ..) builds under them.
 * Both already order themselves behind the store's earlier calls through the store's event and record it behind themselves,
 * so a masked call queued after them, on whichever stream, sees what they wrote.
 * RESERVE, as lfx_pose_graph_reserve_priors / _reserve_marginals: one call after lfx_keyframes_create, before or after
 * keyframes were added, allocates max_points[kind] bytes per kind, zeroed, and two 8-byte words per keyframe of max_keyframes
 * for the masked submap; no later call allocates device memory.  Idempotent.  LFX_ERR_OUT_OF_MEMORY leaves the store as it
 * was, without flags.  A store that never reserves is untouched: every other call is as it was, byte for byte and launch
 * for launch.
 * CONTRACT: the reserve zeroes everything; bytes at or past n_points[kind] are the store's and stay zero --
 * lfx_keyframes_set_flags, _clear_flags and lfx_visibility_run write inside records only, and a caller that writes through
 * lfx_keyframes_flags keeps to that.  Before the reserve, lfx_keyframes_flags, _set_flags, _clear_flags, _submap_masked and
 * _save_masked are LFX_ERR_INVALID_ARGUMENT with nothing queued. */
typedef struct lfx_keyframes_flags_info_t {
  int32_t reserved;          /* 1: lfx_keyframes_reserve_flags has run */
  uint32_t pad;
  uint64_t device_bytes;     /* what the reserve allocated on the device (not part of lfx_keyframes_info_t.device_bytes) */
  uint64_t n_flagged[2];     /* records of the store with a non-zero byte, counted on the device */
} lfx_keyframes_flags_info_t;
int lfx_keyframes_reserve_flags(lfx_ctx *ctx, lfx_keyframes *keyframes, void *stream);
/* The two device addresses ([0] edge, [1] surface), valid until the store is destroyed; the contents are current behind
 * `stream` once the store's earlier calls have passed (the call queues that wait), as lfx_keyframes_view's are. */
int lfx_keyframes_flags(lfx_ctx *ctx, lfx_keyframes *keyframes, uint8_t *d_flags[2], void *stream);
/* The flag bytes of keyframes [first, first + count) of `kind` copied device to device from d_src, which is addressed by the
 * store's record index as above: only d_src[begin[first] .. begin[first + count]) is read -- for a binder with a detector of
 * its own, such as segmentation classes.  lfx_keyframes_clear_flags zeroes the same range.  Both are asynchronous and
 * ordered through the store's event, as every store call is; keyframes without records: LFX_OK, nothing queued (d_src may
 * be NULL). */
int lfx_keyframes_set_flags(lfx_ctx *ctx, lfx_keyframes *keyframes, int kind, uint32_t first, uint32_t count, const uint8_t *d_src,
                            void *stream);
int lfx_keyframes_clear_flags(lfx_ctx *ctx, lfx_keyframes *keyframes, int kind, uint32_t first, uint32_t count, void *stream);
/* n_flagged over the store's records: integer sums on the device, one wait.  Without a reserve the record is all zero and
 * the call is LFX_OK. */
int lfx_keyframes_flags_info(lfx_ctx *ctx, const lfx_keyframes *keyframes, lfx_keyframes_flags_info_t *info, void *stream);
/* lfx_keyframes_submap over the store's own flags.  Selection: lfx_keyframes_submap's, unchanged.  A selected keyframe
 * contributes its KEPT records in record order, each byte for byte what lfx_keyframes_build writes for it.  With kept[k] the
 * kept records of keyframe k, a selected keyframe is written iff the exclusive sum of kept over the selected keyframes before
 * it, plus kept[k], is <= capacity_points; nothing behind the first keyframe that does not fit is written.  A selected
 * keyframe whose records are all flagged is written with 0 records and counts in n_written_keyframes, as an empty keyframe
 * does.  *result has lfx_keyframes_submap's meanings; n_points counts kept records.  One wait, for *result; nothing selected,
 * or nothing kept: no scatter launch (d_out may be NULL).  Every refusal is lfx_keyframes_submap's, and before the reserve
 * LFX_ERR_INVALID_ARGUMENT.  Only integer counts and prefixes decide a record's place (no atomic): the same store, flags,
 * poses and arguments give the same bytes.  Flags and records are read only of the 1 024-record runs of the window that hold
 * a record of a selected keyframe: the cost follows the selected records, not the window. */
int lfx_keyframes_submap_masked(lfx_ctx *ctx, const lfx_keyframes *keyframes, int kind, const double center[3], double radius,
                                uint32_t first, uint32_t count, float *d_out, uint64_t capacity_points,
                                lfx_keyframes_submap_result *result, void *stream);
/* lfx_keyframes_save with the store's flagged records left out: the same file names, lfx_pcd_write and chunking through the
 * store's scratch (a chunk may begin and end inside a keyframe; one wait per chunk, for its kept count).  Each file holds
 * exactly what lfx_keyframes_build_masked of the whole store under the store's flags holds; a kind that is empty or whose
 * records are all flagged writes no file (written[kind] = 0).  Synchronous. */
int lfx_keyframes_save_masked(lfx_ctx *ctx, const lfx_keyframes *keyframes, const char *dirname, int written[2], void *stream);

/* --- the loop closer: revisits found, verified and closed over a store, an index and a graph ------------------------------ */
/* What joins the sections above.  No reference counterpart; the model is LIO-SAM's loop-closure thread (Shan et al., IROS 2020)
 * with Scan Context as the detector.  THE CONTRACT: keyframe id == place entry == graph node id -- the caller adds a keyframe to
 * the store, its descriptor to the index and its pose to the graph in step.  A call that names a keyframe >= min(store size,
 * index size, graph nodes) is LFX_ERR_INVALID_ARGUMENT and nothing is touched.  The closer keeps the three handles and owns
 * none of them: they outlive it.  It adds no kernel of its own: every step below is a public call of this header, and its
 * results are those calls' bytes.
 *
 * DETECT of keyframes first .. first + count - 1: one lfx_place_db_query_gated, the query descriptors the index's own entries
 * first .., gates[q] = { limit = q >= min_gap ? q - min_gap + 1 : 0 (e + min_gap <= q), pose = q }, d_poses the store's pose
 * array, radius = search_radius, k = n_candidates.  Matches with distance > max_distance are turned into the empty match
 * (UINT32_MAX, 0, +inf, 0).
 *
 * VERIFY of query keyframe q against a candidate (c = entry, yaw), c + min_gap <= q:
 *   1. lfx_keyframes_submap of each kind into the closer's buffers (submap_capacity[kind] records): centre = the translation
 *      of keyframe c's current pose, submap_radius, window [max(c - w, 0), min(c + w, q - min_gap) + 1), w =
 *      submap_half_window.  truncated is reported in the closure and is no error.  (lfx_loop_closer_set_masked(closer, 1):
 *      lfx_keyframes_submap_masked in its place, and submap[kind] carries kept counts.)
 *   2. lfx_map_create on each submap with map_cell_size; both maps are destroyed before the call returns.  (The maps allocate
 *      as lfx_map_create does today: per call.  Everything else the closer uses on the device is allocated by
 *      lfx_loop_closer_create: the submap buffers, the downsample output, the count words.)
 *   3. lfx_voxel_downsample of q's surface records as the store holds them (sensor frame) at surface_leaf -- 0: no
 *      downsample; a cloud PCL would hand back unfiltered (status 1) is used as stored.  The edge records are used as stored.
 *   4. lfx_scan_to_map_align_report, one cloud, n_neighbors, max_iter, initial = pose_c x Rz(yaw) (the place index's
 *      convention): R = R_c Rz, (r0 cos + r1 sin, -r0 sin + r1 cos, r2) per row, t = t_c.
 * ACCEPTED iff all of, tested in this order (reason: the first that fails): neither submap and neither cloud of q is empty;
 * the align code is a success or LFX_ALIGN_MAX_ITERATION; report.valid; report.rank == 6; !(reject_degenerate &&
 * report.degenerate); rms_edge <= max_rms_edge; rms_surface <= max_rms_surface; (n_edge_inliers + n_surface_inliers) /
 * (n_edge + n_surface) >= min_inlier_share; where scale_by_sigma2: sigma2 finite and > 0.  The thresholds on rms and inliers
 * have NO MEASURED DEFAULT and ship permissive (+inf, +inf, 0); DESIGN.md section 7 records what the test drive showed.
 * THE EDGE of a closure that ran an alignment with a valid report (accepted or not): i = c, j = q, flags LFX_EDGE_ROBUST,
 * Z = lfx_motion_between(pose_c, result.pose), Omega = lfx_pose_graph_edge_information(result.pose, report.information),
 * every entry divided by sigma2 where scale_by_sigma2.  Otherwise the edge is all zero.
 *
 * UPDATE of keyframes first .. first + count - 1: one detect; per keyframe, verify its candidates best first, stopping at the
 * first accepted or after max_verify; all accepted edges in one lfx_pose_graph_add_edges (LFX_ERR_CAPACITY: the call returns
 * that code, the closures are filled, the graph is untouched); if any went in, lfx_pose_graph_optimize; if its code is
 * CONVERGED or MAX_ITERATIONS, lfx_keyframes_follow from lfx_pose_graph_view for all nodes.  Every verification of the call
 * sees the poses from before the optimisation.  With no accepted closure neither the graph nor the store is written.
 * closures[s] is the last verification of keyframe first + s; a keyframe without a candidate has reason
 * LFX_LOOP_NO_CANDIDATE, candidate UINT32_MAX and every other byte 0.  All calls are synchronous. */
#define LFX_LOOP_ACCEPTED 0
#define LFX_LOOP_NO_CANDIDATE 1         /* update: detect left the keyframe no candidate */
#define LFX_LOOP_EMPTY_QUERY 2          /* the query keyframe has no edge or no surface record */
#define LFX_LOOP_EMPTY_SUBMAP 3         /* a submap of either kind has no record */
#define LFX_LOOP_ALIGN_FAILED 4         /* the align code is neither a success nor LFX_ALIGN_MAX_ITERATION */
#define LFX_LOOP_NO_REPORT 5            /* !report.valid */
#define LFX_LOOP_RANK 6                 /* report.rank != 6 */
#define LFX_LOOP_DEGENERATE 7
#define LFX_LOOP_RMS_EDGE 8
#define LFX_LOOP_RMS_SURFACE 9
#define LFX_LOOP_INLIERS 10
#define LFX_LOOP_SIGMA2 11
typedef struct lfx_loop_closer lfx_loop_closer;
typedef struct lfx_loop_closer_config {
  uint32_t min_gap;              /* 50: a candidate c of q has c + min_gap <= q; >= 1 */
  uint32_t n_candidates;         /* 3; 1 .. 16 */
  uint32_t max_verify;           /* 1; >= 1 */
  uint32_t submap_half_window;   /* 25 (LIO-SAM: historyKeyframeSearchNum) */
  double search_radius;          /* 15.0 (LIO-SAM: historyKeyframeSearchRadius); >= 0, +inf: descriptors alone */
  double max_distance;           /* 0.2: the Scan Context distance above which a candidate is dropped; <= keeps */
  double submap_radius;          /* 25.0; >= 0, finite */
  uint64_t submap_capacity[2];   /* records of the edge / surface submap buffer; the caller sets them, 1 .. 2^32 - 1 */
  float map_cell_size;           /* 1.0 */
  float surface_leaf;            /* 1.0; 0: no downsample */
  uint32_t n_neighbors;          /* 15 */
  int32_t max_iter;              /* 20 */
  double max_rms_edge, max_rms_surface;   /* +inf, +inf: no measured default */
  double min_inlier_share;       /* 0: no measured default */
  int32_t reject_degenerate;     /* 1 */
  int32_t scale_by_sigma2;       /* 1 */
  uint64_t downsample_capacity;  /* records of the downsample output: the most surface records a QUERY keyframe may have where
                                    surface_leaf > 0 (one with more is LFX_ERR_CAPACITY); <= 2^32 - 1.  0, the default: the
                                    store's max_points[1] or 2^20, whichever is less.  Nothing is allocated, and no keyframe
                                    is too large, where surface_leaf is 0 */
} lfx_loop_closer_config;
typedef struct lfx_loop_closure {
  uint32_t query, candidate;     /* q, c */
  int32_t accepted, reason;      /* reason: LFX_LOOP_* */
  lfx_place_match match;         /* the candidate as it was given */
  lfx_align_result result;
  lfx_align_report report;
  lfx_keyframes_submap_result submap[2];
  lfx_pose_graph_edge edge;
} lfx_loop_closure;
typedef struct lfx_loop_closer_result {
  uint32_t n_detected;           /* keyframes of the range with at least one candidate */
  uint32_t n_verified;           /* verifications run */
  uint32_t n_accepted;           /* closures accepted: the edges that went into the graph */
  int32_t followed;              /* 1: the store's poses were taken from the graph */
  lfx_pose_graph_result graph;   /* of lfx_pose_graph_optimize; all zero where it did not run */
} lfx_loop_closer_result;
typedef struct lfx_loop_closer_info_t {
  uint64_t device_bytes;         /* everything lfx_loop_closer_create allocated on the device */
} lfx_loop_closer_info_t;
void lfx_loop_closer_default_config(lfx_loop_closer_config *config);
/* A config outside the ranges above, or a store, an index or a graph of another device than ctx's, is
 * LFX_ERR_INVALID_ARGUMENT, a failed allocation LFX_ERR_OUT_OF_MEMORY with nothing left allocated. */
int lfx_loop_closer_create(lfx_ctx *ctx, const lfx_loop_closer_config *config, lfx_keyframes *keyframes, lfx_place_db *db,
                           lfx_pose_graph *graph, lfx_loop_closer **out);
void lfx_loop_closer_destroy(lfx_loop_closer *closer);
int lfx_loop_closer_info(const lfx_loop_closer *closer, lfx_loop_closer_info_t *info);
/* Verify against clean submaps (lfx_loop_closer_config cannot grow, so the switch is a pair of calls).  0, the default: every
 * byte as described above.  1: step 1 of VERIFY calls lfx_keyframes_submap_masked where it calls lfx_keyframes_submap, and
 * nothing else changes -- closure.submap[kind] then carries kept counts.  Setting 1 on a closer whose store has no flags
 * reserved is LFX_ERR_INVALID_ARGUMENT and the closer stays as it was.  The QUERY keyframe's own clouds are used as stored,
 * flagged records and all: a mover in one scan is a minority of rows under the robust weights, while a submap stacks up to
 * 2 submap_half_window + 1 keyframes of trails. */
int lfx_loop_closer_set_masked(lfx_loop_closer *closer, int masked);
int lfx_loop_closer_get_masked(const lfx_loop_closer *closer, int *masked);
/* candidates host [count][n_candidates]; n_eligible host [count], may be NULL. */
int lfx_loop_closer_detect(lfx_ctx *ctx, lfx_loop_closer *closer, uint32_t first, uint32_t count, lfx_place_match *candidates,
                           uint32_t *n_eligible, void *stream);
/* LFX_ERR_INVALID_ARGUMENT also for a candidate without an entry, with entry + min_gap > query_id or with a yaw that is not
 * finite. */
int lfx_loop_closer_verify(lfx_ctx *ctx, lfx_loop_closer *closer, uint32_t query_id, const lfx_place_match *candidate,
                           lfx_loop_closure *out, void *stream);
/* closures host [count]; result may be NULL. */
int lfx_loop_closer_update(lfx_ctx *ctx, lfx_loop_closer *closer, uint32_t first, uint32_t count, lfx_loop_closure *closures,
                           lfx_loop_closer_result *result, void *stream);

/* --- the voxel filter: clouds of any size thinned to one centroid per voxel of a world-anchored grid ------------------------ */
/* What stands between the world clouds above (lfx_keyframes_build .. _submap_masked, lfx_mapper_view, lfx_odometry_view) and a
 * file or an lfx_map: every place seen N times holds N layers of records, and every system this stack is modelled on thins its
 * clouds to a voxel grid before they become a target (LIO-SAM, LeGO-LOAM: leaves 0.2 m for edges, 0.4 m for surfaces -- the
 * rolling map's).  lfx_voxel_downsample is the reference's per-scan Downsample: one workgroup per cloud and a grid relative to the
 * cloud's own bounds.  This filter works at any size, incrementally, and its output is a pure function of the input SEQUENCE:
 * the same records in the same order give the same bytes, whatever the device made of the order in between.
 *
 * THE MODEL.  leaf > 0; inv = 1.0f / leaf (float).  A record p = (x, y, z, .):
 *   VOXEL    per axis v = floorf(p * inv), the product in float: the rolling map's voxel coordinate.  The grid is anchored at
 *            the world origin, so a voxel is the same voxel whatever else is in the cloud and however it is split over calls.
 *   SKIPPED  x, y or z not finite: counted in n_nonfinite.  Otherwise a |v| that is not below 2^20 on some axis: n_out_of_range.
 *   ADDS     1 to its voxel's count and, per axis, the signed integer
 *              q = (int64) rint((((double)p * (double)inv) - (double)v) * 16777216.0)
 *            -- separate double operations, no contraction, rint to nearest even -- to the voxel's sum S.  Sums are 64-bit
 *            two's-complement integer adds and nothing else (no floating-point atomic), so they do not depend on the order of
 *            arrival; |q| < 1.1 * 2^24, so 2^32 records of one voxel cannot overflow.
 *   RANK     a record's index among all records handed to the filter since the reset, skipped ones included (the host keeps
 *            the running base).  A voxel keeps the least rank that reached it, an integer minimum.
 *   CENTROID per axis (float)((((double)v) + ((double)S / (double)n) * 0x1p-24) / (double)inv), n the count; the 4th float is
 *            1.0f, as lfx_voxel_downsample writes.  A voxel of one record returns it to within leaf * 2^-25 + 1 ulp.
 *   ORDER    voxels are written in ascending order of their least rank: the order of first appearance.
 *   COUNTS   d_counts_out[i] = the count of output voxel i, saturated at 2^32 - 1.
 *   MIN      a voxel with fewer than min_points (>= 1) records is left out (PCL: MinimumPointsNumberPerVoxel).
 *
 * THE TABLE.  2^log2_slots entries of 64 bytes (key, least rank, count, three sums: one line), open addressing with linear
 * probing from the top log2_slots bits of key * 0x9E3779B97F4A7C15 (key: the rolling map's voxel key).  An insert is a compare-
 * and-swap on the entry's key -- empty or equal: found, otherwise the next entry -- at most 2^log2_slots probes, then the
 * record is counted in n_table_full; it never waits on another thread.  Which entry a voxel lands in may depend on the race;
 * nothing observable does.  Size log2_slots for about twice the voxels expected.  An emit marks the surviving voxels' least
 * ranks in a bitmap over ranks (max_records bits), scans the words' population counts and writes: no sort, no second pass
 * over the input.  lfx_voxel_filter_create allocates all of it (64 B per entry, 1 B per 4 ranks, a staging buffer of 2^16
 * records for lfx_voxel_filter_add_host); no later call allocates device memory.  Calls are ordered through one event behind
 * the filter's last call, whatever streams they were given. */
typedef struct lfx_voxel_filter lfx_voxel_filter;
typedef struct lfx_voxel_filter_config {
  uint32_t log2_slots;    /* 4 .. 30: the table has 2^log2_slots voxel entries */
  uint32_t reserved;      /* 0 */
  uint64_t max_records;   /* 1 .. 2^40: ranks a filter can hand out between two resets */
} lfx_voxel_filter_config;
typedef struct lfx_voxel_filter_result {
  uint64_t n_records;       /* ranks handed out since the reset */
  uint64_t n_accumulated;   /* records that reached a voxel */
  uint64_t n_nonfinite;     /* skipped: x, y or z not finite */
  uint64_t n_out_of_range;  /* skipped: a voxel coordinate not below 2^20 in size */
  uint64_t n_table_full;    /* skipped: no entry left for their voxel */
  uint64_t n_voxels;        /* occupied entries */
  uint64_t n_written;       /* voxels written by this emit (count >= min_points) */
} lfx_voxel_filter_result;
typedef struct lfx_voxel_filter_info_t {
  uint64_t slots, max_records;
  uint64_t n_records;        /* ranks handed out since the reset (the host's count) */
  uint64_t device_bytes;     /* everything lfx_voxel_filter_create allocated on the device */
  float leaf;                /* of the last reset; 0 before the first */
  uint32_t reserved;
} lfx_voxel_filter_info_t;
/* All zero: the caller sets every field. */
void lfx_voxel_filter_default_config(lfx_voxel_filter_config *config);
/* A config outside the ranges above is LFX_ERR_INVALID_ARGUMENT, a failed allocation LFX_ERR_OUT_OF_MEMORY with nothing left
 * allocated. */
int lfx_voxel_filter_create(lfx_ctx *ctx, const lfx_voxel_filter_config *config, lfx_voxel_filter **out);
void lfx_voxel_filter_destroy(lfx_voxel_filter *filter);
int lfx_voxel_filter_info(const lfx_voxel_filter *filter, lfx_voxel_filter_info_t *info);
/* Empties the table and sets the leaf (finite, > 0, 1.0f / leaf finite and > 0); ranks restart at 0.  Asynchronous.  Every
 * other call below is LFX_ERR_INVALID_ARGUMENT before the first reset. */
int lfx_voxel_filter_reset(lfx_ctx *ctx, lfx_voxel_filter *filter, float leaf, void *stream);
/* n_points records of 4 floats on the device (lfx_voxel_filter_add) or on the host (_add_host, which goes up in chunks of 2^16
 * records through a pinned block and waits for the chunk before); asynchronous, the records are read behind `stream`.  More
 * records than max_records leaves room for: LFX_ERR_CAPACITY with nothing queued.  n_points 0: LFX_OK, nothing queued. */
int lfx_voxel_filter_add(lfx_ctx *ctx, lfx_voxel_filter *filter, const float *d_points, uint64_t n_points, void *stream);
int lfx_voxel_filter_add_host(lfx_ctx *ctx, lfx_voxel_filter *filter, const float *points, uint64_t n_points, void *stream);
/* The voxels with at least min_points records to d_out (device, capacity_points records of 4 floats) in the order above, their
 * counts to d_counts_out (device u32, may be NULL).  One wait, for *result.  n_table_full != 0, or n_written > capacity_points:
 * LFX_ERR_CAPACITY with *result filled and nothing written to d_out -- a silently thinned map is worse than an error.  The
 * table is not consumed: more adds and another emit are legal, which is how a map grows keyframe by keyframe.  min_points 0
 * or a missing result is LFX_ERR_INVALID_ARGUMENT before anything is touched; d_out may be NULL where nothing is written. */
int lfx_voxel_filter_emit(lfx_ctx *ctx, lfx_voxel_filter *filter, uint32_t min_points, float *d_out, uint64_t capacity_points,
                          uint32_t *d_counts_out, lfx_voxel_filter_result *result, void *stream);
/* The keyframe store straight into the filter: one launch over the store's SENSOR-frame records of keyframes [first, first +
 * count) of `kind`, each read once, transformed with lfx_keyframes_build's arithmetic at the store's current poses and
 * accumulated -- no world cloud is written.  masked != 0 leaves out the records the store's flags leave out (before
 * lfx_keyframes_reserve_flags: LFX_ERR_INVALID_ARGUMENT).  Every source record of the range takes a rank, flagged or not, and
 * ranks are monotone in build order: a following emit gives byte for byte what lfx_voxel_filter_add of lfx_keyframes_build's
 * (masked: lfx_keyframes_build_masked's under the store's flags) output gives.  Asynchronous, ordered behind the store's and
 * the filter's earlier calls.  Keyframes outside the store, a wrong kind: LFX_ERR_INVALID_ARGUMENT; more records than
 * max_records leaves room for: LFX_ERR_CAPACITY; nothing queued either way. */
int lfx_voxel_filter_add_keyframes(lfx_ctx *ctx, lfx_voxel_filter *filter, const lfx_keyframes *keyframes, int kind, uint32_t first,
                                   uint32_t count, int masked, void *stream);
/* lfx_keyframes_save through the filter: per kind a reset with leaf[kind], lfx_voxel_filter_add_keyframes over the whole store
 * (masked as there), an emit with min_points in chunks through the store's scratch, and dirname/edge.pcd, dirname/surface.pcd
 * through lfx_pcd_write.  A kind that is empty or of which no voxel survives writes no file (written[kind] = 0).  A full
 * table, or a kind with more records than the filter's max_records: LFX_ERR_CAPACITY.  The filter is left holding the last
 * kind written.  Synchronous. */
int lfx_keyframes_save_filtered(lfx_ctx *ctx, const lfx_keyframes *keyframes, lfx_voxel_filter *filter, const float leaf[2],
                                uint32_t min_points, int masked, const char *dirname, int written[2], void *stream);

/* --- occupancy grids: 2-D free / occupied / unknown maps rendered from scans by ray casting --------------------------------- */
/* What planners, costmaps, map_server and nav_msgs/OccupancyGrid consume.  No reference counterpart; the model is the ray-cast
 * grid of Cartographer, slam_toolbox and gmapping, with OctoMap's log-odds.  Two steps: every scan is reduced ONCE, from the
 * batch's input records (the free-space evidence is there and nowhere else: a store of feature records cannot feed this), to
 * a virtual 2-D scan of W beams kept on the device with one pose per scan; the grid is then rendered from all kept beams at
 * the poses of the moment -- after a loop closure the poses follow the graph (lfx_occupancy_follow) and the grid is rendered
 * again without any scan being read again.  All arithmetic below is in double, unfused, on the floats read through the
 * context's lfx_layout, unless stated otherwise.  The same beams and poses give the same bytes, whatever the schedule.
 *
 * CONFIG.  origin_x, origin_y: the world coordinates of the lower-left corner of cell (0, 0).  z_min, z_max: the obstacle band,
 *   on the height above the sensor in world axes.  chunk_scans: the scans whose per-scan vote sets the workspace holds at once.
 *   inv_res = 1.0 / (double)resolution; ceil(max_range * inv_res) must be at most 32768.  The column tables col_cos[m],
 *   col_sin[m] = cos, sin of -M_PI + ((2.0 * M_PI) * (double)m) / (double)W come from lfx_occupancy_tables (host only, the ONLY
 *   source: the device is given exactly these values; the same table as the segmentation's).
 *
 * REDUCE (lfx_occupancy_add_batch).  Record i of scan s (i: its index in the scan's input) with the scan's pose [R | t]:
 *   - skipped if x, y or z is not finite, if x*x + y*y == 0, or if r = sqrt((x*x + y*y) + z*z) has r < (double)min_range or
 *     r >= (double)max_range;
 *   - levelled direction: dx = (r0*x + r1*y) + r2*z, dy and dz likewise with rows 1 and 2 of R (the translation is not added);
 *     h2 = dx*dx + dy*dy; skipped if h2 == 0; kf = (float)h2;
 *   - column m: the segmentation's bisection over col_cos / col_sin with (dx, dy) for (x, y), upper half iff dy >= 0.0;
 *   - class: with a class array (d_class, addressed by scan_begin[s] + i as lfx_segment_batch writes it) the record passes a mask
 *     iff bit (1 << class) is set in it (a byte above 3 passes neither); without one it passes both masks;
 *   - OBSTACLE candidate iff (double)z_min <= dz && dz <= (double)z_max and it passes obstacle_mask: the column's obstacle winner
 *     has the least kf, equal floats go to the lower i;
 *   - CLEAR candidate: any other record that passed the gates and passes clear_mask: the column's clear winner has the greatest
 *     kf, equal floats go to the lower i.
 *   Beam (s, m), 16 bytes {x, y, z, kind}: with an obstacle winner its sensor-frame x, y, z (copied bit for bit) and
 *   LFX_OCCUPANCY_HIT; otherwise with a clear winner its x, y, z and LFX_OCCUPANCY_CLEAR; otherwise 0, 0, 0 and
 *   LFX_OCCUPANCY_NONE.  Two 64-bit integer atomics (a minimum and a maximum over a key of kf's bits and the index) do this in
 *   one pass over the records; no floating-point atomic is used anywhere.
 *
 * RENDER (lfx_occupancy_render).  For scan k at the pose the store holds NOW:
 *   - origin cell: ox = floor((t_x - origin_x) * inv_res), oy likewise;
 *   - end cell of each beam of kind != NONE: wx = ((r0*x + r1*y) + r2*z) + t_x (lfx_keyframes_build's sum without the rounding
 *     to float), ex = floor((wx - origin_x) * inv_res); wy, ey likewise (z enters only through R);
 *   - a beam one of whose four cell coordinates is not finite or not below 2^30 in size is skipped (n_skipped_beams):
 *     lfx_occupancy_follow does not inspect poses;
 *   - the line: integer Bresenham from (ox, oy) to (ex, ey) in 64-bit integers: ax = |ex-ox|, ay = |ey-oy|, sx, sy the signs,
 *     err = ax - ay; visit (x, y), stop when it is the end cell; e2 = 2*err; if (e2 > -ay) { err -= ay; x += sx; }
 *     if (e2 < ax) { err += ax; y += sy; } -- max(ax, ay) + 1 cells.  The cells before the end cell are PASSED, the last one is
 *     the END.  Cells outside the grid are left out silently: the ray is clipped, not dropped;
 *   - votes, at most one per cell and scan: a cell is OCCUPIED in scan k if it is the END of at least one HIT beam of k;
 *     otherwise FREE in k if any beam of k passed it or it is the END of a CLEAR beam (a hit beats a miss within a scan: a
 *     neighbouring beam that grazes a wall cell does not erase the wall).  hits[cell] += 1 for OCCUPIED, misses[cell] += 1 for
 *     FREE, both uint32.  The counts are a pure function of the beams and poses rendered; they do not depend on chunk_scans,
 *     the launch shape, the stream or the order of arrival.
 *   A render accumulates; lfx_occupancy_clear zeroes the counts and the counters.  A full re-render is a clear and a render of
 *   (0, n_scans).
 *
 * EMIT (lfx_occupancy_emit).  Per cell n = hits + misses; n < min_observations: -1.  Otherwise
 *   L = clamp((int64)hits * w_hit - (int64)misses * w_miss, l_min, l_max) and the cell is lut[L - l_min],
 *   lut[j] = (int8) rint(100.0 / (1.0 + exp(-(double)(l_min + j) / 100.0))) from lfx_occupancy_emit_table (host only, the ONLY
 *   source: the device is handed these bytes).  The defaults are OctoMap's log-odds in hundredths.  The output is int8
 *   [height][width], row 0 the lowest y: nav_msgs/OccupancyGrid.data.
 *
 * LIMITS.  The 2-D projection (the height band, the column) happens at the rotation of the pose the scan was added with: a
 * later rotation correction moves the end points but does not re-decide the band.  One vote per cell and scan, however many
 * beams cross the cell.  Feature-only stores (the keyframe store, the maps) cannot feed it.
 *
 * THE OBJECT.  lfx_occupancy_create allocates everything on the device: [max_scans][W] beams, [max_scans][12] double poses,
 * the two count arrays, the reduce's [chunk_scans][W][2] keys and the render's two bitmaps per scan of a chunk over a window of
 * side 2 * ceil(max_range * inv_res) + 5 cells around the scan's origin cell; no later call allocates device memory.  Calls
 * are ordered through one event behind the object's last call, whatever streams they were given (the keyframe store's rule,
 * with the same promises about caller-owned buffers).  LFX_ERR_INVALID_ARGUMENT and LFX_ERR_CAPACITY are returned before
 * anything is queued and leave the object as it was. */
#define LFX_OCCUPANCY_NONE 0
#define LFX_OCCUPANCY_HIT 1
#define LFX_OCCUPANCY_CLEAR 2
#define LFX_OCCUPANCY_MAX_BEAMS 4096
#define LFX_OCCUPANCY_MAX_SIDE 16384
typedef struct lfx_occupancy lfx_occupancy;
typedef struct lfx_occupancy_config {
  uint32_t n_beams;             /* W: 1800; even, 4 .. 4096 */
  uint32_t max_scans;           /* the caller sets it; 1 .. 2^24 */
  uint32_t width, height;       /* cells; the caller sets them; 1 .. 16384 */
  float resolution;             /* metres per cell; the caller sets it; finite, > 0 */
  float min_range, max_range;   /* 1.0, 100.0; 0 < min_range < max_range <= 65536 */
  float z_min, z_max;           /* -1.5, 0.5; finite, z_min <= z_max */
  uint32_t chunk_scans;         /* 32; 1 .. 1024 */
  double origin_x, origin_y;    /* the caller sets them; finite */
} lfx_occupancy_config;
typedef struct lfx_occupancy_emit_config {
  int32_t w_hit, w_miss;        /* 85, 40; 1 .. 1000 */
  int32_t l_min, l_max;         /* -200, 350; l_min < l_max, l_max - l_min <= 4096 */
  uint32_t min_observations;    /* 1; >= 1 */
  uint32_t reserved;            /* 0 */
} lfx_occupancy_emit_config;
typedef struct lfx_occupancy_info_t {
  uint32_t n_scans, max_scans, n_beams, width, height, chunk_scans;
  uint32_t window;              /* the side of a scan's window in cells */
  uint32_t reserved;
  uint64_t device_bytes;        /* everything lfx_occupancy_create allocated on the device */
} lfx_occupancy_info_t;
typedef struct lfx_occupancy_view_t {
  const float *beams;           /* device [n_scans][W][4]: x, y, z and the kind's bits */
  const double *poses;          /* device [n_scans][12] */
  const uint32_t *hits, *misses;   /* device [height][width] */
  uint32_t n_scans, reserved;
} lfx_occupancy_view_t;
typedef struct lfx_occupancy_counters_t {   /* of the renders since the last clear */
  uint64_t n_hit_beams, n_clear_beams;      /* beams cast, by kind */
  uint64_t n_skipped_beams;                 /* beams left out for a cell coordinate that is not finite or too large */
  uint64_t n_occupied_votes, n_free_votes;
  uint64_t n_window_miss;                   /* cells of the grid that fell outside their scan's window (guarded, not written): 0
                                               for poses whose rotation is one */
} lfx_occupancy_counters_t;
void lfx_occupancy_default_config(lfx_occupancy_config *config);
/* host only, no context: the column tables the kernels are given.  LFX_ERR_INVALID_ARGUMENT: NULL arguments and every field
 * outside the ranges above. */
int lfx_occupancy_tables(const lfx_occupancy_config *config, double *col_cos /*[W]*/, double *col_sin /*[W]*/);
void lfx_occupancy_emit_default_config(lfx_occupancy_emit_config *config);
/* host only: the emit's look-up table.  LFX_ERR_INVALID_ARGUMENT as above. */
int lfx_occupancy_emit_table(const lfx_occupancy_emit_config *config, int8_t *lut /*[l_max - l_min + 1]*/);
/* What lfx_occupancy_tables refuses is LFX_ERR_INVALID_ARGUMENT, a failed allocation LFX_ERR_OUT_OF_MEMORY with nothing left
 * allocated. */
int lfx_occupancy_create(lfx_ctx *ctx, const lfx_occupancy_config *config, lfx_occupancy **out);
void lfx_occupancy_destroy(lfx_occupancy *grid);
int lfx_occupancy_info(const lfx_occupancy *grid, lfx_occupancy_info_t *info);
/* The device arrays, current behind `stream`. */
int lfx_occupancy_view(lfx_ctx *ctx, const lfx_occupancy *grid, lfx_occupancy_view_t *view, void *stream);
/* The scans of the last device batch (whose INPUT records must still be alive, as for lfx_segment_batch) reduced to beams and
 * appended as scans *first_id .., each with its pose: poses host [n_scans][12], one per scan of the batch.  select (host
 * [n_scans], may be NULL) leaves out the scans whose byte is 0 -- keyframes are a subset of scans.  d_class (device, may be
 * NULL): lfx_segment_batch's classes for this batch, with obstacle_mask / clear_mask over LFX_SEG_*.  Asynchronous; the records
 * and classes are read behind `stream`: a caller that hands the context its next scans (lfx_extract uploads into the same
 * buffer on the context's own stream) waits for `stream` first, as after lfx_segment_batch.  LFX_ERR_INVALID_ARGUMENT: NULL ctx, grid or poses, a pose that is not finite, no batch
 * yet, n_scans not the last batch's, a mask bit above 3; LFX_ERR_CAPACITY: more scans selected than max_scans leaves room
 * for. */
int lfx_occupancy_add_batch(lfx_ctx *ctx, lfx_occupancy *grid, uint32_t n_scans, const double *poses, const uint8_t *select,
                            const uint8_t *d_class, uint32_t obstacle_mask, uint32_t clear_mask, uint32_t *first_id, void *stream);
/* The keyframe store's calls of these names: host poses in (finite) and out (synchronous), and poses taken device to device
 * from d_poses[first .. first + count) -- a pose graph's view -- without being inspected. */
int lfx_occupancy_set_poses(lfx_ctx *ctx, lfx_occupancy *grid, uint32_t first, uint32_t count, const double *poses, void *stream);
int lfx_occupancy_poses(lfx_ctx *ctx, const lfx_occupancy *grid, uint32_t first, uint32_t count, double *poses_out, void *stream);
int lfx_occupancy_follow(lfx_ctx *ctx, lfx_occupancy *grid, const double *d_poses, uint32_t first, uint32_t count, void *stream);
/* Drops the store's scans from n_scans on: the next lfx_occupancy_add_batch appends from id n_scans.  The counts are untouched
 * (what the dropped scans voted stays until a clear).  With it a second small grid (1 x 1 cells) serves as the reducer of live
 * batches for lfx_grid_match_set_scans_occupancy: truncate(0), add_batch, set_scans_occupancy.  n_scans above the store's:
 * LFX_ERR_INVALID_ARGUMENT. */
int lfx_occupancy_truncate(lfx_ctx *ctx, lfx_occupancy *grid, uint32_t n_scans, void *stream);
/* Zeroes the counts and the counters; asynchronous. */
int lfx_occupancy_clear(lfx_ctx *ctx, lfx_occupancy *grid, void *stream);
/* The votes of scans [first, first + count) at their current poses added to the counts; asynchronous.  Scans outside the
 * store: LFX_ERR_INVALID_ARGUMENT. */
int lfx_occupancy_render(lfx_ctx *ctx, lfx_occupancy *grid, uint32_t first, uint32_t count, void *stream);
/* Synchronous: the counters of the renders since the last clear. */
int lfx_occupancy_counters(lfx_ctx *ctx, const lfx_occupancy *grid, lfx_occupancy_counters_t *counters, void *stream);
/* The grid as int8 [height][width] to out: device memory or a pinned block (lfx_host_alloc); asynchronous.  A new emit config's
 * table goes up from a pinned block of the object's, after a wait for the object's last call; the config of the call before
 * is not sent again.  LFX_ERR_INVALID_ARGUMENT: NULL arguments, what lfx_occupancy_emit_table refuses. */
int lfx_occupancy_emit(lfx_ctx *ctx, lfx_occupancy *grid, const lfx_occupancy_emit_config *config, int8_t *out, void *stream);
/* host only, no context: dirname/map.pgm (P5, maxval 255, the top row the highest y; a cell of -1 is 205, a cell >=
 * occupied_percent 0, a cell <= free_percent 254, anything else 205) and dirname/map.yaml (image: map.pgm, resolution, origin:
 * [x, y, 0.0], negate: 0, occupied_thresh and free_thresh as percent / 100; doubles as %.17g) as map_server reads them.
 * LFX_ERR_INVALID_ARGUMENT: NULL arguments, w or h outside 1 .. 16384, a resolution that is not finite and > 0, an origin that is
 * not finite, percents that are not 0 <= free_percent < occupied_percent <= 100; LFX_ERR_FILE: a file cannot be written. */
int lfx_occupancy_write_map(const char *dirname, const int8_t *grid, uint32_t w, uint32_t h, float resolution, double origin_x,
                            double origin_y, int occupied_percent, int free_percent);
/* An emit through a pinned block of the object's (host memory, allocated on first use) and lfx_occupancy_write_map of it with the
 * grid's own resolution and origin.  Synchronous. */
int lfx_occupancy_save(lfx_ctx *ctx, lfx_occupancy *grid, const lfx_occupancy_emit_config *config, const char *dirname,
                       int occupied_percent, int free_percent, void *stream);

/* --- distance fields and costmaps of occupancy grids ------------------------------------------------------------------------ */
/* What a planner plans on: the squared distance from every cell to the nearest obstacle cell (an ESDF once rooted and scaled)
 * and nav2's inflated costmap.  No reference counterpart; the models are the exact separable Euclidean distance transform
 * (Felzenszwalb & Huttenlocher 2012) and costmap_2d::InflationLayer.  Integer arithmetic only up to lfx_distance_metres: the
 * same grid gives the same bytes, whatever the schedule, and the result is exact for every input -- nothing is propagated
 * approximately.  Ties need no rule: only the distance is reported.
 *
 * SOURCE.  G is int8 [H][W] in lfx_occupancy_emit's format: -1 unknown, 0 .. 100 percent, row 0 the lowest y; 1 <= W, H <=
 *   LFX_OCCUPANCY_MAX_SIDE.  lfx_distance_from_occupancy takes for G exactly the bytes lfx_occupancy_emit would write with the
 *   same emit config, computed from the counts in passing: no int8 grid exists in between.
 *
 * CLASSES, one byte per cell: LFX_DISTANCE_OBSTACLE iff G >= occupied_percent || (G < 0 && unknown_is_obstacle); otherwise
 *   LFX_DISTANCE_UNKNOWN iff G < 0; otherwise LFX_DISTANCE_FREE.
 *
 * FIELDS, uint32 [H][W].  d2[y][x] = the minimum over OBSTACLE cells (x', y') of (x-x')^2 + (y-y')^2; LFX_DISTANCE_FAR if the
 *   grid has no obstacle.  With a cap R = max_cells > 0 a minimum above R*R is LFX_DISTANCE_FAR (R*R itself is kept).  i2, only
 *   with `inside`: the same with the cells that are NOT obstacles for sites, so 0 on them; FAR if there is none, FAR above R*R.
 *   The largest value is 2 * 16383^2.
 *
 * METRES (lfx_distance_metres), float [H][W], res = (double)resolution:
 *   a cell that is no obstacle: d2 FAR: +INFINITY, otherwise (float)(sqrt((double)d2) * res), the square root correctly rounded;
 *   an obstacle: without `inside` 0.0f; with it i2 FAR: -INFINITY, otherwise -(float)(sqrt((double)i2) * res).
 *
 * COST TABLE (lfx_distance_cost_table: host only, the ONLY source of the decay; the device is handed these bytes).
 *   Rc = (uint32)ceil((double)inflation_radius / (double)resolution), at most LFX_DISTANCE_MAX_COST_CELLS; n = Rc*Rc + 1;
 *   lut[0] = 254; for k >= 1 with d = sqrt((double)k) * (double)resolution: d <= (double)inscribed_radius: 253;
 *   d > (double)inflation_radius: 0; otherwise (uint8)(252.0 * exp(-(double)cost_scaling_factor * (d - (double)inscribed_radius)))
 *   (truncated: nav2's expression).
 *
 * COSTMAP (lfx_distance_costmap), uint8 [H][W]: an OBSTACLE is 254; otherwise an UNKNOWN cell with track_unknown is 255;
 *   otherwise d2 FAR or d2 > Rc*Rc is 0; otherwise lut[d2].  The last transform must have had max_cells 0 or >= Rc.
 *
 * THE OBJECT.  lfx_distance_create allocates everything on the device: the classes, one 64-bit obstacle mask per column and
 * 64 rows with two carries, the uint16 column distances, d2, i2, the largest cost table (1024^2 + 1 bytes) and four stats
 * words; no later call allocates device memory.  Calls are ordered through one event behind the object's last call, whatever
 * streams they were given (the keyframe store's rule, with the same promises about caller-owned buffers).
 * LFX_ERR_INVALID_ARGUMENT is returned before anything is queued and leaves the object, the last transform's fields included,
 * as it was: NULL arguments, a config out of range, metres / costmap / stats before any transform, a resolution that is not
 * finite and > 0.
 *
 * LIMITS.  A transform always rebuilds the whole field.  An uncapped transform, or one capped above 64 cells, costs
 * log2(W) + 1 passes over each row whatever the grid holds; a cap of up to 64 cells takes a search of at most R columns per
 * cell instead.  The costmap inflates by a circle: no footprint. */
#define LFX_DISTANCE_FAR 0xFFFFFFFFu
#define LFX_DISTANCE_FREE 0
#define LFX_DISTANCE_UNKNOWN 1
#define LFX_DISTANCE_OBSTACLE 2
#define LFX_DISTANCE_MAX_COST_CELLS 1024
typedef struct lfx_distance lfx_distance;
typedef struct lfx_distance_config {
  int32_t occupied_percent;     /* 65; 1 .. 100 */
  uint32_t unknown_is_obstacle; /* 0; 0 / 1 */
  uint32_t max_cells;           /* R: 0 = uncapped, else 1 .. 32767 */
  uint32_t inside;              /* 0; 0 / 1: compute i2 */
  uint32_t reserved;            /* 0 */
} lfx_distance_config;
typedef struct lfx_distance_cost_config {
  float inscribed_radius;       /* 0.22; finite, >= 0 */
  float inflation_radius;       /* 0.55; finite, >= inscribed_radius */
  float cost_scaling_factor;    /* 10.0; finite, >= 0 */
  uint32_t track_unknown;       /* 1; 0 / 1 */
} lfx_distance_cost_config;
typedef struct lfx_distance_info_t {
  uint32_t width, height;
  uint32_t transformed;         /* whether a transform has run; the next two are its config's */
  uint32_t max_cells, inside;
  uint32_t reserved;
  uint64_t device_bytes;        /* everything lfx_distance_create allocated on the device */
} lfx_distance_info_t;
typedef struct lfx_distance_view_t {
  const uint8_t *classes;       /* device [height][width] */
  const uint32_t *d2;           /* device [height][width] */
  const uint32_t *i2;           /* device [height][width]; NULL unless the last transform had `inside` */
} lfx_distance_view_t;
typedef struct lfx_distance_stats_t {   /* of the last transform */
  uint64_t n_obstacle, n_unknown;       /* cells by class */
  uint64_t n_far;                       /* cells whose d2 is FAR */
  uint64_t max_d2;                      /* over the cells whose d2 is not FAR; 0 if there is none */
} lfx_distance_stats_t;
void lfx_distance_default_config(lfx_distance_config *config);
void lfx_distance_cost_default_config(lfx_distance_cost_config *config);
/* host only, no context: n = Rc*Rc + 1.  LFX_ERR_INVALID_ARGUMENT: NULL arguments, a field outside the ranges above, a
 * resolution that is not finite and > 0, Rc above LFX_DISTANCE_MAX_COST_CELLS. */
int lfx_distance_cost_table_size(const lfx_distance_cost_config *config, float resolution, uint32_t *n);
/* host only, no context: the table.  LFX_ERR_INVALID_ARGUMENT as above, and n that is not lfx_distance_cost_table_size's. */
int lfx_distance_cost_table(const lfx_distance_cost_config *config, float resolution, uint8_t *lut /*[n]*/, uint32_t n);
/* width and height outside 1 .. LFX_OCCUPANCY_MAX_SIDE: LFX_ERR_INVALID_ARGUMENT; a failed allocation: LFX_ERR_OUT_OF_MEMORY
 * with nothing left allocated. */
int lfx_distance_create(lfx_ctx *ctx, uint32_t width, uint32_t height, lfx_distance **out);
void lfx_distance_destroy(lfx_distance *field);
int lfx_distance_info(const lfx_distance *field, lfx_distance_info_t *info);
/* The transform of a device grid, int8 [height][width]; asynchronous, d_grid is read behind `stream`. */
int lfx_distance_from_grid(lfx_ctx *ctx, lfx_distance *field, const int8_t *d_grid, const lfx_distance_config *config, void *stream);
/* The transform of an occupancy grid's counts as they stand: the bytes of lfx_occupancy_emit(emit_config) into a buffer and
 * lfx_distance_from_grid of it.  Ordered behind the occupancy grid's last call, whose event moves behind this read (the store's
 * rule for a reader); a new emit config's table goes up as for lfx_occupancy_emit.  LFX_ERR_INVALID_ARGUMENT also: a grid whose
 * width or height is not the field's, what lfx_occupancy_emit_table refuses. */
int lfx_distance_from_occupancy(lfx_ctx *ctx, lfx_distance *field, lfx_occupancy *grid, const lfx_occupancy_emit_config *emit_config,
                                const lfx_distance_config *config, void *stream);
/* The device arrays, current behind `stream`. */
int lfx_distance_view(lfx_ctx *ctx, const lfx_distance *field, lfx_distance_view_t *view, void *stream);
/* float [height][width] to out: device memory or a pinned block (lfx_host_alloc); asynchronous. */
int lfx_distance_metres(lfx_ctx *ctx, lfx_distance *field, float resolution, float *out, void *stream);
/* uint8 [height][width] to out: device memory or a pinned block; asynchronous.  A new (cost config, resolution)'s table goes up
 * from a pinned block of the object's, after a wait for the object's last call; the one of the call before is not sent again.
 * LFX_ERR_INVALID_ARGUMENT also: what lfx_distance_cost_table_size refuses, a last transform with 0 < max_cells < Rc. */
int lfx_distance_costmap(lfx_ctx *ctx, lfx_distance *field, const lfx_distance_cost_config *config, float resolution, uint8_t *out,
                         void *stream);
/* Synchronous: integer reductions, the same numbers whatever the schedule. */
int lfx_distance_stats(lfx_ctx *ctx, const lfx_distance *field, lfx_distance_stats_t *stats, void *stream);

/* --- scan matching in occupancy grids: where a scan is in the map ------------------------------------------------------------ */
/* What a 2-D stack localises with: the likelihood field of the grid (AMCL's likelihood_field model) scored for arbitrary poses
 * -- a particle filter's measurement update -- and searched exhaustively over a window of (x, y, yaw) -- Olson's and
 * Cartographer's correlative scan matcher, for relocalisation, tracking and a 2-D loop check.  No reference counterpart.  The
 * pose found is the initial pose lfx_localize_batch, the rolling map and lfx_loop_closer_verify ask for
 * (lfx_grid_match_pose3).  Everything below is double, unfused, unless stated; scores are integers throughout: the same field,
 * scans and candidates give the same bytes, whatever the schedule.  The device evaluates no trigonometric function.
 *
 * CONFIG.  width, height, resolution, origin_x, origin_y with the meaning and ranges of lfx_occupancy_config (lfx_distance
 *   carries no geometry, so the matcher does); inv_res = 1.0 / (double)resolution.  max_scans 1 .. 1024, max_beams 4 ..
 *   LFX_OCCUPANCY_MAX_BEAMS, max_half_x and max_half_y 0 .. LFX_GRID_MATCH_MAX_HALF cells, max_half_theta 0 ..
 *   LFX_GRID_MATCH_MAX_HALF_THETA steps.
 *
 * SCORE TABLE (lfx_grid_match_table: host only, the ONLY source; the device is handed these bytes).
 *   Rs = (uint32)ceil((double)max_distance / (double)resolution), at most LFX_GRID_MATCH_MAX_CELLS; n = Rs*Rs + 1; for k = 0 ..
 *   Rs*Rs with d = sqrt((double)k) * (double)resolution: d > (double)max_distance: lut[k] = 0; otherwise
 *   lut[k] = (uint16)rint((double)peak * exp(-(d*d) / ((2.0 * (double)sigma) * (double)sigma))).  A caller may hand any uint16
 *   table of a legal size (Rs*Rs + 1 entries, Rs in 0 .. 64) instead, fixed-point log-likelihoods for one.
 *
 * FIELD (lfx_grid_match_set_field), S uint16 [H][W] from a distance field's d2: S[y][x] = 0 where d2 is LFX_DISTANCE_FAR or
 *   d2 >= n, otherwise lut[d2].  The last transform must have had max_cells 0 or >= Rs (the costmap's rule).
 *
 * SCANS (lfx_grid_match_set_scans).  Beams are lfx_occupancy_view_t.beams; only those whose kind bits are LFX_OCCUPANCY_HIT
 *   take part.  With the scan's level l[9] (row-major 3 x 3; NULL: identity) and the beam's x, y, z as doubles:
 *   px = (l0*x + l1*y) + l2*z, py = (l3*x + l4*y) + l5*z; a beam whose px or py is not finite is left out.  n_points[s] is the
 *   number kept.  The points are a multiset (the sums are integer); they are kept compacted, in beam order.
 *   lfx_grid_match_set_scans_occupancy takes a store's scans with the rotations of the poses the store holds NOW for levels,
 *   read on the device: with the stored (t_x, t_y) as candidate at c = 1, s = 0 the cells below are exactly
 *   lfx_occupancy_render's end cells.
 *
 * CANDIDATE.  (tx, ty, c, s): the caller supplies the cosine and the sine.  For a point: wx = (c*px - s*py) + tx,
 *   wy = (s*px + c*py) + ty, ex = floor((wx - origin_x) * inv_res), ey = floor((wy - origin_y) * inv_res).  A point is OUTSIDE
 *   and adds 0 if ex or ey is not finite or not below 2^30 in size, or if (ex, ey) is no cell of the grid.
 *   score = the sum of S[ey][ex] over the scan's points in uint32 (at most 4096 * 65535 < 2^28); inside = the number of
 *   points whose cell is in the grid.
 *
 * SEARCH (lfx_grid_match_search).  Nx = 2*half_x + 1, Ny = 2*half_y + 1, T = 2*half_theta + 1.  The rotations come from
 *   lfx_grid_match_rotations (host only, the ONLY source: the call computes them and sends them up):
 *   angle_j = yaw0 + (double)(j - half_theta) * theta_step, c = cos(angle_j), s = sin(angle_j) by the host's libm (half_theta == 0: angle_0 = yaw0, theta_step is not read).  Per
 *   (scan, j) and point the base cell (bx, by) is the candidate arithmetic with tx = x0, ty = y0.  Candidate (j, iy, ix) scores
 *   the point at cell (bx + (ix - half_x)*step_cells, by + (iy - half_y)*step_cells): the scan is shifted by WHOLE CELLS (the
 *   correlative matcher's trick; this is the contract, and not the same as the score at x0 + k*resolution after rounding).  A
 *   point whose base cell is OUTSIDE by the size rule is outside for every shift.  index = (j*Ny + iy)*Nx + ix; the best is
 *   the greatest score, equal scores go to the lowest index, found with integer maxima over the 64-bit key
 *   (score << 32) | (0xFFFFFFFF - index): no floating point anywhere.
 *
 * THE OBJECT.  lfx_grid_match_create allocates everything on the device: S, the largest table, [max_scans][max_beams] points
 *   and their counts, the search's keys and a ring of rotation tables; no later call allocates device memory.  Calls are
 *   ordered through one event behind the object's last call, whatever streams they were given (the keyframe store's rule, with
 *   the same promises about caller-owned buffers).  LFX_ERR_INVALID_ARGUMENT and LFX_ERR_CAPACITY are returned before anything
 *   is queued and leave the object as it was.
 *
 * LIMITS.  The search is exhaustive: no multi-resolution branch and bound.  Translation moves in whole cells times step_cells;
 * sub-cell refinement is the caller's, or the 3-D alignment's that follows.  Only HIT beams score: free-space evidence is
 * unused.  The level is fixed per scan.  One field per object. */
#define LFX_GRID_MATCH_MAX_CELLS 64
#define LFX_GRID_MATCH_MAX_HALF 256
#define LFX_GRID_MATCH_MAX_HALF_THETA 180
typedef struct lfx_grid_match lfx_grid_match;
typedef struct lfx_grid_match_config {
  uint32_t width, height;       /* cells; the caller sets them; 1 .. 16384 */
  float resolution;             /* metres per cell; the caller sets it; finite, > 0 */
  uint32_t max_scans;           /* 64; 1 .. 1024 */
  uint32_t max_beams;           /* 1800; 4 .. 4096 */
  uint32_t max_half_x, max_half_y;   /* 50, 50; 0 .. 256 cells */
  uint32_t max_half_theta;      /* 30; 0 .. 180 steps */
  double origin_x, origin_y;    /* the caller sets them; finite */
} lfx_grid_match_config;
typedef struct lfx_grid_match_table_config {
  float sigma;                  /* 0.2; finite, > 0 */
  float max_distance;           /* 2.0 (AMCL's laser_likelihood_max_dist); finite, >= 0 */
  uint32_t peak;                /* 1000; 1 .. 65535 */
  uint32_t reserved;            /* 0 */
} lfx_grid_match_table_config;
typedef struct lfx_grid_match_search_config {
  uint32_t half_x, half_y;      /* 10, 10; cells, within the object's maxima */
  uint32_t step_cells;          /* 1; 1 .. 16 */
  uint32_t half_theta;          /* 0; within the object's maximum */
  double theta_step;            /* 0.0; finite and > 0 unless half_theta == 0 */
} lfx_grid_match_search_config;
typedef struct lfx_grid_match_info_t {
  uint32_t width, height, max_scans, max_beams, max_half_x, max_half_y, max_half_theta;
  uint32_t field_set;           /* whether lfx_grid_match_set_field has run; table_cells is its table's Rs */
  uint32_t table_cells;
  uint32_t n_scans, n_beams;    /* of the last lfx_grid_match_set_scans*; 0 before any */
  uint32_t reserved;
  uint64_t device_bytes;        /* everything lfx_grid_match_create allocated on the device */
} lfx_grid_match_info_t;
typedef struct lfx_grid_match_view_t {
  const uint16_t *field;        /* device [height][width] */
  const double *points;         /* device [max_scans][max_beams][2]: scan s's first n_points[s] pairs */
  const uint32_t *n_points;     /* device [max_scans] */
} lfx_grid_match_view_t;
void lfx_grid_match_default_config(lfx_grid_match_config *config);
void lfx_grid_match_table_default_config(lfx_grid_match_table_config *config);
void lfx_grid_match_search_default_config(lfx_grid_match_search_config *config);
/* host only, no context: n = Rs*Rs + 1.  LFX_ERR_INVALID_ARGUMENT: NULL arguments, a field outside the ranges above, a
 * resolution that is not finite and > 0, Rs above LFX_GRID_MATCH_MAX_CELLS. */
int lfx_grid_match_table_size(const lfx_grid_match_table_config *config, float resolution, uint32_t *n);
/* host only, no context: the table.  LFX_ERR_INVALID_ARGUMENT as above, and n that is not lfx_grid_match_table_size's. */
int lfx_grid_match_table(const lfx_grid_match_table_config *config, float resolution, uint16_t *lut /*[n]*/, uint32_t n);
/* host only: dims = {Nx, Ny, T}.  LFX_ERR_INVALID_ARGUMENT: NULL arguments, half_x or half_y above LFX_GRID_MATCH_MAX_HALF,
 * half_theta above LFX_GRID_MATCH_MAX_HALF_THETA, step_cells outside 1 .. 16, with half_theta > 0 a theta_step that is not
 * finite and > 0. */
int lfx_grid_match_search_size(const lfx_grid_match_search_config *search, uint32_t dims[3]);
/* host only: the search's rotations, cs [2*half_theta + 1][2] = {cos, sin} of angle_j.  LFX_ERR_INVALID_ARGUMENT: NULL cs, a
 * yaw0 that is not finite, half_theta above the maximum, with half_theta > 0 a theta_step that is not finite and > 0. */
int lfx_grid_match_rotations(double yaw0, uint32_t half_theta, double theta_step, double *cs);
/* host only: the pose of candidate `index` of a search around centre {x0, y0, yaw0}: pose2 = {x0 + (double)((ix - half_x) *
 * step_cells) * (double)resolution, y0 + (double)((iy - half_y) * step_cells) * (double)resolution, angle_j}.
 * LFX_ERR_INVALID_ARGUMENT: what lfx_grid_match_search_size refuses, an index that is not below T*Ny*Nx, a resolution or a
 * centre that is not finite. */
int lfx_grid_match_candidate(const lfx_grid_match_search_config *search, float resolution, const double centre[3], uint32_t index,
                             double pose2[3]);
/* host only: pose [3][4] = [Rz(yaw) x level | (x, y, z)] of pose2 = {x, y, yaw}; level [9] row-major or NULL = identity.  The
 * initial pose lfx_localize_batch asks for.  Each element of the product is ((a*b + c*d) + e*f) in this order. */
int lfx_grid_match_pose3(const double pose2[3], const double *level, double z, double pose[12]);
/* A config outside the ranges above: LFX_ERR_INVALID_ARGUMENT; a failed allocation: LFX_ERR_OUT_OF_MEMORY with nothing left
 * allocated. */
int lfx_grid_match_create(lfx_ctx *ctx, const lfx_grid_match_config *config, lfx_grid_match **out);
void lfx_grid_match_destroy(lfx_grid_match *matcher);
int lfx_grid_match_info(const lfx_grid_match *matcher, lfx_grid_match_info_t *info);
/* The device arrays, current behind `stream`. */
int lfx_grid_match_view(lfx_ctx *ctx, const lfx_grid_match *matcher, lfx_grid_match_view_t *view, void *stream);
/* S from the field's d2 and the table lut [n] (host); asynchronous.  The field is read behind its own event, which moves behind
 * the read (the store's rule for a reader); the table goes up from a pinned block of the object's, after a wait for the
 * object's last call.  LFX_ERR_INVALID_ARGUMENT: NULL arguments, a field whose sides are not the matcher's, a field without a
 * transform, n that is not Rs*Rs + 1 for an Rs in 0 .. 64, a last transform with 0 < max_cells < Rs. */
int lfx_grid_match_set_field(lfx_ctx *ctx, lfx_grid_match *matcher, lfx_distance *field, const uint16_t *lut, uint32_t n, void *stream);
/* Scans 0 .. n_scans - 1 of the object from d_beams, device [n_scans][n_beams][4] as lfx_occupancy_view_t.beams, read behind
 * `stream`; levels host [n_scans][9] or NULL = identity (not inspected).  Replaces every scan the object held; asynchronous.
 * LFX_ERR_INVALID_ARGUMENT: NULL arguments, n_scans 0, n_beams 0; LFX_ERR_CAPACITY: n_scans above max_scans, n_beams above
 * max_beams. */
int lfx_grid_match_set_scans(lfx_ctx *ctx, lfx_grid_match *matcher, const float *d_beams, uint32_t n_scans, uint32_t n_beams,
                             const double *levels, void *stream);
/* The same of an occupancy store's scans [first, first + count), the levels the rotations of the poses the store holds now
 * (use_rotation 0: identity).  Ordered behind the store's last call, whose event moves behind this read. */
int lfx_grid_match_set_scans_occupancy(lfx_ctx *ctx, lfx_grid_match *matcher, lfx_occupancy *grid, uint32_t first, uint32_t count,
                                       int use_rotation, void *stream);
/* score and inside of scan `scan` at the P candidates d_candidates, device double [P][4] = {tx, ty, c, s}, to d_score uint32
 * [P] and d_inside uint32 [P] (may be NULL), all device memory; 1 <= P <= 2^24; asynchronous.  LFX_ERR_INVALID_ARGUMENT also: no
 * field yet, a scan that is not set. */
int lfx_grid_match_score(lfx_ctx *ctx, lfx_grid_match *matcher, uint32_t scan, const double *d_candidates, uint32_t n_candidates,
                         uint32_t *d_score, uint32_t *d_inside, void *stream);
/* The window of `search` around centres host [n_scans][3] = {x0, y0, yaw0}, one per scan of [first, first + n_scans); outputs
 * on the device: d_best uint32 [n_scans][4] = {score, index, inside, n_points}; d_slice_best (may be NULL) uint32 [n_scans][T][2]
 * = {score, index}, the best of each heading under the same tie rule; d_volume (may be NULL) uint32 [n_scans][T][Ny][Nx].
 * Asynchronous; the rotations go up through a ring of pinned blocks of the object's.  LFX_ERR_INVALID_ARGUMENT also: no field
 * yet, scans that are not set, a centre that is not finite, what lfx_grid_match_search_size refuses; LFX_ERR_CAPACITY: a
 * window beyond the object's maxima. */
int lfx_grid_match_search(lfx_ctx *ctx, lfx_grid_match *matcher, uint32_t first, uint32_t n_scans, const double *centres,
                          const lfx_grid_match_search_config *search, uint32_t *d_best, uint32_t *d_slice_best, uint32_t *d_volume,
                          void *stream);

/* --- per-stage entry points (device-backed mirrors of the reference's free functions) ----- */
/* One ring given as angle-sorted x[n], y[n] host arrays; every stage runs the same device
 * routines the fused ring kernel runs.  Optional inputs may be NULL.
 *   groups     replaces the XY neighbour test by NeighborCheckDebug (neighbor.hpp:116-136)
 *   curvature_in  use these values instead of computing them (EdgeLabel/SurfaceLabel tests)
 * flags select what runs; outputs may be NULL. */
#define LFX_STAGE_LABEL 1u          /* AssignLabel              label.hpp:141-164          */
#define LFX_STAGE_OCCLUSION 2u      /* LabelOccludedPoints      occlusion.hpp:81-91        */
#define LFX_STAGE_OUT_OF_RANGE 4u   /* LabelOutOfRange          out_of_range.hpp:36-48     */
#define LFX_STAGE_PARALLEL_BEAM 8u  /* LabelParallelBeamPoints  parallel_beam.hpp:36-51    */
#define LFX_STAGE_SINGLE_BLOCK 16u  /* label the whole array as one block without borders (EdgeLabel::Assign, label.hpp:72-95) */
#define LFX_STAGE_CURVATURE 32u     /* CalcCurvature must succeed (N >= 2P+1)  curvature.cpp:44-50 */
#define LFX_STAGE_ALL 47u           /* what the fused ring kernel runs */
int lfx_stage_ring(lfx_ctx *ctx, const lfx_params *params, uint32_t flags, uint32_t n, const float *x,
                   const float *y, const int32_t *groups, const double *curvature_in,
                   const double *range_in /* use these ranges instead of sqrt(x^2+y^2) (CalcCurvature tests) */,
                   double *range_out /* [n]  Range, range.hpp:45-74 */,
                   double *curvature_out /* [n]  CalcCurvature, curvature.cpp:44-50 */,
                   uint8_t *link_out /* [n-1] IsNeighborXY(i,i+1), neighbor.hpp:44-48 */,
                   uint8_t *labels_out /* [n] */, int32_t *ring_status_out);
/* Convolution1D (convolution.cpp:35-66) for any odd weight; returns LFX_ERR_INVALID_ARGUMENT where the reference throws. */
int lfx_stage_convolution1d(lfx_ctx *ctx, const double *input, uint32_t n, const double *weight, uint32_t m,
                            double *out);
/* ExtractAngleSortedRings (ring.hpp:141-147) alone: per-ring angle-sorted original indices. */
int lfx_stage_ring_projection(lfx_ctx *ctx, const void *points, size_t n_points, uint32_t *sorted_index,
                              uint32_t *n_rings, uint16_t *ring_id /* [256] */, uint32_t *ring_count /* [256] */);

/* --- colored_scan (debug cloud of the node, feature_extraction.cpp:153,161) ---------------- */
/* LabelToColor, extraction/src/color_points.cpp:39-68: rgb of one PointLabel; returns
 * LFX_ERR_INVALID_ARGUMENT for a value that is not a label (the reference throws). */
int lfx_label_to_color(uint8_t label, uint8_t rgb[3]);
/* ColorPointsByLabel (color_points.hpp:60-74) for a whole scan on the host: out[i] = {x, y, z, rgb packed
 * as PCL does (0xFF << 24 | r << 16 | g << 8 | b, bit-cast to float; a = 255 is PointXYZRGB's default)} for input point i, from the labels lfx_extract
 * returned.  points: the scan's records (layout as given to lfx_create); out: n_points * 4 floats. */
int lfx_color_points_by_label(const lfx_ctx *ctx, const void *points, size_t n_points, const uint8_t *labels,
                              float *out);

/* --- the route selection, as a function ---------------------------------------------------- */
/* Which kernels a batch is given depends on what the batches before it reported about the stream (organised scans are read
 * in place, anything else is bucketed first; rotated / reversed rings get their transforms found first; see
 * INTEGRATION.md 3).  This is that decision with nothing around it -- no context, no device: `report` = the counters a
 * batch leaves behind ([0] rings deferred by the first unit pass, [1] repaired after it, [2] sent to the workgroup-per-ring
 * kernel, [3] repaired before it, [4] scans on the fall-back list, [5] whether the organised-scan kernel ran, [6] scans in
 * the batch, [7] scans given up for the angle order of their rings alone, [8] rings found rotated / reversed, [9] whether
 * the transforms were looked for, [10] scans given up for a (0, 0, 0) record alone (zero filter on), [11] whether the holes
 * form ran, [12] ring groups that held such a record then), `report_rings` = rings of that batch (0 = no report yet),
 * `state` in and out = {rings transformed, every scan bucketed, batches until the organised route is tried again, order
 * repair first, grid with holes}, `choice` out = {organised-scan kernel first, with ring transforms, fall-back list entries
 * launched for, one-launch tail, order repair before the first unit pass, rings the second unit pass is launched for, the
 * holes form (count pass first)}.  `organised_possible`: bit 0 = the organised-scan kernel can run (ring ids 0 .. n - 1, the
 * canonical record layout); LFX_ROUTE_NO_HOLES_FORM beside it = the context cannot run the holes form (no zero filter, or
 * long rings), so the flag is never kept.  tests/test_route_choice.py drives it row by row, tests/test_route_streams.py over
 * whole streams. */
#define LFX_ROUTE_NO_HOLES_FORM 2
#define LFX_ROUTE_REPORT_WORDS 14
#define LFX_ROUTE_STATE_WORDS 5
#define LFX_ROUTE_CHOICE_WORDS 7
int lfx_route_choice(const uint32_t report[LFX_ROUTE_REPORT_WORDS], uint32_t report_rings, uint32_t state[LFX_ROUTE_STATE_WORDS],
                     int organised_possible, uint32_t batch, uint32_t max_rings, uint32_t choice[LFX_ROUTE_CHOICE_WORDS]);

/* --- measurement ------------------------------------------------------------------------- */
#define LFX_N_KERNELS 24  /* ring_scatter, ring_unit, ring_order, ring_unit (second pass), ring_extract (the bucketing route), ring_totals, feature_compact (compaction), ring_unit_org (organised scans), ring_cut (transforms of rotated / reversed rings), fallback_tail (the organised route's tail), grid_count (valid returns per ring and column piece of a grid with holes), batch_reset, ring_long (rings longer than LFX_MAX_RING_POINTS), then the pose graph's: linearize, node (gradient and P's blocks), reduce, chain_factor, chain_solve, s_assemble, s_diag, s_panel, s_update, s_solve, step */
int lfx_set_profiling(lfx_ctx *ctx, int enabled);
/* Record the events around every n-th batch only (default 1; the pose graph's kernels have no batches and are timed in
 * every lfx_pose_graph_optimize while profiling is on).  The event pairs between the kernels of a batch
 * cost ~7 % of the device-resident throughput at 64x1800x256; sampled, the durations stay live and the cost goes. */
int lfx_set_profiling_interval(lfx_ctx *ctx, uint32_t every_n_batches);
/* Sum of HIP-event durations per kernel since profiling was enabled, and launches counted. */
int lfx_kernel_times(lfx_ctx *ctx, double ms[LFX_N_KERNELS], uint64_t launches[LFX_N_KERNELS]);
const char *lfx_kernel_name(int k);
/* What THIS device gives at this moment, so that a rate measured on it can be told from a rate measured on another box of the
 * same model: copy_gbs = bytes read + bytes written per second by a plain float4 copy of `bytes` bytes (0: 1 GiB), the best
 * of three; clock_mhz = the shader clock a wave sees while every SIMD of the device runs a chain of dependent 32-bit adds
 * (a SIMD-32 takes a wave in two cycles, four waves share it).  Allocates and frees 2 x bytes of device memory; about 10 ms; on `stream` (a hipStream_t, or NULL). */
int lfx_box_calibration(lfx_ctx *ctx, size_t bytes, void *stream, double *copy_gbs, double *clock_mhz);

#ifdef __cplusplus
}
#endif
#endif  /* LFX_H_ */
