// lfx.hpp -- C++ host side over the C ABI (lfx.h): what a maintainer of the reference node calls.
//
// The reference operator is the body of FeatureExtraction::Callback,
// /root/reference/extraction/app/feature_extraction.cpp:114-157; this header gives it a name,
// lfx::FeatureExtraction::ExtractFeatures(cloud), with the reference's types: PointXYZIR in
// (lib/include/lidar_feature_library/point_type.hpp:62-86), edge and surface PointXYZIR clouds out
// (intensity = (float)curvature, label.hpp:166-179), plus the per-point labels and curvature.
// Header only; link with liblfx.so.  Errors of the C ABI become lfx::Error; per-ring conditions
// the reference reports with RCLCPP_WARN (feature_extraction.cpp:154-156) are in ring_status.
#ifndef LFX_HPP_
#define LFX_HPP_

#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "lfx.h"

namespace lfx
{

struct alignas(16) PointXYZIR   // same 32-byte layout as the reference's PCL point type
{
  float x, y, z, pad;
  float intensity;
  std::uint16_t ring;
  std::uint8_t reserved[10];
};
static_assert(sizeof(PointXYZIR) == 32, "PointXYZIR must be 32 bytes");

struct Error : std::runtime_error
{
  Error(int c, const std::string & what)
  : std::runtime_error(what), code(c) {}
  int code;
};

struct HyperParameters : lfx_params   // hyper_parameter.hpp:32-65
{
  HyperParameters() {lfx_default_params(this);}
  static HyperParameters LaunchYaml() {HyperParameters p; lfx_launch_params(&p); return p;}
};

struct RingInfo
{
  std::uint16_t id;
  std::uint32_t count, offset;
  lfx_ring_status status;
};

struct Features
{
  std::vector<PointXYZIR> edge, surface;        // rings ascending, angle ascending inside a ring
  std::vector<std::uint32_t> edge_index, surface_index;   // original point indices
  std::vector<std::uint8_t> labels;             // PointLabel per input point (point_label.hpp:32-42)
  std::vector<double> curvature;                // per input point
  std::vector<std::uint32_t> sorted_index;      // ExtractAngleSortedRings, ring.hpp:141-147
  std::vector<RingInfo> rings;
};

// The sensor's poses within one sweep (lfx_trajectory; include/lfx.h, the de-skew section): 2 .. 64 knots with strictly
// ascending times, every pose [R | t] row-major in ONE fixed frame; the records are brought to the sensor frame at t_ref.
struct Trajectory
{
  std::vector<double> times;      // [k]: seconds with a time field, fractions of the sweep with TimeField::FromIndex()
  std::vector<double> poses;      // [k][12]
  double t_ref = 0.0;
  // Knots from gyro samples (lfx_trajectory_from_gyro): rates [k][3] rad/s in the sensor frame, the first pose the identity
  static Trajectory FromGyro(
    const std::vector<double> & times, const std::vector<double> & rates, double t_ref, const double * bias = nullptr,
    const double * velocity = nullptr)
  {
    Trajectory out;
    out.times = times;
    out.poses.assign(12 * times.size(), 0.0);
    out.t_ref = t_ref;
    if (rates.size() != 3 * times.size() ||
      lfx_trajectory_from_gyro(times.data(), rates.data(), static_cast<std::uint32_t>(times.size()), bias, velocity, out.poses.data()) != LFX_OK)
    {
      throw Error(LFX_ERR_INVALID_ARGUMENT, "invalid gyro samples");
    }
    return out;
  }
  // (points into this object: valid while it lives unchanged)
  lfx_trajectory View() const
  {
    if (poses.size() != 12 * times.size()) {throw Error(LFX_ERR_INVALID_ARGUMENT, "a trajectory holds 12 pose values per time");}
    return lfx_trajectory{static_cast<std::uint32_t>(times.size()), times.data(), poses.data(), t_ref};
  }
};
inline std::vector<lfx_trajectory> Views(const std::vector<Trajectory> & trajectories)
{
  std::vector<lfx_trajectory> out;
  for (const Trajectory & t : trajectories) {out.push_back(t.View());}
  return out;
}

class FeatureExtraction
{
public:
  // max_rings: the sensor's ring count (ring ids 0 .. max_rings-1).  Given, a driver's column-major scan is read in
  // place by the organised-scan kernel (no bucketing pass); 0 = unknown (256 ring ids, every scan is bucketed).
  // outputs: LFX_OUT_* mask of the per-point arrays to bring back besides the two clouds; what the node publishes
  // (feature_extraction.cpp:161-170) needs none of them, its colored_scan debug cloud needs LFX_OUT_LABELS.
  explicit FeatureExtraction(
    const HyperParameters & params = HyperParameters(), int device = 0,
    std::uint32_t max_points_per_scan = 262144, std::uint32_t max_points_per_ring = 0,
    std::uint32_t max_rings = 0, std::uint32_t outputs = LFX_OUT_ALL)
  {
    lfx_config cfg{};
    cfg.struct_size = sizeof(cfg);
    cfg.max_points_per_scan = max_points_per_scan;
    cfg.max_batch = 1;
    cfg.max_points_per_ring = max_points_per_ring;
    cfg.max_rings = max_rings;
    cfg.outputs = outputs;
    const int rc = lfx_create(&ctx_, device, &params, &cfg);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(nullptr));}
    max_points_ = max_points_per_scan;
  }
  ~FeatureExtraction()
  {
    for (void * p : pinned_) {lfx_host_free(ctx_, p);}
    lfx_destroy(ctx_);
  }
  FeatureExtraction(const FeatureExtraction &) = delete;
  FeatureExtraction & operator=(const FeatureExtraction &) = delete;

  // The sensor's ring ids where they are not 0 .. rings-1 (the reference buckets by whatever uint16 a point carries,
  // ring.hpp:114-125).  ExtractFeatures finds them by itself; a caller that knows them spares the first scan a second run.
  void SetRingIds(const std::vector<std::uint16_t> & ids) const
  {
    const int rc = lfx_set_ring_ids(ctx_, ids.empty() ? nullptr : ids.data(), static_cast<std::uint32_t>(ids.size()));
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
  }

  // A point buffer in pinned host memory, owned by this object: lfx_extract reads it by DMA (a buffer from anywhere
  // else is first copied through the context's staging buffer).  Let GetPointCloud fill it.
  PointXYZIR * PinnedPoints(std::size_t capacity)
  {
    void * p = nullptr;
    const int rc = lfx_host_alloc(ctx_, capacity * sizeof(PointXYZIR), &p);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
    pinned_.push_back(p);
    return static_cast<PointXYZIR *>(p);
  }

  // feature_extraction.cpp:114-157 for one cloud, results left where the library put them (pinned host memory owned by
  // the context, valid until the next call): no copies.
  lfx_scan_result ExtractFeaturesView(const PointXYZIR * points, std::size_t n) const
  {
    lfx_scan_result r{};
    const int rc = lfx_extract(ctx_, points, n, &r);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
    return r;
  }

  // The pipelined pair (lfx_extract_submit / lfx_extract_wait): Submit returns at once with a ticket, Wait gives that
  // scan's view.  Two scans may be in flight; the upload of one runs beside the kernels of the one before.  For the
  // node: Submit the cloud that just arrived, Wait for (and publish) the one submitted by the previous callback.
  std::uint64_t Submit(const PointXYZIR * points, std::size_t n) const
  {
    std::uint64_t ticket = 0;
    const int rc = lfx_extract_submit(ctx_, points, n, &ticket);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
    return ticket;
  }
  lfx_scan_result Wait(std::uint64_t ticket) const
  {
    lfx_scan_result r{};
    const int rc = lfx_extract_wait(ctx_, ticket, &r);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
    return r;
  }

  // The same, copied into containers the caller keeps.
  Features ExtractFeatures(const PointXYZIR * points, std::size_t n) const
  {
    const lfx_scan_result r = ExtractFeaturesView(points, n);
    Features f;
    if (r.labels) {f.labels.assign(r.labels, r.labels + r.n_points);}
    if (r.curvature) {f.curvature.assign(r.curvature, r.curvature + r.n_points);}
    if (r.sorted_index) {f.sorted_index.assign(r.sorted_index, r.sorted_index + r.n_sorted);}
    f.edge_index.assign(r.edge_index, r.edge_index + r.n_edge);
    f.surface_index.assign(r.surface_index, r.surface_index + r.n_surface);
    fill(f.edge, r.edge_points, r.edge_index, r.n_edge, points);
    fill(f.surface, r.surface_points, r.surface_index, r.n_surface, points);
    for (std::uint32_t k = 0; k < r.n_rings; k++) {
      f.rings.push_back(
        RingInfo{r.ring_id[k], r.ring_count[k], r.ring_offset[k], static_cast<lfx_ring_status>(r.ring_status[k])});
    }
    return f;
  }
  Features ExtractFeatures(const std::vector<PointXYZIR> & cloud) const
  {
    return ExtractFeatures(cloud.data(), cloud.size());
  }
  // colored_scan of the node (feature_extraction.cpp:153): x, y, z + packed rgb per input point.
  std::vector<float> ColorPointsByLabel(const PointXYZIR * points, std::size_t n, const Features & f) const
  {
    std::vector<float> out(4 * n);
    const int rc = lfx_color_points_by_label(ctx_, points, n, f.labels.data(), out.data());
    if (rc != LFX_OK) {throw Error(rc, "invalid label");}
    return out;
  }
  // The sensor's motion during the sweep taken out of the clouds of the scans this object was last given (lfx_deskew_batch),
  // in place: what Localizer::Update(), Odometry::Update() and Mapper::Add read afterwards is de-skewed.  sweeps: one per
  // scan (t0, t1 and the motion: the sensor frame at the sweep's end in its frame at the start); time: where a record's
  // firing time comes from (TimeField::FromIndex(), TimeField::FromFields(...)); to: LFX_DESKEW_TO_END or _TO_START.
  // d_edge_out / d_surface_out: device buffers laid out like the context's clouds for the out-of-place form (both, or
  // neither); stream: a hipStream_t the call is queued on.
  void Deskew(
    const lfx_time_field & time, const std::vector<lfx_sweep> & sweeps, int to = LFX_DESKEW_TO_END, float * d_edge_out = nullptr,
    float * d_surface_out = nullptr, void * stream = nullptr) const
  {
    const int rc = lfx_deskew_batch(ctx_, &time, sweeps.data(), static_cast<std::uint32_t>(sweeps.size()), to, d_edge_out, d_surface_out, stream);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
  }
  // The same along the sensor's poses within each sweep (lfx_deskew_batch_trajectory), one trajectory per scan: for a
  // caller with an IMU, a wheel odometer or a pose stream
  void DeskewTrajectory(
    const lfx_time_field & time, const std::vector<Trajectory> & trajectories, float * d_edge_out = nullptr,
    float * d_surface_out = nullptr, void * stream = nullptr) const
  {
    const std::vector<lfx_trajectory> views = Views(trajectories);
    const int rc = lfx_deskew_batch_trajectory(ctx_, &time, views.data(), static_cast<std::uint32_t>(views.size()), d_edge_out, d_surface_out, stream);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
  }
  // The scan-context descriptors of the scans this object was last given (lfx_scan_context_batch), from their input records:
  // d_desc_out [n_scans][R][S] floats in memory the device writes -- device memory, or a pinned block of this object
  // (PinnedFloats), which the host then reads once `stream` has passed the call.
  static lfx_scan_context_config DefaultScanContextConfig() {lfx_scan_context_config c; lfx_scan_context_default_config(&c); return c;}
  void ScanContext(const lfx_scan_context_config & config, std::uint32_t n_scans, float * d_desc_out, void * stream = nullptr) const
  {
    const int rc = lfx_scan_context_batch(ctx_, &config, n_scans, d_desc_out, stream);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
  }
  // Ground, clusters and clutter (lfx_segment_batch): the class (LFX_SEG_*) and the cluster id of every input record of the
  // scans this object was last given, through a range image per scan; d_class_out (one byte per record), d_id_out and
  // d_counts_out ([n_scans][4], either may be null) in memory the device writes, addressed by the view's scan_begin.
  // lfx_batch_points: the input records of the scans this object was last given -- what d_class_out / d_id_out are sized by
  std::uint64_t BatchPoints() const
  {
    std::uint64_t n = 0;
    lfx_batch_points(ctx_, &n);
    return n;
  }
  static lfx_segment_config DefaultSegmentConfig() {lfx_segment_config c; lfx_segment_default_config(&c); return c;}
  void Segment(
    const lfx_segment_config & config, std::uint32_t n_scans, std::uint8_t * d_class_out, std::uint32_t * d_id_out = nullptr,
    std::uint32_t * d_counts_out = nullptr, void * stream = nullptr) const
  {
    const int rc = lfx_segment_batch(ctx_, &config, n_scans, d_class_out, d_id_out, d_counts_out, stream);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
  }
  // lfx_pack_features through a class mask (lfx_pack_features_segmented): the features whose original point has a class of the
  // cloud's mask, in order; d_offsets_out [2][batch + 1] and d_counts_out [2][batch] (may be null) are the begin / count
  // tables Mapper::Add and RollingMap::Insert take.
  void PackFeaturesSegmented(
    const std::uint8_t * d_class, float * d_edge_out, float * d_surface_out, std::uint32_t * d_offsets_out, std::size_t capacity_points,
    std::uint32_t * d_counts_out = nullptr, std::uint32_t edge_mask = LFX_SEG_EDGE_MASK_DEFAULT,
    std::uint32_t surface_mask = LFX_SEG_SURFACE_MASK_DEFAULT, void * stream = nullptr) const
  {
    const int rc = lfx_pack_features_segmented(ctx_, d_class, edge_mask, surface_mask, d_edge_out, d_surface_out, d_offsets_out, d_counts_out,
      capacity_points, stream);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
  }
  // lfx_batch_status: waits for `stream` and throws if a scan this object was last given carries an error bit.  The wait a
  // caller needs between ScanContext (queued, reads the scans' input records) and the next scan it hands over.
  void BatchStatus(void * stream = nullptr) const
  {
    const int rc = lfx_batch_status(ctx_, stream, nullptr);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
  }
  float * PinnedFloats(std::size_t count)
  {
    void * p = nullptr;
    const int rc = lfx_host_alloc(ctx_, count * sizeof(float), &p);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
    pinned_.push_back(p);
    return static_cast<float *>(p);
  }
  lfx_ctx * handle() const {return ctx_;}
  // records the device clouds of the last scan may span (their buffers' extent: one scan of max_points_per_scan)
  std::size_t CloudCapacity() const {return max_points_;}

private:
  static void fill(
    std::vector<PointXYZIR> & out, const float * pts, const std::uint32_t * idx, std::uint32_t n,
    const PointXYZIR * in)
  {
    out.resize(n);
    for (std::uint32_t k = 0; k < n; k++) {
      PointXYZIR q{};
      q.x = pts[4 * k]; q.y = pts[4 * k + 1]; q.z = pts[4 * k + 2]; q.pad = 1.0f;
      q.intensity = pts[4 * k + 3];            // (float)curvature, label.hpp:176
      q.ring = in[idx[k]].ring;
      out[k] = q;
    }
  }
  lfx_ctx * ctx_ = nullptr;
  std::vector<void *> pinned_;
  std::uint32_t max_points_ = 0;
};

// Where a point's firing time comes from (lfx_time_field): its index in the scan, or the time channel of a PointCloud2
// field list (the first field named t, time, timestamp, time_stamp or offset_time).  No device.
struct TimeField
{
  static lfx_time_field FromIndex() {return lfx_time_field{LFX_TIME_FROM_INDEX, 0u, 0u, 0u, 1.0};}
  static lfx_time_field FromFields(const std::vector<lfx_point_field> & fields, std::uint32_t point_step, bool is_bigendian = false)
  {
    lfx_time_field out{};
    const int rc = lfx_time_field_from_fields(fields.data(), static_cast<std::uint32_t>(fields.size()), point_step, is_bigendian ? 1 : 0, &out);
    if (rc != LFX_OK) {
      throw Error(rc, rc == LFX_ERR_NO_TIME_FIELD ? "the cloud has no per-point time field" : "the time field must be FLOAT32, FLOAT64 or UINT32 inside point_step");
    }
    return out;
  }
};

// Map files (PCD) as pcl::io::loadPCDFile<pcl::PointXYZ> reads them and pcl::io::save writes them (lfx_pcd_read /
// lfx_pcd_write): records of 4 floats, x, y, z, 1.0f.  No device.
inline std::vector<float> ReadPcd(const std::string & path, bool drop_nonfinite = false)
{
  char msg[512];
  std::uint64_t n = 0, bad = 0;
  int rc = lfx_pcd_read(path.c_str(), nullptr, 0, drop_nonfinite ? 1 : 0, &n, &bad, msg, sizeof(msg));
  std::vector<float> out(4 * static_cast<std::size_t>(n));
  if (rc == LFX_OK) {rc = lfx_pcd_read(path.c_str(), out.data(), n, drop_nonfinite ? 1 : 0, &n, &bad, msg, sizeof(msg));}
  if (rc != LFX_OK) {throw Error(rc, msg);}
  out.resize(4 * static_cast<std::size_t>(n));
  return out;
}
inline void WritePcd(const std::string & path, const std::vector<float> & points)
{
  char msg[512];
  const int rc = lfx_pcd_write(path.c_str(), points.data(), points.size() / 4, msg, sizeof(msg));
  if (rc != LFX_OK) {throw Error(rc, msg);}
}

// A report's covariance (lfx_align_report::covariance: rotation increment in the scan's frame, then translation in the map
// frame) in the order of geometry_msgs/PoseWithCovariance: x, y, z, rotation about the fixed X, Y, Z axes.  No device.
inline void CovarianceRos(const double pose[12], const double covariance[36], double out[36])
{
  const int rc = lfx_align_covariance_ros(pose, covariance, out);
  if (rc != LFX_OK) {throw Error(rc, "lfx_align_covariance_ros: a null pointer");}
}

// The consumer of the two clouds: Localizer of the reference's localization package (localization/include/
// lidar_feature_localization/localizer.hpp:48-95) -- maps built once (there: two KD-trees in the problem's constructor),
// Init(pose), Update(scan) -> success, Get() -> pose.  Poses are [R | t], row-major 3 x 4.
class Localizer
{
public:
  // edge_map / surface_map: records of 4 floats (x, y, z, -) on the host; cell_size: the grid behind the nearest-neighbour
  // search (lfx_map_create).  `fx` must outlive the localizer.
  Localizer(
    const FeatureExtraction & fx, const std::vector<float> & edge_map, const std::vector<float> & surface_map,
    int max_iter = 20, float cell_size = 1.0f)
  : ctx_(fx.handle()), max_iter_(max_iter)
  {
    int rc = lfx_map_create_host(ctx_, edge_map.data(), static_cast<std::uint32_t>(edge_map.size() / 4), cell_size, &edge_, nullptr);
    if (rc == LFX_OK) {
      rc = lfx_map_create_host(ctx_, surface_map.data(), static_cast<std::uint32_t>(surface_map.size() / 4), cell_size, &surface_, nullptr);
    }
    if (rc != LFX_OK) {
      lfx_map_destroy(edge_);
      throw Error(rc, lfx_last_error(ctx_));
    }
    const double identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    for (int i = 0; i < 12; i++) {last_.pose[i] = identity[i];}
  }
  // The localization node's start (localization.cpp:78-85): both maps read from PCD files, records with a non-finite
  // coordinate left out (lfx_map_create requires finite points).  The node runs max_iter 40 (localization.cpp:54).
  Localizer(
    const FeatureExtraction & fx, const std::string & edge_pcd_path, const std::string & surface_pcd_path,
    int max_iter = 20, float cell_size = 1.0f)
  : Localizer(fx, ReadPcd(edge_pcd_path, true), ReadPcd(surface_pcd_path, true), max_iter, cell_size) {}
  ~Localizer() {lfx_map_destroy(edge_); lfx_map_destroy(surface_);}
  Localizer(const Localizer &) = delete;
  Localizer & operator=(const Localizer &) = delete;

  void Init(const double pose[12])
  {
    for (int i = 0; i < 12; i++) {last_.pose[i] = pose[i];}
    initialized_ = true;
  }
  bool IsInitialized() const {return initialized_;}
  const double * Get() const {return last_.pose;}
  const lfx_align_result & Result() const {return last_;}      // OptimizationResult of the last Update
  // How good that pose is (information matrix, covariance, degeneracy, inliers), if the last Update was given a report to
  // fill; valid == 0 otherwise.  The reference's node publishes a constant here (subscriber.hpp:158-169).
  const lfx_align_report & LastReport() const {return report_;}

  // Update with the scan the FeatureExtraction was last given (its clouds are still on the device: nothing is copied)
  bool Update() {return Update(static_cast<lfx_align_report *>(nullptr));}
  // (with a report: one more search and row build at the returned pose and one reduction; the pose is the same bits)
  bool Update(lfx_align_report * report)
  {
    lfx_align_result r{};
    report_ = lfx_align_report{};
    const int rc = report ?
      lfx_localize_batch_report(ctx_, edge_, surface_, kNeighbors, max_iter_, 1.0f, 1u, last_.pose, &r, &report_, nullptr) :
      lfx_localize_batch(ctx_, edge_, surface_, kNeighbors, max_iter_, 1.0f, 1u, last_.pose, &r, nullptr);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
    last_ = r;
    if (report) {*report = report_;}
    return LFX_ALIGN_SUCCESS(r.code);
  }
  // Update with clouds received from elsewhere (scan_edge / scan_surface as published: 4 floats per point)
  bool Update(const float * edge, std::uint32_t n_edge, const float * surface, std::uint32_t n_surface, lfx_align_report * report = nullptr)
  {
    lfx_align_result r{};
    report_ = lfx_align_report{};
    const int rc = report ?
      lfx_localize_host_report(ctx_, edge_, surface_, kNeighbors, max_iter_, 1.0f, edge, n_edge, surface, n_surface, last_.pose, &r, &report_, nullptr) :
      lfx_localize_host(ctx_, edge_, surface_, kNeighbors, max_iter_, 1.0f, edge, n_edge, surface, n_surface, last_.pose, &r, nullptr);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
    last_ = r;
    if (report) {*report = report_;}
    return LFX_ALIGN_SUCCESS(r.code);
  }

private:
  static constexpr std::uint32_t kNeighbors = 15;               // N_NEIGHBORS, localizer.hpp:46
  lfx_ctx * ctx_;
  int max_iter_;
  lfx_map * edge_ = nullptr, * surface_ = nullptr;
  lfx_align_result last_{};
  lfx_align_report report_{};
  bool initialized_ = false;
};

// Scan-to-local-map odometry: Odometry<PoseUpdater, EdgeSurfaceMap, EdgeSurfaceScan> of the reference's localization package
// (odometry.hpp:43-71; the node that would run it, OdometrySubscriber, subscriber.hpp:192-239) -- Update(scan) aligns the
// scan against the last n_local_scans scans from the previous pose and adds it; CurrentPose().  The store and the window
// maps live on the device of `fx`, which must outlive the odometry.  Poses are [R | t], row-major 3 x 4.
class Odometry
{
public:
  static lfx_odometry_config DefaultConfig() {lfx_odometry_config c; lfx_odometry_default_config(&c); return c;}
  explicit Odometry(const FeatureExtraction & fx, const lfx_odometry_config & config = DefaultConfig())
  : ctx_(fx.handle())
  {
    const int rc = lfx_odometry_create(ctx_, &config, &odometry_);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
  }
  ~Odometry() {lfx_odometry_destroy(odometry_);}
  Odometry(const Odometry &) = delete;
  Odometry & operator=(const Odometry &) = delete;

  // Update with every scan the FeatureExtraction was last given, in order (their clouds are still on the device)
  const std::vector<lfx_odometry_result> & Update()
  {
    lfx_device_view view{};
    int rc = lfx_device_results(ctx_, &view);
    if (rc == LFX_OK) {
      results_.assign(view.batch, lfx_odometry_result{});
      rc = lfx_odometry_update_batch(ctx_, odometry_, view.batch, results_.data(), nullptr);
    }
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
    return results_;
  }
  // The same with every scan de-skewed by its own constant-velocity prediction first (lfx_odometry_update_batch_deskewed):
  // the motion between the last two poses, scaled by sweep_ratio (sweep time over scan period).  sweep_times: t0, t1 per
  // scan with a time field; empty with TimeField::FromIndex()
  const std::vector<lfx_odometry_result> & UpdateBatchDeskewed(
    const lfx_time_field & time, const std::vector<double> & sweep_times = {}, double sweep_ratio = 1.0, int to = LFX_DESKEW_TO_END)
  {
    lfx_device_view view{};
    int rc = lfx_device_results(ctx_, &view);
    if (rc == LFX_OK && !sweep_times.empty() && sweep_times.size() != 2 * static_cast<std::size_t>(view.batch)) {
      throw Error(LFX_ERR_INVALID_ARGUMENT, "sweep_times must hold t0, t1 per scan");
    }
    if (rc == LFX_OK) {
      results_.assign(view.batch, lfx_odometry_result{});
      rc = lfx_odometry_update_batch_deskewed(ctx_, odometry_, &time, sweep_times.empty() ? nullptr : sweep_times.data(), sweep_ratio, to,
        view.batch, results_.data(), nullptr);
    }
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
    return results_;
  }
  // The same with every scan de-skewed along the caller's trajectory of it (lfx_odometry_update_batch_trajectory)
  const std::vector<lfx_odometry_result> & UpdateBatchTrajectory(const lfx_time_field & time, const std::vector<Trajectory> & trajectories)
  {
    const std::vector<lfx_trajectory> views = Views(trajectories);
    results_.assign(views.size(), lfx_odometry_result{});
    const int rc = lfx_odometry_update_batch_trajectory(ctx_, odometry_, &time, views.data(), static_cast<std::uint32_t>(views.size()),
      results_.data(), nullptr);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
    return results_;
  }
  // Update with clouds received from elsewhere (scan_edge / scan_surface as published: 4 floats per point)
  const lfx_odometry_result & Update(const float * edge, std::uint32_t n_edge, const float * surface, std::uint32_t n_surface)
  {
    results_.assign(1, lfx_odometry_result{});
    const int rc = lfx_odometry_update_host(ctx_, odometry_, edge, n_edge, surface, n_surface, results_.data(), nullptr);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
    return results_[0];
  }
  // Update with one scan's clouds in memory the device reads (lfx_odometry_update): device buffers, or pinned blocks a kernel
  // has filled -- the filtered clouds of FeatureExtraction::PackFeaturesSegmented, for one
  const lfx_odometry_result & UpdateDevice(const float * d_edge, std::uint32_t n_edge, const float * d_surface, std::uint32_t n_surface)
  {
    results_.assign(1, lfx_odometry_result{});
    const int rc = lfx_odometry_update(ctx_, odometry_, d_edge, n_edge, d_surface, n_surface, results_.data(), nullptr);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
    return results_[0];
  }
  // Reports of the scans the Update calls align (off by default): Reports() = those of the last Update, one per scan,
  // valid == 0 for a scan that was not aligned
  void SetReports(bool on)
  {
    const int rc = lfx_odometry_set_reports(odometry_, on ? 1 : 0);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
  }
  std::vector<lfx_align_report> Reports() const
  {
    std::uint32_t n = 0;
    int rc = lfx_odometry_reports(odometry_, nullptr, 0, &n);
    std::vector<lfx_align_report> out(n);
    if (rc == LFX_OK && n) {rc = lfx_odometry_reports(odometry_, out.data(), n, &n);}
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
    return out;
  }
  std::vector<double> CurrentPose() const
  {
    std::vector<double> pose(12);
    lfx_odometry_pose(odometry_, pose.data());
    return pose;
  }
  lfx_odometry_store_view View() const
  {
    lfx_odometry_store_view v{};
    lfx_odometry_view(odometry_, &v);
    return v;
  }
  // EdgeSurfaceMap::Save(dirname): dirname/edge.pcd and dirname/surface.pcd from the store, each only if non-empty
  void Save(const std::string & dirname, int written[2] = nullptr) const
  {
    int w[2] = {0, 0};
    const int rc = lfx_odometry_save(ctx_, odometry_, dirname.c_str(), w, nullptr);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
    if (written) {written[0] = w[0]; written[1] = w[1];}
  }

private:
  lfx_ctx * ctx_;
  lfx_odometry * odometry_ = nullptr;
  std::vector<lfx_odometry_result> results_;
};

// The keyframe map builder: MapBuilder<PointType> of the reference's mapping package (map.hpp:95-153; the node,
// mapping.cpp) with its map on the device of `fx`, which must outlive the mapper.  One mapper per map: an edge mapper and a
// surface mapper for the two files the localization node loads.  Poses are [R | t], row-major 3 x 4.
class Mapper
{
public:
  enum Which {kEdge = 2, kSurface = 3};     // the clouds of the last device batch (their count's word in scan_info)
  static lfx_mapper_config DefaultConfig() {lfx_mapper_config c; lfx_mapper_default_config(&c); return c;}
  explicit Mapper(const FeatureExtraction & fx, const lfx_mapper_config & config = DefaultConfig())
  : fx_(fx)
  {
    const int rc = lfx_mapper_create(fx.handle(), &config, &mapper_);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(fx.handle()));}
  }
  ~Mapper() {lfx_mapper_destroy(mapper_);}
  Mapper(const Mapper &) = delete;
  Mapper & operator=(const Mapper &) = delete;

  // MapBuilder::Callback for the edge or surface cloud of every scan the FeatureExtraction was last given (still on the
  // device), one pose (12 doubles) per scan; the outcomes (LFX_KEYFRAME_*)
  const std::vector<std::uint8_t> & Add(Which which, const std::vector<double> & poses)
  {
    lfx_device_view view{};
    int rc = lfx_device_results(fx_.handle(), &view);
    if (rc == LFX_OK && poses.size() != 12 * static_cast<std::size_t>(view.batch)) {rc = LFX_ERR_INVALID_ARGUMENT;}
    if (rc == LFX_OK) {
      outcomes_.assign(view.batch, 0);
      rc = lfx_mapper_add(fx_.handle(), mapper_, which == kEdge ? view.edge_points : view.surface_points, view.scan_begin,
        view.scan_info + which, 4, view.batch, fx_.CloudCapacity(), poses.data(), outcomes_.data(), nullptr);
    }
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(fx_.handle()));}
    return outcomes_;
  }
  // MapBuilder::Callback for one cloud received from elsewhere (4 floats per point, as published)
  std::uint8_t Add(const float * points, std::uint32_t n_points, const double pose[12])
  {
    std::uint8_t outcome = 0;
    const int rc = lfx_mapper_add_host(fx_.handle(), mapper_, points, n_points, pose, &outcome, nullptr);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(fx_.handle()));}
    return outcome;
  }
  lfx_mapper_store_view View() const
  {
    lfx_mapper_store_view v{};
    lfx_mapper_view(mapper_, &v);
    return v;
  }
  // SaveMap: false (and no file) for an empty map
  bool Save(const std::string & path) const
  {
    int written = 0;
    const int rc = lfx_mapper_save(fx_.handle(), mapper_, path.c_str(), &written, nullptr);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(fx_.handle()));}
    return written != 0;
  }

private:
  const FeatureExtraction & fx_;
  lfx_mapper * mapper_ = nullptr;
  std::vector<std::uint8_t> outcomes_;
};

// The rolling voxel map (lfx_rolling_map): one point per voxel in a window that follows the vehicle, an edge store and a
// surface store on the device of `fx`, which must outlive it -- the map LOAM's mapping stage keeps.  Update() aligns every
// scan the FeatureExtraction was last given against the boxes cut out around its initial pose and inserts it at the result;
// fed an Odometry's poses of the same scans it corrects them against everything the window still holds.  Poses are
// [R | t], row-major 3 x 4.
class RollingMap
{
public:
  enum Kind {kEdge = LFX_ROLLING_EDGE, kSurface = LFX_ROLLING_SURFACE};
  static lfx_rolling_map_config DefaultConfig() {lfx_rolling_map_config c; lfx_rolling_map_default_config(&c); return c;}
  explicit RollingMap(const FeatureExtraction & fx, const lfx_rolling_map_config & config = DefaultConfig())
  : ctx_(fx.handle())
  {
    const int rc = lfx_rolling_map_create(ctx_, &config, &map_);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
  }
  ~RollingMap() {lfx_rolling_map_destroy(map_);}
  RollingMap(const RollingMap &) = delete;
  RollingMap & operator=(const RollingMap &) = delete;
  RollingMap(RollingMap && o) noexcept : ctx_(o.ctx_), map_(o.map_), results_(std::move(o.results_)) {o.map_ = nullptr;}
  RollingMap & operator=(RollingMap && o) noexcept
  {
    if (this != &o) {
      lfx_rolling_map_destroy(map_);
      ctx_ = o.ctx_; map_ = o.map_; results_ = std::move(o.results_);
      o.map_ = nullptr;
    }
    return *this;
  }

  // lfx_rolling_map_update_batch for every scan the FeatureExtraction was last given; odometry_poses: 12 doubles per scan
  // (an Odometry's results for the same scans), or empty: every scan starts from the current pose
  const std::vector<lfx_rolling_map_result> & Update(const std::vector<double> & odometry_poses = {})
  {
    lfx_device_view view{};
    int rc = lfx_device_results(ctx_, &view);
    if (rc == LFX_OK && !odometry_poses.empty() && odometry_poses.size() != 12 * static_cast<std::size_t>(view.batch)) {
      throw Error(LFX_ERR_INVALID_ARGUMENT, "odometry_poses must hold 12 doubles per scan");
    }
    if (rc == LFX_OK) {
      results_.assign(view.batch, lfx_rolling_map_result{});
      rc = lfx_rolling_map_update_batch(ctx_, map_, view.batch, odometry_poses.empty() ? nullptr : odometry_poses.data(), results_.data(),
        nullptr);
    }
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
    return results_;
  }
  void Recenter(const double center[3])
  {
    const int rc = lfx_rolling_map_recenter(map_, center);
    if (rc != LFX_OK) {throw Error(rc, "the centre must be finite and have a voxel");}
  }
  // one cloud received from elsewhere (4 floats per point) into the edge or the surface store at `pose`
  void Insert(Kind kind, const float * points, std::uint32_t n_points, const double pose[12])
  {
    const int rc = lfx_rolling_map_insert_host(ctx_, map_, kind, points, n_points, pose, nullptr);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
  }
  // the live voxels of the box lo .. hi (metres) of one store into device memory of the caller's (d_out: capacity_points
  // records of 4 floats, or null with capacity 0), ascending (vz, vy, vx); returns how many the box holds
  std::uint64_t Extract(Kind kind, const double lo[3], const double hi[3], float * d_out, std::uint64_t capacity_points) const
  {
    std::uint64_t n = 0;
    const int rc = lfx_rolling_map_extract(ctx_, map_, kind, lo, hi, d_out, capacity_points, &n, nullptr);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
    return n;
  }
  std::vector<double> CurrentPose() const
  {
    std::vector<double> pose(12);
    lfx_rolling_map_pose(map_, pose.data());
    return pose;
  }
  lfx_rolling_map_view_t View() const
  {
    lfx_rolling_map_view_t v{};
    const int rc = lfx_rolling_map_view(ctx_, map_, &v, nullptr);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
    return v;
  }
  // dirname/edge.pcd and dirname/surface.pcd of the whole windows, each only if non-empty
  void Save(const std::string & dirname, int written[2] = nullptr) const
  {
    int w[2] = {0, 0};
    const int rc = lfx_rolling_map_save(ctx_, map_, dirname.c_str(), w, nullptr);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(ctx_));}
    if (written) {written[0] = w[0]; written[1] = w[1];}
  }
  lfx_rolling_map * handle() const {return map_;}

private:
  lfx_ctx * ctx_;
  lfx_rolling_map * map_ = nullptr;
  std::vector<lfx_rolling_map_result> results_;
};

// The place index (lfx_place_db): scan-context descriptors of one config on the device of `fx`, which must outlive it, each
// compared with a query under every column shift.  For start-up relocalisation (index the keyframes of a map, query with
// the first scan) and for loop detection (index the keyframes as the mapper adds them; query the range that leaves the most
// recent ones out).  A match's yaw: the revisit's initial pose is the entry's pose times Rz(yaw).
class PlaceDb
{
public:
  PlaceDb(const FeatureExtraction & fx, const lfx_scan_context_config & config, std::uint32_t capacity)
  : fx_(fx), config_(config)
  {
    const int rc = lfx_place_db_create(fx.handle(), &config, capacity, &db_);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(fx.handle()));}
  }
  ~PlaceDb() {lfx_place_db_destroy(db_);}
  PlaceDb(const PlaceDb &) = delete;
  PlaceDb & operator=(const PlaceDb &) = delete;

  const lfx_scan_context_config & Config() const {return config_;}
  // n descriptors the device reads (device memory, or a pinned block); entry = insertion order
  void Add(const float * d_desc, std::uint32_t n, void * stream = nullptr)
  {
    const int rc = lfx_place_db_add(fx_.handle(), db_, d_desc, n, stream);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(fx_.handle()));}
  }
  // the same from pageable host memory (descriptors kept in a file)
  void AddHost(const std::vector<float> & desc, std::uint32_t n, void * stream = nullptr)
  {
    const int rc = desc.size() == static_cast<std::size_t>(n) * config_.n_rings * config_.n_sectors ?
      lfx_place_db_add_host(fx_.handle(), db_, desc.data(), n, stream) : LFX_ERR_INVALID_ARGUMENT;
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(fx_.handle()));}
  }
  std::uint32_t Size() const
  {
    std::uint32_t n = 0;
    lfx_place_db_size(db_, &n);
    return n;
  }
  std::vector<float> Download(std::uint32_t first, std::uint32_t count, void * stream = nullptr) const
  {
    std::vector<float> out(static_cast<std::size_t>(count) * config_.n_rings * config_.n_sectors);
    const int rc = lfx_place_db_download(fx_.handle(), db_, first, count, out.data(), stream);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(fx_.handle()));}
    return out;
  }
  // per query the k best of entries [first, first + count): [n_queries][k], ascending distance
  std::vector<lfx_place_match> Query(
    const float * d_desc, std::uint32_t n_queries, std::uint32_t k, std::uint32_t first, std::uint32_t count, void * stream = nullptr) const
  {
    std::vector<lfx_place_match> out(static_cast<std::size_t>(n_queries) * k);
    const int rc = lfx_place_db_query(fx_.handle(), db_, d_desc, n_queries, first, count, k, out.data(), stream);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(fx_.handle()));}
    return out;
  }
  std::vector<lfx_place_match> Query(const float * d_desc, std::uint32_t n_queries, std::uint32_t k = 1) const
  {
    return Query(d_desc, n_queries, k, 0, Size());
  }
  // the same with a gate per query (lfx_place_db_query_gated): entry e is eligible for query q iff e < gates[q].limit and,
  // where d_poses is given and gates[q].pose is not LFX_PLACE_NO_POSE, its pose lies within `radius` of pose gates[q].pose;
  // n_eligible (may be null) takes the eligible entries of each query
  std::vector<lfx_place_match> QueryGated(
    const float * d_desc, const std::vector<lfx_place_gate> & gates, const double * d_poses, double radius, std::uint32_t k = 1,
    std::vector<std::uint32_t> * n_eligible = nullptr, void * stream = nullptr) const
  {
    const std::uint32_t n_queries = static_cast<std::uint32_t>(gates.size());
    std::vector<lfx_place_match> out(gates.size() * k);
    if (n_eligible) {n_eligible->assign(gates.size(), 0u);}
    const int rc = lfx_place_db_query_gated(fx_.handle(), db_, d_desc, n_queries, gates.data(), d_poses, radius, k, out.data(),
        n_eligible ? n_eligible->data() : nullptr, stream);
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(fx_.handle()));}
    return out;
  }
  lfx_place_db * handle() const {return db_;}

private:
  const FeatureExtraction & fx_;
  lfx_scan_context_config config_;
  lfx_place_db * db_ = nullptr;
};

// The pose graph (lfx_pose_graph): keyframe poses as nodes, odometry steps and loop closures as edges, optimised on the
// device of `fx`, which must outlive it.  Poses are 12 doubles [R | t] row-major; node 0 is fixed unless ReleaseFirst frees
// it.  An edge's information comes from an alignment report through EdgeInformation, its measurement from
// lfx_motion_between.  Absolute fixes of single nodes (GNSS positions with a lever arm, poses against an older map) are
// priors: ReservePriors once, then AddPriors.
class PoseGraph
{
public:
  static lfx_pose_graph_config DefaultConfig(std::uint32_t max_nodes, std::uint32_t max_edges)
  {
    lfx_pose_graph_config c;
    lfx_pose_graph_default_config(&c);
    c.max_nodes = max_nodes;
    c.max_edges = max_edges;
    return c;
  }
  PoseGraph(const FeatureExtraction & fx, const lfx_pose_graph_config & config)
  : fx_(fx)
  {
    Check(lfx_pose_graph_create(fx.handle(), &config, &graph_));
  }
  ~PoseGraph() {lfx_pose_graph_destroy(graph_);}
  PoseGraph(const PoseGraph &) = delete;
  PoseGraph & operator=(const PoseGraph &) = delete;

  // report_information in an edge's residual coordinates (lfx_pose_graph_edge_information)
  static std::vector<double> EdgeInformation(const double pose_j[12], const double report_information[36])
  {
    std::vector<double> out(36);
    if (lfx_pose_graph_edge_information(pose_j, report_information, out.data()) != LFX_OK) {throw Error(LFX_ERR_INVALID_ARGUMENT, "null argument");}
    return out;
  }
  // poses: n x 12 doubles; the id of the first node added
  std::uint32_t AddNodes(const std::vector<double> & poses, void * stream = nullptr)
  {
    std::uint32_t first = 0;
    Check(poses.size() % 12u == 0u ? lfx_pose_graph_add_nodes(fx_.handle(), graph_, poses.data(), static_cast<std::uint32_t>(poses.size() / 12u), &first, stream) :
      LFX_ERR_INVALID_ARGUMENT);
    return first;
  }
  void SetFixed(std::uint32_t node, bool fixed = true, void * stream = nullptr) {Check(lfx_pose_graph_set_fixed(fx_.handle(), graph_, node, fixed ? 1 : 0, stream));}
  void AddEdges(const std::vector<lfx_pose_graph_edge> & edges, void * stream = nullptr)
  {
    Check(lfx_pose_graph_add_edges(fx_.handle(), graph_, edges.data(), static_cast<std::uint32_t>(edges.size()), stream));
  }
  lfx_pose_graph_result Optimize(void * stream = nullptr)
  {
    lfx_pose_graph_result r;
    Check(lfx_pose_graph_optimize(fx_.handle(), graph_, &r, stream));
    return r;
  }
  std::vector<double> Poses(std::uint32_t first, std::uint32_t count, void * stream = nullptr) const
  {
    std::vector<double> out(static_cast<std::size_t>(count) * 12u);
    Check(lfx_pose_graph_poses(fx_.handle(), graph_, first, count, out.data(), stream));
    return out;
  }
  std::vector<double> Poses() const {return Poses(0, Info().n_nodes);}
  void SetPoses(std::uint32_t first, const std::vector<double> & poses, void * stream = nullptr)
  {
    Check(poses.size() % 12u == 0u ? lfx_pose_graph_set_poses(fx_.handle(), graph_, first, static_cast<std::uint32_t>(poses.size() / 12u), poses.data(), stream) :
      LFX_ERR_INVALID_ARGUMENT);
  }
  // the poses on the device ([n_nodes][12] doubles), current behind `stream`
  const double * View(std::uint32_t * n_nodes, void * stream = nullptr) const
  {
    const double * p = nullptr;
    Check(lfx_pose_graph_view(fx_.handle(), graph_, &p, n_nodes, stream));
    return p;
  }
  // per edge rho and w at the poses the last Optimize left
  void EdgeChi2(std::vector<double> & rho, std::vector<double> & w, void * stream = nullptr) const
  {
    const std::uint32_t n = Info().n_edges;
    rho.resize(n);
    w.resize(n);
    Check(lfx_pose_graph_edge_chi2(fx_.handle(), graph_, 0, n, rho.data(), w.data(), stream));
  }
  lfx_pose_graph_info_t Info() const
  {
    lfx_pose_graph_info_t i;
    lfx_pose_graph_info(graph_, &i);
    return i;
  }
  // priors (absolute fixes of single nodes): room for max_priors of them, once, before the first
  void ReservePriors(std::uint32_t max_priors) {Check(lfx_pose_graph_reserve_priors(fx_.handle(), graph_, max_priors));}
  void AddPriors(const std::vector<lfx_pose_graph_prior> & priors, void * stream = nullptr)
  {
    Check(lfx_pose_graph_add_priors(fx_.handle(), graph_, priors.data(), static_cast<std::uint32_t>(priors.size()), stream));
  }
  // node 0 free from now on (SetFixed(0) still holds it); without a prior nothing but the damping holds a free first node
  void ReleaseFirst(bool released = true, void * stream = nullptr) {Check(lfx_pose_graph_release_first(fx_.handle(), graph_, released ? 1 : 0, stream));}
  // covariances of the optimised nodes (lfx.h, COVARIANCES): room for them, once; then per node Sigma_kk (count x 36
  // doubles) and per pair (i, j) the 12 x 12 joint block (pairs: i0, j0, i1, j1, ...; n x 144 doubles).  `code` (may be
  // null) takes LFX_POSE_GRAPH_CONVERGED or _NOT_POSITIVE_DEFINITE; without it the latter throws.
  void ReserveMarginals() {Check(lfx_pose_graph_reserve_marginals(fx_.handle(), graph_));}
  std::vector<double> Marginals(std::uint32_t first, std::uint32_t count, std::int32_t * code = nullptr, void * stream = nullptr)
  {
    std::vector<double> out(static_cast<std::size_t>(count) * 36u);
    std::int32_t got = 0;
    Check(lfx_pose_graph_marginals(fx_.handle(), graph_, first, count, out.data(), &got, stream));
    Coded(got, code);
    return out;
  }
  std::vector<double> Marginals() {return Marginals(0, Info().n_nodes);}
  std::vector<double> JointCovariances(const std::vector<std::uint32_t> & pairs, std::int32_t * code = nullptr, void * stream = nullptr)
  {
    std::vector<double> out(pairs.size() / 2u * 144u);
    std::int32_t got = 0;
    Check(pairs.size() % 2u == 0u ? lfx_pose_graph_joint_covariances(fx_.handle(), graph_, pairs.data(), static_cast<std::uint32_t>(pairs.size() / 2u),
      out.data(), &got, stream) : LFX_ERR_INVALID_ARGUMENT);
    Coded(got, code);
    return out;
  }
  // the covariance of the residual of an edge (i, j) at the current poses, from the pair's joint block
  // (lfx_pose_graph_relative_covariance): its inverse gates a loop candidate
  static std::vector<double> RelativeCovariance(const double pose_i[12], const double pose_j[12], const double joint[144])
  {
    std::vector<double> out(36);
    if (lfx_pose_graph_relative_covariance(pose_i, pose_j, joint, out.data()) != LFX_OK) {throw Error(LFX_ERR_INVALID_ARGUMENT, "null argument");}
    return out;
  }
  // per prior rho and w at the poses the last Optimize left
  void PriorChi2(std::vector<double> & rho, std::vector<double> & w, void * stream = nullptr) const
  {
    const std::uint32_t n = PriorInfo().n_priors;
    rho.resize(n);
    w.resize(n);
    Check(lfx_pose_graph_prior_chi2(fx_.handle(), graph_, 0, n, rho.data(), w.data(), stream));
  }
  lfx_pose_graph_prior_info_t PriorInfo() const
  {
    lfx_pose_graph_prior_info_t i;
    lfx_pose_graph_prior_info(graph_, &i);
    return i;
  }
  lfx_pose_graph * handle() const {return graph_;}

private:
  void Check(int rc) const
  {
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(fx_.handle()));}
  }
  static void Coded(std::int32_t got, std::int32_t * code)
  {
    if (code) {*code = got;} else if (got != LFX_POSE_GRAPH_CONVERGED) {throw Error(LFX_ERR_INVALID_ARGUMENT, "H + lambda I is not positive definite");}
  }
  const FeatureExtraction & fx_;
  lfx_pose_graph * graph_ = nullptr;
};

class VoxelFilter;

// The keyframe store (lfx_keyframes): every keyframe's edge and surface records in the SENSOR frame and one pose per
// keyframe on the device of `fx`, which must outlive it; world clouds are written from the two at the poses of the moment,
// so a map follows a PoseGraph: Follow(graph), then Build, Submap or Save.  Keyframe ids count from 0 in order of addition
// (add graph nodes in step and id == node id).  Poses are 12 doubles [R | t] row-major; clouds are records of 4 floats.
class Keyframes
{
public:
  enum Kind {kEdge = LFX_KEYFRAMES_EDGE, kSurface = LFX_KEYFRAMES_SURFACE};
  Keyframes(const FeatureExtraction & fx, std::uint32_t max_keyframes, std::uint64_t max_edge_points, std::uint64_t max_surface_points)
  : fx_(fx)
  {
    lfx_keyframes_config config;
    lfx_keyframes_default_config(&config);
    config.max_keyframes = max_keyframes;
    config.max_points[0] = max_edge_points;
    config.max_points[1] = max_surface_points;
    Check(lfx_keyframes_create(fx.handle(), &config, &store_));
  }
  ~Keyframes() {lfx_keyframes_destroy(store_);}
  Keyframes(const Keyframes &) = delete;
  Keyframes & operator=(const Keyframes &) = delete;

  // both clouds of every scan the FeatureExtraction was last given (still on the device), one pose (12 doubles) per scan;
  // the id of the first keyframe added
  std::uint32_t Add(const std::vector<double> & poses, void * stream = nullptr)
  {
    lfx_device_view view{};
    Check(lfx_device_results(fx_.handle(), &view));
    if (poses.size() != 12 * static_cast<std::size_t>(view.batch)) {Check(LFX_ERR_INVALID_ARGUMENT);}
    const lfx_keyframes_clouds edge{view.edge_points, view.scan_begin, view.scan_info + 2, 4, 0, fx_.CloudCapacity()};
    const lfx_keyframes_clouds surface{view.surface_points, view.scan_begin, view.scan_info + 3, 4, 0, fx_.CloudCapacity()};
    std::uint32_t first = 0;
    Check(lfx_keyframes_add(fx_.handle(), store_, &edge, &surface, view.batch, poses.data(), &first, stream));
    return first;
  }
  // one keyframe received from elsewhere (4 floats per point; either cloud may be empty); its id
  std::uint32_t AddHost(const std::vector<float> & edge, const std::vector<float> & surface, const double pose[12], void * stream = nullptr)
  {
    std::uint32_t id = 0;
    Check(lfx_keyframes_add_host(fx_.handle(), store_, edge.data(), static_cast<std::uint32_t>(edge.size() / 4u), surface.data(),
      static_cast<std::uint32_t>(surface.size() / 4u), pose, &id, stream));
    return id;
  }
  // every keyframe that is a node of `graph` takes the node's pose, device to device
  void Follow(const PoseGraph & graph, void * stream = nullptr)
  {
    std::uint32_t n = 0;
    const double * d_poses = graph.View(&n, stream);
    const std::uint32_t have = Info().n_keyframes;
    Check(lfx_keyframes_follow(fx_.handle(), store_, d_poses, 0, n < have ? n : have, stream));
  }
  void SetPoses(std::uint32_t first, const std::vector<double> & poses, void * stream = nullptr)
  {
    Check(poses.size() % 12u == 0u ? lfx_keyframes_set_poses(fx_.handle(), store_, first, static_cast<std::uint32_t>(poses.size() / 12u), poses.data(), stream) :
      LFX_ERR_INVALID_ARGUMENT);
  }
  std::vector<double> Poses(std::uint32_t first, std::uint32_t count, void * stream = nullptr) const
  {
    std::vector<double> out(static_cast<std::size_t>(count) * 12u);
    Check(lfx_keyframes_poses(fx_.handle(), store_, first, count, out.data(), stream));
    return out;
  }
  // the world cloud of keyframes [first, first + count) at the current poses to d_out (device, capacity_points records);
  // its records.  Returns before the cloud is written: read it behind `stream`.
  std::uint64_t Build(Kind kind, std::uint32_t first, std::uint32_t count, float * d_out, std::uint64_t capacity_points, void * stream = nullptr) const
  {
    std::uint64_t n = 0;
    Check(lfx_keyframes_build(fx_.handle(), store_, kind, first, count, d_out, capacity_points, &n, stream));
    return n;
  }
  // Build without the records whose byte of d_flags (device, addressed by the store's record index of `kind`: what
  // Visibility::Run writes) is non-zero; the kept records.  d_begin_out (device, [count + 1], may be null): the kept records
  // before each keyframe.  Waits once, for the count.
  std::uint64_t BuildMasked(Kind kind, std::uint32_t first, std::uint32_t count, const std::uint8_t * d_flags, float * d_out,
    std::uint64_t capacity_points, std::uint64_t * d_begin_out = nullptr, void * stream = nullptr) const
  {
    std::uint64_t n = 0;
    Check(lfx_keyframes_build_masked(fx_.handle(), store_, kind, first, count, d_flags, d_out, capacity_points, d_begin_out, &n, stream));
    return n;
  }
  // the records Build would write (from the host's mirror; nothing is queued)
  std::uint64_t Points(Kind kind, std::uint32_t first, std::uint32_t count) const
  {
    std::uint64_t n = 0;
    const int rc = lfx_keyframes_build(fx_.handle(), store_, kind, first, count, nullptr, 0, &n, nullptr);
    if (rc != LFX_ERR_CAPACITY) {Check(rc);}
    return n;
  }
  // the keyframes of [first, first + count) within `radius` of `center`, written whole in ascending id to d_out
  lfx_keyframes_submap_result Submap(Kind kind, const double center[3], double radius, std::uint32_t first, std::uint32_t count, float * d_out,
    std::uint64_t capacity_points, void * stream = nullptr) const
  {
    lfx_keyframes_submap_result r;
    Check(lfx_keyframes_submap(fx_.handle(), store_, kind, center, radius, first, count, d_out, capacity_points, &r, stream));
    return r;
  }
  // dirname/edge.pcd and dirname/surface.pcd at the current poses; which of the two were written
  std::pair<bool, bool> Save(const std::string & dirname, void * stream = nullptr) const
  {
    int written[2] = {0, 0};
    Check(lfx_keyframes_save(fx_.handle(), store_, dirname.c_str(), written, stream));
    return {written[0] != 0, written[1] != 0};
  }
  // Flags kept in the store (lfx.h, the section behind lfx_keyframes_build_masked): one byte per record and kind, non-zero
  // leaves the record out.  ReserveFlags once, before or after keyframes were added; Flags gives the two device arrays,
  // addressed by the store's record index -- what Visibility::Run and BuildMasked take as d_flags.
  void ReserveFlags(void * stream = nullptr) {Check(lfx_keyframes_reserve_flags(fx_.handle(), store_, stream));}
  std::pair<std::uint8_t *, std::uint8_t *> Flags(void * stream = nullptr)
  {
    std::uint8_t * d[2] = {nullptr, nullptr};
    Check(lfx_keyframes_flags(fx_.handle(), store_, d, stream));
    return {d[0], d[1]};
  }
  // the flag bytes of keyframes [first, first + count) from d_src (device, addressed by the store's record index), or zeroed
  void SetFlags(Kind kind, std::uint32_t first, std::uint32_t count, const std::uint8_t * d_src, void * stream = nullptr)
  {
    Check(lfx_keyframes_set_flags(fx_.handle(), store_, kind, first, count, d_src, stream));
  }
  void ClearFlags(Kind kind, std::uint32_t first, std::uint32_t count, void * stream = nullptr)
  {
    Check(lfx_keyframes_clear_flags(fx_.handle(), store_, kind, first, count, stream));
  }
  lfx_keyframes_flags_info_t FlagsInfo(void * stream = nullptr) const
  {
    lfx_keyframes_flags_info_t i;
    Check(lfx_keyframes_flags_info(fx_.handle(), store_, &i, stream));
    return i;
  }
  // Submap and Save without the records the store's flags leave out; n_points counts kept records
  lfx_keyframes_submap_result SubmapMasked(Kind kind, const double center[3], double radius, std::uint32_t first, std::uint32_t count,
    float * d_out, std::uint64_t capacity_points, void * stream = nullptr) const
  {
    lfx_keyframes_submap_result r;
    Check(lfx_keyframes_submap_masked(fx_.handle(), store_, kind, center, radius, first, count, d_out, capacity_points, &r, stream));
    return r;
  }
  std::pair<bool, bool> SaveMasked(const std::string & dirname, void * stream = nullptr) const
  {
    int written[2] = {0, 0};
    Check(lfx_keyframes_save_masked(fx_.handle(), store_, dirname.c_str(), written, stream));
    return {written[0] != 0, written[1] != 0};
  }
  // Save through a VoxelFilter (defined behind it): per kind one centroid per voxel of its leaf with at least min_points
  // records, in the order of first appearance; masked: without the records the store's flags leave out.  A kind of which no
  // voxel survives writes no file.
  std::pair<bool, bool> SaveFiltered(VoxelFilter & filter, const std::string & dirname, float edge_leaf = 0.2f, float surface_leaf = 0.4f,
    std::uint32_t min_points = 1, bool masked = false, void * stream = nullptr) const;
  lfx_keyframes_info_t Info() const
  {
    lfx_keyframes_info_t i;
    lfx_keyframes_info(store_, &i);
    return i;
  }
  lfx_keyframes * handle() const {return store_;}

private:
  void Check(int rc) const
  {
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(fx_.handle()));}
  }
  const FeatureExtraction & fx_;
  lfx_keyframes * store_ = nullptr;
};

// The voxel filter (lfx_voxel_filter): clouds of any size thinned to one centroid per voxel of a grid anchored at the world
// origin, on the device of `fx`, which must outlive it.  Reset(leaf), then Add / AddKeyframes as often as wanted, then Emit;
// the output is a pure function of the sequence of records (the order of first appearance, centroids from integer sums).
// log2_slots: the table has 2^log2_slots voxel entries -- about twice the voxels expected; max_records: the records between
// two resets.
class VoxelFilter
{
public:
  VoxelFilter(const FeatureExtraction & fx, std::uint32_t log2_slots, std::uint64_t max_records)
  : fx_(fx)
  {
    lfx_voxel_filter_config config;
    lfx_voxel_filter_default_config(&config);
    config.log2_slots = log2_slots;
    config.max_records = max_records;
    Check(lfx_voxel_filter_create(fx.handle(), &config, &filter_));
  }
  ~VoxelFilter() {lfx_voxel_filter_destroy(filter_);}
  VoxelFilter(const VoxelFilter &) = delete;
  VoxelFilter & operator=(const VoxelFilter &) = delete;

  void Reset(float leaf, void * stream = nullptr) {Check(lfx_voxel_filter_reset(fx_.handle(), filter_, leaf, stream));}
  // n_points records of 4 floats on the device; read behind `stream`
  void Add(const float * d_points, std::uint64_t n_points, void * stream = nullptr)
  {
    Check(lfx_voxel_filter_add(fx_.handle(), filter_, d_points, n_points, stream));
  }
  void AddHost(const std::vector<float> & points, void * stream = nullptr)
  {
    Check(lfx_voxel_filter_add_host(fx_.handle(), filter_, points.data(), points.size() / 4u, stream));
  }
  // keyframes [first, first + count) of a store at its current poses, straight from its sensor-frame records
  void AddKeyframes(const Keyframes & keyframes, Keyframes::Kind kind, std::uint32_t first, std::uint32_t count, bool masked = false,
    void * stream = nullptr)
  {
    Check(lfx_voxel_filter_add_keyframes(fx_.handle(), filter_, keyframes.handle(), kind, first, count, masked ? 1 : 0, stream));
  }
  // the voxels with at least min_points records to d_out (device, capacity_points records), their counts to d_counts_out
  // (device, may be null).  Waits once, for the result; a full table or too small a capacity throws with nothing written.
  lfx_voxel_filter_result Emit(std::uint32_t min_points, float * d_out, std::uint64_t capacity_points, std::uint32_t * d_counts_out = nullptr,
    void * stream = nullptr)
  {
    lfx_voxel_filter_result r;
    Check(lfx_voxel_filter_emit(fx_.handle(), filter_, min_points, d_out, capacity_points, d_counts_out, &r, stream));
    return r;
  }
  lfx_voxel_filter_info_t Info() const
  {
    lfx_voxel_filter_info_t i;
    lfx_voxel_filter_info(filter_, &i);
    return i;
  }
  lfx_voxel_filter * handle() const {return filter_;}

private:
  void Check(int rc) const
  {
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(fx_.handle()));}
  }
  const FeatureExtraction & fx_;
  lfx_voxel_filter * filter_ = nullptr;
};

inline std::pair<bool, bool> Keyframes::SaveFiltered(VoxelFilter & filter, const std::string & dirname, float edge_leaf, float surface_leaf,
  std::uint32_t min_points, bool masked, void * stream) const
{
  int written[2] = {0, 0};
  const float leaf[2] = {edge_leaf, surface_leaf};
  Check(lfx_keyframes_save_filtered(fx_.handle(), store_, filter.handle(), leaf, min_points, masked ? 1 : 0, dirname.c_str(), written, stream));
  return {written[0] != 0, written[1] != 0};
}

// A 2-D occupancy grid (lfx_occupancy) on the device of `fx`, which must outlive it: Add reduces the scans the
// FeatureExtraction was last given to W beams each and keeps them with one pose per scan; Render casts the kept beams through
// the grid at the poses of the moment (SetPoses / Follow move them; Clear and Render again after a loop closure: no scan is
// read again); Emit gives nav_msgs/OccupancyGrid.data and Save the map.pgm / map.yaml pair map_server reads.
class OccupancyGrid
{
public:
  static lfx_occupancy_config DefaultConfig() {lfx_occupancy_config c; lfx_occupancy_default_config(&c); return c;}
  static lfx_occupancy_emit_config DefaultEmitConfig() {lfx_occupancy_emit_config c; lfx_occupancy_emit_default_config(&c); return c;}
  // config: DefaultConfig() with max_scans, width, height, resolution, origin_x and origin_y set
  OccupancyGrid(const FeatureExtraction & fx, const lfx_occupancy_config & config)
  : fx_(fx), config_(config)
  {
    Check(lfx_occupancy_create(fx.handle(), &config, &grid_));
  }
  ~OccupancyGrid() {lfx_occupancy_destroy(grid_);}
  OccupancyGrid(const OccupancyGrid &) = delete;
  OccupancyGrid & operator=(const OccupancyGrid &) = delete;

  // every scan the FeatureExtraction was last given, one pose (12 doubles) per scan; d_class: FeatureExtraction::Segment's
  // classes for them, or null; select: empty, or one byte per scan, 0 leaving the scan out (keyframes are a subset of scans);
  // the id of the first scan added.  Returns before the records are read: they must stay on the device until `stream` has
  // passed the call -- FeatureExtraction::BatchStatus(stream) before the next scan is handed to the extraction.
  std::uint32_t Add(const std::vector<double> & poses, const std::uint8_t * d_class = nullptr, std::uint32_t obstacle_mask = 15u,
    std::uint32_t clear_mask = 15u, void * stream = nullptr, const std::vector<std::uint8_t> & select = {})
  {
    std::uint32_t first = 0;
    const bool sized = poses.size() % 12u == 0u && (select.empty() || select.size() == poses.size() / 12u);
    Check(sized ? lfx_occupancy_add_batch(fx_.handle(), grid_, static_cast<std::uint32_t>(poses.size() / 12u), poses.data(),
      select.empty() ? nullptr : select.data(), d_class, obstacle_mask, clear_mask, &first, stream) : LFX_ERR_INVALID_ARGUMENT);
    return first;
  }
  // every scan that is a node of `graph` takes the node's pose, device to device
  void Follow(const PoseGraph & graph, void * stream = nullptr)
  {
    std::uint32_t n = 0;
    const double * d_poses = graph.View(&n, stream);
    const std::uint32_t have = Info().n_scans;
    Check(lfx_occupancy_follow(fx_.handle(), grid_, d_poses, 0, n < have ? n : have, stream));
  }
  void SetPoses(std::uint32_t first, const std::vector<double> & poses, void * stream = nullptr)
  {
    Check(poses.size() % 12u == 0u ? lfx_occupancy_set_poses(fx_.handle(), grid_, first, static_cast<std::uint32_t>(poses.size() / 12u), poses.data(), stream) :
      LFX_ERR_INVALID_ARGUMENT);
  }
  std::vector<double> Poses(std::uint32_t first, std::uint32_t count, void * stream = nullptr) const
  {
    std::vector<double> out(static_cast<std::size_t>(count) * 12u);
    Check(lfx_occupancy_poses(fx_.handle(), grid_, first, count, out.data(), stream));
    return out;
  }
  void Clear(void * stream = nullptr) {Check(lfx_occupancy_clear(fx_.handle(), grid_, stream));}
  // drops the kept scans from n_scans on (the counts stay): a small grid as the reducer of live scans starts every batch with Truncate(0)
  void Truncate(std::uint32_t n_scans, void * stream = nullptr) {Check(lfx_occupancy_truncate(fx_.handle(), grid_, n_scans, stream));}
  void Render(std::uint32_t first, std::uint32_t count, void * stream = nullptr) {Check(lfx_occupancy_render(fx_.handle(), grid_, first, count, stream));}
  // a full re-render: every kept scan at its current pose
  void RenderAll(void * stream = nullptr)
  {
    Clear(stream);
    Render(0, Info().n_scans, stream);
  }
  lfx_occupancy_counters_t Counters(void * stream = nullptr) const
  {
    lfx_occupancy_counters_t r;
    Check(lfx_occupancy_counters(fx_.handle(), grid_, &r, stream));
    return r;
  }
  // int8 [height][width], row 0 the lowest y, to device memory or a pinned block (FeatureExtraction::PinnedFloats); returns
  // before it is written: read it behind `stream`
  void Emit(std::int8_t * out, const lfx_occupancy_emit_config & config = DefaultEmitConfig(), void * stream = nullptr)
  {
    Check(lfx_occupancy_emit(fx_.handle(), grid_, &config, out, stream));
  }
  void Save(const std::string & dirname, int occupied_percent = 65, int free_percent = 25, const lfx_occupancy_emit_config & config = DefaultEmitConfig(),
    void * stream = nullptr)
  {
    Check(lfx_occupancy_save(fx_.handle(), grid_, &config, dirname.c_str(), occupied_percent, free_percent, stream));
  }
  lfx_occupancy_info_t Info() const
  {
    lfx_occupancy_info_t i;
    lfx_occupancy_info(grid_, &i);
    return i;
  }
  const lfx_occupancy_config & Config() const {return config_;}
  lfx_occupancy * handle() const {return grid_;}

private:
  void Check(int rc) const
  {
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(fx_.handle()));}
  }
  const FeatureExtraction & fx_;
  lfx_occupancy_config config_;
  lfx_occupancy * grid_ = nullptr;
};

// A distance field (lfx_distance) over grids of width x height cells on the device of `fx`, which must outlive it: a
// transform (FromGrid of an int8 grid on the device, FromOccupancy of an OccupancyGrid's counts as they stand) gives the
// exact squared distance of every cell to the nearest obstacle cell; Metres and Costmap turn the last transform into an ESDF
// and into nav2's inflated costs.  After a loop closure: OccupancyGrid::Follow, RenderAll, then one FromOccupancy.
class DistanceField
{
public:
  static lfx_distance_config DefaultConfig() {lfx_distance_config c; lfx_distance_default_config(&c); return c;}
  static lfx_distance_cost_config DefaultCostConfig() {lfx_distance_cost_config c; lfx_distance_cost_default_config(&c); return c;}
  // lfx_distance_cost_table: the bytes the costmap kernel is handed (host only)
  static std::vector<std::uint8_t> CostTable(const lfx_distance_cost_config & config, float resolution)
  {
    std::uint32_t n = 0;
    if (lfx_distance_cost_table_size(&config, resolution, &n) != LFX_OK) {throw Error(LFX_ERR_INVALID_ARGUMENT, "the cost config is refused");}
    std::vector<std::uint8_t> lut(n);
    if (lfx_distance_cost_table(&config, resolution, lut.data(), n) != LFX_OK) {throw Error(LFX_ERR_INVALID_ARGUMENT, "the cost config is refused");}
    return lut;
  }
  DistanceField(const FeatureExtraction & fx, std::uint32_t width, std::uint32_t height)
  : fx_(fx)
  {
    Check(lfx_distance_create(fx.handle(), width, height, &field_));
  }
  ~DistanceField() {lfx_distance_destroy(field_);}
  DistanceField(const DistanceField &) = delete;
  DistanceField & operator=(const DistanceField &) = delete;

  // d_grid: int8 [height][width] on the device, lfx_occupancy_emit's format; read behind `stream`
  void FromGrid(const std::int8_t * d_grid, const lfx_distance_config & config = DefaultConfig(), void * stream = nullptr)
  {
    Check(lfx_distance_from_grid(fx_.handle(), field_, d_grid, &config, stream));
  }
  // the bytes grid.Emit(emit_config) would write, transformed without being written
  void FromOccupancy(OccupancyGrid & grid, const lfx_distance_config & config = DefaultConfig(),
    const lfx_occupancy_emit_config & emit_config = OccupancyGrid::DefaultEmitConfig(), void * stream = nullptr)
  {
    Check(lfx_distance_from_occupancy(fx_.handle(), field_, grid.handle(), &emit_config, &config, stream));
  }
  // the device arrays, current behind `stream`; i2 is null unless the last transform had `inside`
  lfx_distance_view_t View(void * stream = nullptr) const
  {
    lfx_distance_view_t v;
    Check(lfx_distance_view(fx_.handle(), field_, &v, stream));
    return v;
  }
  // float / uint8 [height][width] to device memory or a pinned block (FeatureExtraction::PinnedFloats); both return before
  // the output is written: read it behind `stream`
  void Metres(float resolution, float * out, void * stream = nullptr) {Check(lfx_distance_metres(fx_.handle(), field_, resolution, out, stream));}
  void Costmap(float resolution, std::uint8_t * out, const lfx_distance_cost_config & config = DefaultCostConfig(), void * stream = nullptr)
  {
    Check(lfx_distance_costmap(fx_.handle(), field_, &config, resolution, out, stream));
  }
  lfx_distance_stats_t Stats(void * stream = nullptr) const
  {
    lfx_distance_stats_t s;
    Check(lfx_distance_stats(fx_.handle(), field_, &s, stream));
    return s;
  }
  lfx_distance_info_t Info() const
  {
    lfx_distance_info_t i;
    lfx_distance_info(field_, &i);
    return i;
  }
  lfx_distance * handle() const {return field_;}

private:
  void Check(int rc) const
  {
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(fx_.handle()));}
  }
  const FeatureExtraction & fx_;
  lfx_distance * field_ = nullptr;
};

// A scan matcher over an occupancy grid (lfx_grid_match) on the device of `fx`, which must outlive it: SetField takes a
// DistanceField's last transform through a score table, SetScans an OccupancyGrid's kept scans; Score rates arbitrary
// candidate poses (a particle filter's measurement update), Search a window of whole-cell shifts and headings around a centre
// (relocalisation, tracking, a 2-D loop check).  Candidate and Pose3 turn the index found into the initial pose the 3-D
// alignment asks for.  Outputs go to device memory or a pinned block (FeatureExtraction::PinnedFloats), read behind `stream`.
class GridMatcher
{
public:
  struct Best {std::uint32_t score, index, inside, n_points;};
  static lfx_grid_match_config DefaultConfig() {lfx_grid_match_config c; lfx_grid_match_default_config(&c); return c;}
  static lfx_grid_match_table_config DefaultTableConfig() {lfx_grid_match_table_config c; lfx_grid_match_table_default_config(&c); return c;}
  static lfx_grid_match_search_config DefaultSearchConfig() {lfx_grid_match_search_config c; lfx_grid_match_search_default_config(&c); return c;}
  // lfx_grid_match_table: the values the field kernel is handed (host only)
  static std::vector<std::uint16_t> Table(const lfx_grid_match_table_config & config, float resolution)
  {
    std::uint32_t n = 0;
    if (lfx_grid_match_table_size(&config, resolution, &n) != LFX_OK) {throw Error(LFX_ERR_INVALID_ARGUMENT, "the score table config is refused");}
    std::vector<std::uint16_t> lut(n);
    if (lfx_grid_match_table(&config, resolution, lut.data(), n) != LFX_OK) {throw Error(LFX_ERR_INVALID_ARGUMENT, "the score table config is refused");}
    return lut;
  }
  // {x, y, yaw} of candidate `index` of a search around `centre` (host only)
  static std::array<double, 3> Candidate(const lfx_grid_match_search_config & search, float resolution, const std::array<double, 3> & centre, std::uint32_t index)
  {
    std::array<double, 3> pose2{};
    if (lfx_grid_match_candidate(&search, resolution, centre.data(), index, pose2.data()) != LFX_OK) {throw Error(LFX_ERR_INVALID_ARGUMENT, "no such candidate");}
    return pose2;
  }
  // [Rz(yaw) x level | (x, y, z)], 12 doubles; level: 9 doubles or null = identity (host only)
  static std::array<double, 12> Pose3(const std::array<double, 3> & pose2, const double * level = nullptr, double z = 0.0)
  {
    std::array<double, 12> pose{};
    lfx_grid_match_pose3(pose2.data(), level, z, pose.data());
    return pose;
  }
  // config: DefaultConfig() with width, height, resolution, origin_x and origin_y set
  GridMatcher(const FeatureExtraction & fx, const lfx_grid_match_config & config)
  : fx_(fx), config_(config)
  {
    Check(lfx_grid_match_create(fx.handle(), &config, &matcher_));
  }
  ~GridMatcher() {lfx_grid_match_destroy(matcher_);}
  GridMatcher(const GridMatcher &) = delete;
  GridMatcher & operator=(const GridMatcher &) = delete;

  void SetField(DistanceField & field, const std::vector<std::uint16_t> & lut, void * stream = nullptr)
  {
    Check(lfx_grid_match_set_field(fx_.handle(), matcher_, field.handle(), lut.data(), static_cast<std::uint32_t>(lut.size()), stream));
  }
  void SetField(DistanceField & field, const lfx_grid_match_table_config & table = DefaultTableConfig(), void * stream = nullptr)
  {
    SetField(field, Table(table, config_.resolution), stream);
  }
  // the store's scans [first, first + count), levelled by the rotations of the poses it holds now (use_rotation) or not at all
  void SetScans(OccupancyGrid & grid, std::uint32_t first, std::uint32_t count, bool use_rotation = true, void * stream = nullptr)
  {
    Check(lfx_grid_match_set_scans_occupancy(fx_.handle(), matcher_, grid.handle(), first, count, use_rotation ? 1 : 0, stream));
  }
  // d_beams: device [n_scans][n_beams][4] as lfx_occupancy_view_t.beams; levels: empty, or 9 doubles per scan
  void SetScans(const float * d_beams, std::uint32_t n_scans, std::uint32_t n_beams, const std::vector<double> & levels = {}, void * stream = nullptr)
  {
    Check(levels.empty() || levels.size() == 9u * static_cast<std::size_t>(n_scans) ?
      lfx_grid_match_set_scans(fx_.handle(), matcher_, d_beams, n_scans, n_beams, levels.empty() ? nullptr : levels.data(), stream) : LFX_ERR_INVALID_ARGUMENT);
  }
  // d_candidates: double [n][4] = {tx, ty, cos, sin}; d_score, d_inside (may be null): uint32 [n]
  void Score(std::uint32_t scan, const double * d_candidates, std::uint32_t n, std::uint32_t * d_score, std::uint32_t * d_inside = nullptr, void * stream = nullptr)
  {
    Check(lfx_grid_match_score(fx_.handle(), matcher_, scan, d_candidates, n, d_score, d_inside, stream));
  }
  // centres: {x0, y0, yaw0} per scan of [first, first + centres.size() / 3); d_best: uint32 [n][4]; the others may be null
  void Search(std::uint32_t first, const std::vector<double> & centres, const lfx_grid_match_search_config & search, std::uint32_t * d_best,
    std::uint32_t * d_slice_best = nullptr, std::uint32_t * d_volume = nullptr, void * stream = nullptr)
  {
    Check(centres.size() % 3u == 0u ? lfx_grid_match_search(fx_.handle(), matcher_, first, static_cast<std::uint32_t>(centres.size() / 3u), centres.data(), &search,
      d_best, d_slice_best, d_volume, stream) : LFX_ERR_INVALID_ARGUMENT);
  }
  lfx_grid_match_info_t Info() const
  {
    lfx_grid_match_info_t i;
    lfx_grid_match_info(matcher_, &i);
    return i;
  }
  const lfx_grid_match_config & Config() const {return config_;}
  lfx_grid_match * handle() const {return matcher_;}

private:
  void Check(int rc) const
  {
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(fx_.handle()));}
  }
  const FeatureExtraction & fx_;
  lfx_grid_match_config config_;
  lfx_grid_match * matcher_ = nullptr;
};

// Visibility votes (lfx_visibility): which records of a window of a Keyframes store's keyframes were looked through by the
// keyframes near them, and the DYNAMIC flag that decides.  None of the defaults is measured on real data.
class Visibility
{
public:
  static lfx_visibility_config DefaultConfig()
  {
    lfx_visibility_config config;
    lfx_visibility_default_config(&config);
    return config;
  }
  Visibility(const FeatureExtraction & fx, const lfx_visibility_config & config, std::uint32_t max_window, std::uint32_t max_resident_images)
  : fx_(fx)
  {
    Check(lfx_visibility_create(fx.handle(), &config, max_window, max_resident_images, &vis_));
  }
  ~Visibility() {lfx_visibility_destroy(vis_);}
  Visibility(const Visibility &) = delete;
  Visibility & operator=(const Visibility &) = delete;

  // the votes of keyframes [first, first + count) on each other: d_flags[kind] (device u8, required) and d_votes[kind] (device
  // u32, either may be null) addressed by the store's record index of the kind.  Waits once, for the result.
  lfx_visibility_result Run(const Keyframes & keyframes, std::uint32_t first, std::uint32_t count, std::uint32_t * const d_votes[2],
    std::uint8_t * const d_flags[2], void * stream = nullptr)
  {
    lfx_visibility_result r;
    Check(lfx_visibility_run(fx_.handle(), vis_, keyframes.handle(), first, count, d_votes, d_flags, &r, stream));
    return r;
  }
  lfx_visibility_info_t Info() const
  {
    lfx_visibility_info_t i;
    lfx_visibility_info(vis_, &i);
    return i;
  }
  lfx_visibility * handle() const {return vis_;}

private:
  void Check(int rc) const
  {
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(fx_.handle()));}
  }
  const FeatureExtraction & fx_;
  lfx_visibility * vis_ = nullptr;
};

// The loop closer (lfx_loop_closer): revisits found in a PlaceDb, verified against submaps of a Keyframes store and closed in
// a PoseGraph, all three on the device of `fx` and all of them outliving it.  THE CONTRACT: keyframe id == place entry ==
// graph node id (add to the three in step).  Update(first, count) is the whole loop: detect, verify, add the accepted edges,
// optimise, make the store follow.  The thresholds on rms and inliers ship permissive (no measured default).
class LoopCloser
{
public:
  static lfx_loop_closer_config DefaultConfig(std::uint64_t edge_submap_capacity, std::uint64_t surface_submap_capacity)
  {
    lfx_loop_closer_config c;
    lfx_loop_closer_default_config(&c);
    c.submap_capacity[0] = edge_submap_capacity;
    c.submap_capacity[1] = surface_submap_capacity;
    return c;
  }
  LoopCloser(const FeatureExtraction & fx, const lfx_loop_closer_config & config, Keyframes & keyframes, PlaceDb & db, PoseGraph & graph)
  : fx_(fx), config_(config)
  {
    Check(lfx_loop_closer_create(fx.handle(), &config, keyframes.handle(), db.handle(), graph.handle(), &closer_));
  }
  ~LoopCloser() {lfx_loop_closer_destroy(closer_);}
  LoopCloser(const LoopCloser &) = delete;
  LoopCloser & operator=(const LoopCloser &) = delete;

  // the candidates of keyframes first .. first + count - 1: [count][n_candidates], best first, the empty match where none is left
  std::vector<lfx_place_match> Detect(std::uint32_t first, std::uint32_t count, std::vector<std::uint32_t> * n_eligible = nullptr, void * stream = nullptr)
  {
    std::vector<lfx_place_match> out(static_cast<std::size_t>(count) * config_.n_candidates);
    if (n_eligible) {n_eligible->assign(count, 0u);}
    Check(lfx_loop_closer_detect(fx_.handle(), closer_, first, count, out.data(), n_eligible ? n_eligible->data() : nullptr, stream));
    return out;
  }
  lfx_loop_closure Verify(std::uint32_t query_id, const lfx_place_match & candidate, void * stream = nullptr)
  {
    lfx_loop_closure out;
    Check(lfx_loop_closer_verify(fx_.handle(), closer_, query_id, &candidate, &out, stream));
    return out;
  }
  // closures: one per keyframe of the range (its last verification)
  lfx_loop_closer_result Update(std::uint32_t first, std::uint32_t count, std::vector<lfx_loop_closure> & closures, void * stream = nullptr)
  {
    lfx_loop_closer_result r;
    closures.resize(count);
    Check(lfx_loop_closer_update(fx_.handle(), closer_, first, count, closures.data(), &r, stream));
    return r;
  }
  lfx_loop_closer_info_t Info() const
  {
    lfx_loop_closer_info_t i;
    lfx_loop_closer_info(closer_, &i);
    return i;
  }
  // verify against submaps without the store's flagged records (the store has reserved flags: Keyframes::ReserveFlags); the
  // query keyframe's own clouds are used as stored
  void SetMasked(bool masked = true)
  {
    const int rc = lfx_loop_closer_set_masked(closer_, masked ? 1 : 0);
    if (rc != LFX_OK) {throw Error(rc, "SetMasked: the closer's store has no flags reserved");}
  }
  bool Masked() const
  {
    int m = 0;
    lfx_loop_closer_get_masked(closer_, &m);
    return m != 0;
  }

private:
  void Check(int rc) const
  {
    if (rc != LFX_OK) {throw Error(rc, lfx_last_error(fx_.handle()));}
  }
  const FeatureExtraction & fx_;
  lfx_loop_closer_config config_;
  lfx_loop_closer * closer_ = nullptr;
};

}  // namespace lfx
#endif  // LFX_HPP_
