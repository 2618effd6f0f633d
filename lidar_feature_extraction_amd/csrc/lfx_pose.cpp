// lfx_pose.cpp -- the pose arithmetic of the host, no device and no context: the keyframe test of the mapping node
// (lfx_pose_diff), the motions and trajectories of the de-skew section (lfx_motion_*, lfx_trajectory_*), a report's
// covariance in ROS order (include/lfx.h).  Plain C++ with no HIP header, contraction off: tests/test_trajectory_host.py
// builds it on its own under AddressSanitizer and UndefinedBehaviorSanitizer.
#include "../../include/lfx.h"
#include "lfx_deskew_rows.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

static_assert(lfx::kTrjStride == LFX_TRAJECTORY_SEGMENT_DOUBLES && lfx::kDskStride == lfx::kTrjStride, "a row is what lfx.h says a segment takes");

extern "C" {

// PoseDiffIsSufficientlySmall's two quantities (map.hpp:49-60) in Eigen 3.4's order of operations (include/lfx.h)
int lfx_pose_diff(const double pose0[12], const double pose1[12], double * translation, double * rotation)
{
  if (!pose0 || !pose1 || !translation || !rotation) {return LFX_ERR_INVALID_ARGUMENT;}
  auto R0 = [&](int r, int c) {return pose0[4 * r + c];};
  auto R1 = [&](int r, int c) {return pose1[4 * r + c];};
  double m[3][3], t[3];
  for (int r = 0; r < 3; r++) {
    // (R0^T)(r, k) = R0(k, r)
    const double inv_t = -((R0(0, r) * pose0[3] + R0(1, r) * pose0[7]) + R0(2, r) * pose0[11]);
    t[r] = ((R0(0, r) * pose1[3] + R0(1, r) * pose1[7]) + R0(2, r) * pose1[11]) + inv_t;
    for (int c = 0; c < 3; c++) {m[r][c] = (R0(0, r) * R1(0, c) + R0(1, r) * R1(1, c)) + R0(2, r) * R1(2, c);}
  }
  *translation = std::sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
  // Quaterniond(d.rotation()): Shoemake's algorithm as Eigen writes it (q.vec() only)
  double q[3];
  const double tr = (m[0][0] + m[1][1]) + m[2][2];
  if (tr > 0.0) {
    const double s = 0.5 / std::sqrt(tr + 1.0);
    q[0] = (m[2][1] - m[1][2]) * s;
    q[1] = (m[0][2] - m[2][0]) * s;
    q[2] = (m[1][0] - m[0][1]) * s;
  } else {
    int i = 0;
    if (m[1][1] > m[0][0]) {i = 1;}
    if (m[2][2] > m[i][i]) {i = 2;}
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    const double s0 = std::sqrt(((m[i][i] - m[j][j]) - m[k][k]) + 1.0);
    q[i] = 0.5 * s0;
    const double s = 0.5 / s0;
    q[j] = (m[j][i] + m[i][j]) * s;
    q[k] = (m[k][i] + m[i][k]) * s;
  }
  *rotation = std::sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
  return LFX_OK;
}

// The motions of the de-skew section (include/lfx.h): pose0^-1 pose1 as lfx_pose_diff forms it, its angle-axis vector, a
// fraction of it.
int lfx_motion_between(const double pose0[12], const double pose1[12], double motion[12])
{
  if (!pose0 || !pose1 || !motion) {return LFX_ERR_INVALID_ARGUMENT;}
  auto R0 = [&](int r, int c) {return pose0[4 * r + c];};
  auto R1 = [&](int r, int c) {return pose1[4 * r + c];};
  double out[12];                                     // (motion may be one of the poses)
  bool same = true;
  for (int i = 0; i < 12; i++) {same = same && pose0[i] == pose1[i];}
  if (same) {
    // a sensor that has not moved: the identity itself, not R0^T R0 as it rounds (de-skew by it changes no bit)
    const double identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    std::memcpy(motion, identity, sizeof(identity));
    return LFX_OK;
  }
  for (int r = 0; r < 3; r++) {
    const double inv_t = -((R0(0, r) * pose0[3] + R0(1, r) * pose0[7]) + R0(2, r) * pose0[11]);
    out[4 * r + 3] = ((R0(0, r) * pose1[3] + R0(1, r) * pose1[7]) + R0(2, r) * pose1[11]) + inv_t;
    for (int c = 0; c < 3; c++) {out[4 * r + c] = (R0(0, r) * R1(0, c) + R0(1, r) * R1(1, c)) + R0(2, r) * R1(2, c);}
  }
  std::memcpy(motion, out, sizeof(out));
  return LFX_OK;
}

int lfx_motion_twist(const double motion[12], double w[3], double * theta)
{
  if (!motion || !w || !theta) {return LFX_ERR_INVALID_ARGUMENT;}
  auto m = [&](int r, int c) {return motion[4 * r + c];};
  // Quaterniond(R_D), Shoemake's algorithm as Eigen writes it (lfx_pose_diff), with its scalar part
  double q[3], qw;
  const double tr = (m(0, 0) + m(1, 1)) + m(2, 2);
  if (tr > 0.0) {
    const double t = std::sqrt(tr + 1.0);
    qw = 0.5 * t;
    const double s = 0.5 / t;
    q[0] = (m(2, 1) - m(1, 2)) * s;
    q[1] = (m(0, 2) - m(2, 0)) * s;
    q[2] = (m(1, 0) - m(0, 1)) * s;
  } else {
    int i = 0;
    if (m(1, 1) > m(0, 0)) {i = 1;}
    if (m(2, 2) > m(i, i)) {i = 2;}
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    const double t = std::sqrt(((m(i, i) - m(j, j)) - m(k, k)) + 1.0);
    q[i] = 0.5 * t;
    const double s = 0.5 / t;
    qw = (m(k, j) - m(j, k)) * s;
    q[j] = (m(j, i) + m(i, j)) * s;
    q[k] = (m(k, i) + m(i, k)) * s;
  }
  const double n = std::sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
  if (n == 0.0) {
    w[0] = w[1] = w[2] = 0.0;
    *theta = 0.0;
    return LFX_OK;
  }
  const double th = 2.0 * std::atan2(n, qw), f = th / n;
  w[0] = q[0] * f; w[1] = q[1] * f; w[2] = q[2] * f;
  *theta = th;
  return LFX_OK;
}

// the rotation of the angle-axis vector ratio * w (theta = |w|) into res's 3 x 3, as the de-skew kernels form it
static void rotation_of(const double w[3], double theta, double ratio, double res[12])
{
  if (theta < 1e-8) {
    const double x = ratio * w[0], y = ratio * w[1], z = ratio * w[2];
    const double r[9] = {1.0, 0.0 - z, y, z, 1.0, 0.0 - x, 0.0 - y, x, 1.0};   // (0 - 0: no negative zero for the identity)
    for (int i = 0; i < 3; i++) {for (int j = 0; j < 3; j++) {res[4 * i + j] = r[3 * i + j];}}
  } else {
    const double k[3] = {w[0] / theta, w[1] / theta, w[2] / theta};
    const double a = ratio * theta, c = std::cos(a), s = std::sin(a), v = 1.0 - c;
    const double hat[9] = {0.0, -k[2], k[1], k[2], 0.0, -k[0], -k[1], k[0], 0.0};
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) {res[4 * i + j] = ((i == j ? c : 0.0) + hat[3 * i + j] * s) + k[i] * (k[j] * v);}
    }
  }
}

int lfx_motion_scale(const double motion[12], double ratio, double out[12])
{
  if (!motion || !out) {return LFX_ERR_INVALID_ARGUMENT;}
  double w[3], theta;
  lfx_motion_twist(motion, w, &theta);
  double res[12];                                     // (out may be motion)
  rotation_of(w, theta, ratio, res);
  for (int i = 0; i < 3; i++) {res[4 * i + 3] = ratio * motion[4 * i + 3];}
  std::memcpy(out, res, sizeof(res));
  return LFX_OK;
}

// The trajectories of the de-skew section (include/lfx.h): the segment table of one, knots from gyro samples.
// the rotation of pose a times that of b, every sum (a0 b0 + a1 b1) + a2 b2, into out's 3 x 3
static void rotate(const double a[12], const double b[12], double out[12])
{
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) {out[4 * r + c] = (a[4 * r] * b[c] + a[4 * r + 1] * b[4 + c]) + a[4 * r + 2] * b[8 + c];}
  }
}

int lfx_trajectory_segments(const lfx_trajectory * tr, double * segments_out)
{
  if (!tr || !segments_out || !tr->times || !tr->poses) {return LFX_ERR_INVALID_ARGUMENT;}
  const uint32_t n = tr->n_knots;
  if (n < 2u || n > LFX_MAX_TRAJECTORY_KNOTS) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!lfx::ascending_times(tr->times, n) || !lfx::finite_run(tr->poses, 12 * (size_t)n) || !std::isfinite(tr->t_ref)) {return LFX_ERR_INVALID_ARGUMENT;}
  const double * t = tr->times, * P = tr->poses;
  // the reference pose: a knot's own where t_ref is a knot time, else the model's at t_ref
  double ref[12];
  uint32_t at = 0;                                    // knots with times[k] <= t_ref
  while (at < n && t[at] <= tr->t_ref) {at++;}
  if (at > 0u && t[at - 1] == tr->t_ref) {
    std::memcpy(ref, P + 12 * (size_t)(at - 1), sizeof(ref));
  } else {
    const uint32_t j = std::min(std::max(at, 1u) - 1u, n - 2u);
    const double * a = P + 12 * (size_t)j, * b = a + 12;
    const double beta = (tr->t_ref - t[j]) * (1.0 / (t[j + 1] - t[j]));
    double D[12], S[12];
    lfx_motion_between(a, b, D);
    lfx_motion_scale(D, beta, S);
    rotate(a, S, ref);
    for (int i = 0; i < 3; i++) {ref[4 * i + 3] = a[4 * i + 3] + beta * (b[4 * i + 3] - a[4 * i + 3]);}
  }
  double Q[2][12];                                    // Q_j and Q_{j+1}, swapped as the segments go by
  lfx_motion_between(ref, P, Q[0]);
  for (uint32_t j = 0; j + 1 < n; j++) {
    const double * q0 = Q[j & 1u];
    double * q1 = Q[(j + 1u) & 1u], * T = segments_out + (size_t)lfx::kTrjStride * j;
    lfx_motion_between(ref, P + 12 * (size_t)(j + 1), q1);
    double D[12], w[3], theta;
    lfx_motion_between(q0, q1, D);
    lfx_motion_twist(D, w, &theta);
    lfx::write_twist(T, w, theta);
    for (int a = 0; a < 3; a++) {
      for (int c = 0; c < 3; c++) {T[lfx::kTrjA + 3 * a + c] = q0[4 * a + c];}
      T[lfx::kTrjQ + a] = q0[4 * a + 3];
      T[lfx::kTrjDq + a] = q1[4 * a + 3] - q0[4 * a + 3];
    }
    T[lfx::kTrjTime] = t[j];
    T[lfx::kTrjInvDt] = 1.0 / (t[j + 1] - t[j]);
  }
  return LFX_OK;
}

int lfx_trajectory_from_gyro(const double * times, const double * rates, uint32_t n, const double bias[3], const double velocity[3],
  double * poses_out)
{
  if (!times || !rates || !poses_out || n < 2u) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!lfx::ascending_times(times, n) || !lfx::finite_run(rates, 3 * (size_t)n)) {return LFX_ERR_INVALID_ARGUMENT;}
  if ((bias && !lfx::finite_run(bias, 3)) || (velocity && !lfx::finite_run(velocity, 3))) {return LFX_ERR_INVALID_ARGUMENT;}
  const double identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  std::memcpy(poses_out, identity, sizeof(identity));
  for (uint32_t j = 0; j + 1 < n; j++) {
    const double * r0 = rates + 3 * (size_t)j, * r1 = r0 + 3, * a = poses_out + 12 * (size_t)j;
    double * b = poses_out + 12 * (size_t)(j + 1), phi[3], E[12];
    const double dt = times[j + 1] - times[j];
    for (int i = 0; i < 3; i++) {
      const double bi = bias ? bias[i] : 0.0;
      phi[i] = (0.5 * ((r0[i] - bi) + (r1[i] - bi))) * dt;
    }
    rotation_of(phi, std::sqrt((phi[0] * phi[0] + phi[1] * phi[1]) + phi[2] * phi[2]), 1.0, E);
    rotate(a, E, b);
    for (int i = 0; i < 3; i++) {b[4 * i + 3] = velocity ? velocity[i] * (times[j + 1] - times[0]) : 0.0;}
  }
  return LFX_OK;
}

// A report's covariance in the order of geometry_msgs/PoseWithCovariance (include/lfx.h): out = T C T^T, T = [[0, I], [R, 0]].
// Every sum of three terms is (a0 b0 + a1 b1) + a2 b2 (this file is built with contraction off).
int lfx_align_covariance_ros(const double pose[12], const double covariance[36], double out[36])
{
  if (!pose || !covariance || !out) {return LFX_ERR_INVALID_ARGUMENT;}
  auto R = [&](int r, int c) {return pose[4 * r + c];};
  double tc[36];                                      // T C: rows 0-2 = C's translation rows, rows 3-5 = R times its rotation rows
  for (int c = 0; c < 6; c++) {
    for (int i = 0; i < 3; i++) {
      tc[6 * i + c] = covariance[6 * (3 + i) + c];
      tc[6 * (3 + i) + c] = (R(i, 0) * covariance[c] + R(i, 1) * covariance[6 + c]) + R(i, 2) * covariance[12 + c];
    }
  }
  double res[36];                                     // (out may be covariance)
  for (int r = 0; r < 6; r++) {
    for (int j = 0; j < 3; j++) {
      res[6 * r + j] = tc[6 * r + 3 + j];
      res[6 * r + 3 + j] = (tc[6 * r] * R(j, 0) + tc[6 * r + 1] * R(j, 1)) + tc[6 * r + 2] * R(j, 2);
    }
  }
  std::memcpy(out, res, sizeof(res));
  return LFX_OK;
}

// A report's information in a pose-graph edge's residual coordinates (include/lfx.h): out = B H B^T, B = blkdiag(I, R^T).
// Every sum of three terms is (a0 b0 + a1 b1) + a2 b2.
int lfx_pose_graph_edge_information(const double pose_j[12], const double report_information[36], double out[36])
{
  if (!pose_j || !report_information || !out) {return LFX_ERR_INVALID_ARGUMENT;}
  auto R = [&](int r, int c) {return pose_j[4 * r + c];};
  const double * H = report_information;
  double bh[36];                                      // B H: rows 0-2 = H's rotation rows, rows 3-5 = R^T times its translation rows
  for (int c = 0; c < 6; c++) {
    for (int i = 0; i < 3; i++) {
      bh[6 * i + c] = H[6 * i + c];
      bh[6 * (3 + i) + c] = (R(0, i) * H[18 + c] + R(1, i) * H[24 + c]) + R(2, i) * H[30 + c];
    }
  }
  double res[36];                                     // (out may be report_information)
  for (int r = 0; r < 6; r++) {
    for (int j = 0; j < 3; j++) {
      res[6 * r + j] = bh[6 * r + j];
      res[6 * r + 3 + j] = (bh[6 * r + 3] * R(0, j) + bh[6 * r + 4] * R(1, j)) + bh[6 * r + 5] * R(2, j);
    }
  }
  std::memcpy(out, res, sizeof(res));
  return LFX_OK;
}

// The covariance of the residual of an edge (i, j, Z = T_i^-1 T_j) at the current poses, from the two nodes' joint covariance
// (include/lfx.h): out = [A_i A_j] joint [A_i A_j]^T with the Jacobians at phi = 0, where Jri = I, R_Z^T R_i^T = R_j^T and
// R_Z^T = R_j^T R_i.  Every sum of three terms is (a0 b0 + a1 b1) + a2 b2; the sums over the twelve increments run left to
// right; the lower triangle is computed and mirrored.
int lfx_pose_graph_relative_covariance(const double pose_i[12], const double pose_j[12], const double joint[144], double out[36])
{
  if (!pose_i || !pose_j || !joint || !out) {return LFX_ERR_INVALID_ARGUMENT;}
  auto Ri = [&](int r, int c) {return pose_i[4 * r + c];};
  auto Rj = [&](int r, int c) {return pose_j[4 * r + c];};
  const double dt[3] = {pose_j[3] - pose_i[3], pose_j[7] - pose_i[7], pose_j[11] - pose_i[11]};
  double d[3], M[9], dx[9];                           // d = R_i^T (t_j - t_i), M = R_j^T R_i = R_Z^T
  for (int r = 0; r < 3; r++) {d[r] = (Ri(0, r) * dt[0] + Ri(1, r) * dt[1]) + Ri(2, r) * dt[2];}
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) {M[3 * r + c] = (Rj(0, r) * Ri(0, c) + Rj(1, r) * Ri(1, c)) + Rj(2, r) * Ri(2, c);}
  }
  dx[0] = 0.0; dx[1] = -d[2]; dx[2] = d[1]; dx[3] = d[2]; dx[4] = 0.0; dx[5] = -d[0]; dx[6] = -d[1]; dx[7] = d[0]; dx[8] = 0.0;
  double A[72] = {0.0};                               // [A_i A_j], 6 x 12
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) {
      A[12 * r + c] = -M[3 * r + c];
      A[12 * (3 + r) + c] = (M[3 * r] * dx[c] + M[3 * r + 1] * dx[3 + c]) + M[3 * r + 2] * dx[6 + c];
      A[12 * (3 + r) + 3 + c] = -Rj(c, r);
      A[12 * r + 6 + c] = r == c ? 1.0 : 0.0;
      A[12 * (3 + r) + 9 + c] = Rj(c, r);
    }
  }
  double AS[72];                                      // A joint
  for (int r = 0; r < 6; r++) {
    for (int c = 0; c < 12; c++) {
      double acc = 0.0;
      for (int m = 0; m < 12; m++) {acc += A[12 * r + m] * joint[12 * m + c];}
      AS[12 * r + c] = acc;
    }
  }
  for (int r = 0; r < 6; r++) {
    for (int c = 0; c <= r; c++) {
      double acc = 0.0;
      for (int m = 0; m < 12; m++) {acc += AS[12 * r + m] * A[12 * c + m];}
      out[6 * r + c] = acc;
      out[6 * c + r] = acc;
    }
  }
  return LFX_OK;
}

// What the three azimuth-binned subsystems below share (the device's side: lfx_kernels_image.hpp).  Direction m of W is
// -pi + 2 pi m / W: the first half of the table is the half circle y < 0, the second (from m = W / 2, angle 0) y >= 0.
static void azimuth_table(uint32_t W, double * cos_out, double * sin_out)
{
  for (uint32_t m = 0; m < W; m++) {
    const double angle = -M_PI + ((2.0 * M_PI) * (double)m) / (double)W;
    cos_out[m] = std::cos(angle);
    sin_out[m] = std::sin(angle);
  }
}

// a range image's rows, columns and ranges: what the segmentation and the visibility votes both ask of a config
static bool range_image_ok(uint32_t H, uint32_t W, float min_range, float max_range)
{
  if (H < 1u || H > LFX_SEGMENT_MAX_ROWS || W < 4u || W > LFX_SEGMENT_MAX_COLUMNS || (W & 1u)) {return false;}
  return std::isfinite(min_range) && std::isfinite(max_range) && min_range > 0.0f && min_range < max_range;
}

// Scan-context descriptors (include/lfx.h, the place recognition section): the defaults, and the tables the kernel is given.
void lfx_scan_context_default_config(lfx_scan_context_config * config)
{
  if (!config) {return;}
  *config = lfx_scan_context_config{};
  config->n_rings = 20;
  config->n_sectors = 60;
  config->max_radius = 80.0f;
  config->min_radius = 0.1f;
  config->sensor_height = 2.0f;
}

int lfx_scan_context_tables(const lfx_scan_context_config * config, double * sector_cos, double * sector_sin, double * ring_r2)
{
  if (!config || !sector_cos || !sector_sin || !ring_r2) {return LFX_ERR_INVALID_ARGUMENT;}
  const uint32_t R = config->n_rings, S = config->n_sectors;
  if (R < 1u || R > LFX_SCAN_CONTEXT_MAX_RINGS || S < 4u || S > LFX_SCAN_CONTEXT_MAX_SECTORS || (S & 1u)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!std::isfinite(config->max_radius) || !std::isfinite(config->min_radius) || !std::isfinite(config->sensor_height)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!(config->min_radius >= 0.0f) || !(config->min_radius < config->max_radius)) {return LFX_ERR_INVALID_ARGUMENT;}
  azimuth_table(S, sector_cos, sector_sin);
  for (uint32_t j = 0; j <= R; j++) {
    const double e = ((double)config->max_radius * (double)j) / (double)R;
    ring_r2[j] = e * e;
  }
  return LFX_OK;
}

// Scan segmentation (include/lfx.h, the segmentation section): the defaults, and the tables the kernels are given.
void lfx_segment_default_config(lfx_segment_config * config)
{
  if (!config) {return;}
  *config = lfx_segment_config{};
  config->n_rows = 16;
  config->n_columns = 1800;
  config->row_step = 0.034906585f;
  config->min_range = 1.0f;
  config->max_range = 100.0f;
  config->ground_first_row = 0;
  config->ground_last_row = 7;
  config->ground_tan = 0.17632698f;
  config->segment_tan = 1.7320508f;
  config->segment_min_points = 30;
  config->small_min_points = 5;
  config->small_min_rows = 3;
}

int lfx_segment_tables(const lfx_segment_config * config, double * col_cos, double * col_sin, double consts[4])
{
  if (!config || !col_cos || !col_sin || !consts) {return LFX_ERR_INVALID_ARGUMENT;}
  const lfx_segment_config & c = *config;
  const uint32_t H = c.n_rows, W = c.n_columns;
  if (!range_image_ok(H, W, c.min_range, c.max_range)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!std::isfinite(c.row_step) || !(c.row_step > 0.0f)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!(c.ground_first_row <= c.ground_last_row) || !(c.ground_last_row < H)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!std::isfinite(c.ground_tan) || !(c.ground_tan >= 0.0f) || !std::isfinite(c.segment_tan) || !(c.segment_tan > 0.0f)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (c.segment_min_points < 1u || c.small_min_points < 1u || c.small_min_rows < 1u) {return LFX_ERR_INVALID_ARGUMENT;}
  azimuth_table(W, col_cos, col_sin);
  const double col_step = (2.0 * M_PI) / (double)W, row_step = (double)c.row_step;
  consts[0] = std::sin(col_step); consts[1] = std::cos(col_step);
  consts[2] = std::sin(row_step); consts[3] = std::cos(row_step);
  return LFX_OK;
}

// Visibility votes (include/lfx.h, the visibility section): the defaults, and the tables the kernels are given.
void lfx_visibility_default_config(lfx_visibility_config * config)
{
  if (!config) {return;}
  *config = lfx_visibility_config{};
  config->n_rows = 32;
  config->n_columns = 360;
  config->elev_min = -0.43633232f;
  config->elev_step = 0.027270770f;
  config->min_range = 1.0f;
  config->max_range = 100.0f;
  config->radius = 15.0f;
  config->margin_abs = 0.3f;
  config->margin_rel = 0.02f;
  config->guard = 1;
  config->min_through = 2;
  config->agree_weight = 1;
}

int lfx_visibility_tables(const lfx_visibility_config * config, double * col_cos, double * col_sin, double * row_tan)
{
  if (!config || !col_cos || !col_sin || !row_tan) {return LFX_ERR_INVALID_ARGUMENT;}
  const lfx_visibility_config & c = *config;
  const uint32_t H = c.n_rows, W = c.n_columns;
  if (!range_image_ok(H, W, c.min_range, c.max_range)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!std::isfinite(c.elev_min) || !std::isfinite(c.elev_step) || !(c.elev_step > 0.0f)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!((double)c.elev_min > -M_PI / 2.0) || !((double)c.elev_min + (double)H * (double)c.elev_step < M_PI / 2.0)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!std::isfinite(c.radius) || !(c.radius >= 0.0f)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!std::isfinite(c.margin_abs) || !(c.margin_abs >= 0.0f) || !std::isfinite(c.margin_rel) || !(c.margin_rel >= 0.0f)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (c.guard > 2u || c.min_through < 1u || c.reserved != 0u) {return LFX_ERR_INVALID_ARGUMENT;}
  azimuth_table(W, col_cos, col_sin);
  for (uint32_t j = 0; j <= H; j++) {
    row_tan[j] = std::tan((double)c.elev_min + (double)j * (double)c.elev_step);
  }
  return LFX_OK;
}

// Occupancy grids (include/lfx.h, the occupancy section): the defaults, the column tables and the emit's look-up table.
void lfx_occupancy_default_config(lfx_occupancy_config * config)
{
  if (!config) {return;}
  *config = lfx_occupancy_config{};
  config->n_beams = 1800;
  config->min_range = 1.0f;
  config->max_range = 100.0f;
  config->z_min = -1.5f;
  config->z_max = 0.5f;
  config->chunk_scans = 32;
}

int lfx_occupancy_tables(const lfx_occupancy_config * config, double * col_cos, double * col_sin)
{
  if (!config || !col_cos || !col_sin) {return LFX_ERR_INVALID_ARGUMENT;}
  const lfx_occupancy_config & c = *config;
  const uint32_t W = c.n_beams;
  if (W < 4u || W > LFX_OCCUPANCY_MAX_BEAMS || (W & 1u)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (c.max_scans < 1u || c.max_scans > (1u << 24)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (c.width < 1u || c.width > LFX_OCCUPANCY_MAX_SIDE || c.height < 1u || c.height > LFX_OCCUPANCY_MAX_SIDE) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!std::isfinite(c.resolution) || !(c.resolution > 0.0f)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!std::isfinite(c.origin_x) || !std::isfinite(c.origin_y)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!std::isfinite(c.min_range) || !std::isfinite(c.max_range) || !(c.min_range > 0.0f) || !(c.min_range < c.max_range) || !(c.max_range <= 65536.0f)) {
    return LFX_ERR_INVALID_ARGUMENT;
  }
  if (!std::isfinite(c.z_min) || !std::isfinite(c.z_max) || !(c.z_min <= c.z_max)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (c.chunk_scans < 1u || c.chunk_scans > 1024u) {return LFX_ERR_INVALID_ARGUMENT;}
  const double inv_res = 1.0 / (double)c.resolution;
  if (!(std::ceil((double)c.max_range * inv_res) <= 32768.0)) {return LFX_ERR_INVALID_ARGUMENT;}
  azimuth_table(W, col_cos, col_sin);
  return LFX_OK;
}

void lfx_occupancy_emit_default_config(lfx_occupancy_emit_config * config)
{
  if (!config) {return;}
  *config = lfx_occupancy_emit_config{};
  config->w_hit = 85;
  config->w_miss = 40;
  config->l_min = -200;
  config->l_max = 350;
  config->min_observations = 1;
}

int lfx_occupancy_emit_table(const lfx_occupancy_emit_config * config, int8_t * lut)
{
  if (!config || !lut) {return LFX_ERR_INVALID_ARGUMENT;}
  const lfx_occupancy_emit_config & c = *config;
  if (c.w_hit < 1 || c.w_hit > 1000 || c.w_miss < 1 || c.w_miss > 1000) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!(c.l_min < c.l_max) || (int64_t)c.l_max - (int64_t)c.l_min > 4096) {return LFX_ERR_INVALID_ARGUMENT;}
  if (c.min_observations < 1u || c.reserved != 0u) {return LFX_ERR_INVALID_ARGUMENT;}
  const int64_t n = (int64_t)c.l_max - (int64_t)c.l_min + 1;
  for (int64_t j = 0; j < n; j++) {
    const double l = (double)((int64_t)c.l_min + j);
    lut[j] = (int8_t)std::rint(100.0 / (1.0 + std::exp(-l / 100.0)));
  }
  return LFX_OK;
}

}  // extern "C"
