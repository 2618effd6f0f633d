// lfx_deskew_rows.hpp -- the rows of doubles the de-skew kernels read (lfx_kernels_deskew.hpp), as the host writes them:
// one per scan for a constant motion (lfx_deskew.hip), one per segment along a trajectory (lfx_trajectory_segments,
// lfx_pose.cpp).  No HIP header: the host-only file includes it too.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace lfx
{

enum
{
  // the twist both kinds of row begin with
  kRowK = 0,        // k = w / theta (0 where theta < 1e-8)
  kRowTheta = 3,
  kRowW = 4,        // w: the small-angle form reads it
  // a scan's row, constant motion
  kDskV = 7,        // v = t_D
  kDskR = 10,       // R_D, row-major 3 x 3
  kDskT0 = 19,
  kDskInvDt = 20,   // 1 / (t1 - t0)
  kDskScale = 21,   // seconds per unit of the time field
  kDskStride = 24,
  // a segment's row
  kTrjA = 7,        // the rotation of Q_j, row-major 3 x 3
  kTrjQ = 16,       // its translation
  kTrjDq = 19,      // q_{j+1} - q_j
  kTrjTime = 22,    // times[j]
  kTrjInvDt = 23,   // 1 / (times[j+1] - times[j])
  kTrjStride = 24
};

inline void write_twist(double * T, const double w[3], double theta)
{
  for (int a = 0; a < 3; a++) {
    T[kRowK + a] = theta < 1e-8 ? 0.0 : w[a] / theta;
    T[kRowW + a] = w[a];
  }
  T[kRowTheta] = theta;
}

// what is asked of the numbers a caller hands in
inline bool finite_run(const double * v, size_t n)
{
  for (size_t i = 0; i < n; i++) {
    if (!std::isfinite(v[i])) {return false;}
  }
  return true;
}

inline bool ascending_times(const double * t, uint32_t n)
{
  if (!finite_run(t, n)) {return false;}
  for (uint32_t i = 1; i < n; i++) {
    if (!(t[i] > t[i - 1])) {return false;}
  }
  return true;
}

}  // namespace lfx
