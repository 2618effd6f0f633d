// lfx_kernels_image.hpp -- what the kernels that bin records by azimuth share (the scan-context descriptor, the
// segmentation's range image, the visibility images): the one read of a record's coordinates, the gates in front of a
// projection, and the column of a direction over a table cos / sin of -pi + 2 pi m / W (lfx_pose.cpp, azimuth_table).  The
// arithmetic is include/lfx.h's, in double, unfused: the pragma below holds for the code here whatever includes it.
#pragma once

#include "lfx_kernels_common.hpp"

#pragma clang fp contract(off)

namespace lfx
{

// x, y, z of one input record.  XYZ16: the record is a canonical one (x, y, z little-endian in the first 12 bytes of a
// 16-byte aligned 32-byte record -- the host's canonical_xyz16, lfx_internal.hpp), read with one 16-byte load.
template<bool XYZ16>
__device__ inline void load_xyz(const uint8_t * rec, const Layout & L, float & x, float & y, float & z)
{
  if (XYZ16) {
    const float4 v = *reinterpret_cast<const float4 *>(rec);
    x = v.x; y = v.y; z = v.z;
  } else {
    x = load_f32(rec + L.ox, L.be); y = load_f32(rec + L.oy, L.be); z = load_f32(rec + L.oz, L.be);
  }
}

// The gates every range image puts in front of its projection: a point with a non-finite coordinate or on the sensor's
// axis (xy2 = x^2 + y^2 == 0: no direction) has no cell.  Else xy2 and r = sqrt(xy2 + z^2); the comparison of r with a
// range, and the row, are the caller's.
__device__ inline bool planar_range(double x, double y, double z, double & xy2, double & r)
{
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) {return false;}
  xy2 = x * x + y * y;
  if (xy2 == 0.0) {return false;}
  r = sqrt(xy2 + z * z);
  return true;
}

// The column of direction (xd, yd) among W (even, >= 4): the half of the circle it lies in (upper: y >= 0, which -0.0 is --
// columns [W / 2, W)), then the last direction m of that half whose cross product cs[m] * yd - sn[m] * xd is >= 0 -- two
// rounded products and one subtraction.  The half's first direction is never asked: it is the answer where no later one
// passes, so the seam needs no case of its own.
__device__ inline uint32_t azimuth_column(const double * cs, const double * sn, uint32_t W, double xd, double yd, bool upper)
{
  const uint32_t m0 = upper ? W / 2u : 0u;
  uint32_t lo = 0, hi = W / 2u - 1u;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    const double cross = cs[m0 + mid] * yd - sn[m0 + mid] * xd;
    if (cross >= 0.0) {lo = mid;} else {hi = mid - 1u;}
  }
  return m0 + lo;
}

}  // namespace lfx
