// lfx_kernels_transform.hpp -- the one record transform the odometry's store and the mapper's map are written with.
#pragma once

#include <hip/hip_runtime.h>

namespace lfx
{

// pcl::transformPointCloud with an Affine3d (PCL's generic Transformer<double>) for one record: every coordinate
// ((r0 * x + r1 * y) + r2 * z) + t in double, rounded once to float (the units are compiled with -ffp-contract=off: no fused
// multiply-add), the record's 4th float copied.  m: [R | t] row-major.  odometry_append_kernel and map_append_kernel
// (lfx_kernels_mapping.hpp) both call it, so the odometry's store and the mapper's map hold the same bits.
__device__ inline float4 pcl_transform_record(const double * m, const float4 p)
{
  const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
  float4 q;
  q.x = (float)(((m[0] * x + m[1] * y) + m[2] * z) + m[3]);
  q.y = (float)(((m[4] * x + m[5] * y) + m[6] * z) + m[7]);
  q.z = (float)(((m[8] * x + m[9] * y) + m[10] * z) + m[11]);
  q.w = p.w;
  return q;
}

}  // namespace lfx
