// lfx_kernels_odometry.hpp -- the device side of the odometry's store (lfx_odometry.hip): a scan's two clouds transformed
// into the store, their bounds on the way.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "lfx_kernels_common.hpp"
#include "lfx_kernels_transform.hpp"

namespace lfx
{

struct OdoPose
{
  double m[12];                           // point_to_map, [R | t] row-major
};

constexpr int kAppendThreads = 256;

// RecentScans::Add (recent_scans.hpp:67-73) for both clouds of one scan in one launch: pcl_transform_record.  Workgroups
// [0, edge_blocks) take the edge cloud, the rest the surface cloud.  bounds [2][6] (edge, surface), zeroed before the launch:
// words 0-2 the complement of the least x, y, z and words 3-5 the greatest, both by atomicMax over float_order -- all
// zero = no point.
__global__ __launch_bounds__(kAppendThreads) void odometry_append_kernel(
  OdoPose P, const float4 * __restrict__ edge_src, uint32_t n_edge, const float4 * __restrict__ surface_src, uint32_t n_surface,
  float4 * __restrict__ edge_dst, float4 * __restrict__ surface_dst, uint32_t edge_blocks, uint32_t * __restrict__ bounds)
{
  const bool surf = blockIdx.x >= edge_blocks;       // (uniform over the workgroup)
  const uint32_t i = (surf ? blockIdx.x - edge_blocks : blockIdx.x) * kAppendThreads + threadIdx.x;
  const uint32_t n = surf ? n_surface : n_edge;
  uint32_t v[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  if (i < n) {
    const float4 p = (surf ? surface_src : edge_src)[i];
    const float4 q = pcl_transform_record(P.m, p);
    (surf ? surface_dst : edge_dst)[i] = q;
    v[0] = ~float_order(q.x); v[1] = ~float_order(q.y); v[2] = ~float_order(q.z);
    v[3] = float_order(q.x); v[4] = float_order(q.y); v[5] = float_order(q.z);
  }
#pragma unroll
  for (int a = 0; a < 6; a++) {
    for (int off = 32; off >= 1; off >>= 1) {v[a] = max(v[a], (uint32_t)__shfl_xor((int)v[a], off, 64));}
  }
  if ((threadIdx.x & 63) == 0 && v[3] != 0u) {       // (a wave with a point has a non-zero greatest-x word)
    uint32_t * b = bounds + (surf ? 6 : 0);
#pragma unroll
    for (int a = 0; a < 6; a++) {atomicMax(&b[a], v[a]);}
  }
}

}  // namespace lfx
