// lfx_kernels_mapping.hpp -- the device side of the keyframe mapper (lfx_mapping.hip): every added cloud of one call
// transformed behind the map in one launch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "lfx_kernels_transform.hpp"

namespace lfx
{

constexpr int kMapAppendThreads = 256;

// One added cloud of a call: `count` records from record `src` of the caller's points, transformed by `m`, to record `dst`
// of the map; its workgroups are [first_block, first_block + ceil(count / kMapAppendThreads)).  128 bytes.
struct MapAppendEntry
{
  double m[12];                           // the cloud's pose, [R | t] row-major
  uint64_t dst;
  uint32_t src, count, first_block, pad[3];
};
static_assert(sizeof(MapAppendEntry) == 128 && alignof(MapAppendEntry) <= 64, "MapAppendEntry is 128 bytes, placed on 64-byte boundaries");

// Map::TransformAdd (map.hpp:68-74) for every added cloud of a call.  Workgroups map to (cloud, chunk of kMapAppendThreads
// records) through the table: the entry is the last one whose first_block <= blockIdx.x (a binary search, uniform over
// the workgroup).  One 16-byte load and one 16-byte store per record; no LDS.
__global__ __launch_bounds__(kMapAppendThreads) void map_append_kernel(
  const MapAppendEntry * __restrict__ table, uint32_t n_entries, const float4 * __restrict__ src, float4 * __restrict__ dst)
{
  const uint32_t b = blockIdx.x;
  uint32_t lo = 0u, hi = n_entries;         // table[lo].first_block <= b < table[hi].first_block
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (table[mid].first_block <= b) {lo = mid;} else {hi = mid;}
  }
  const MapAppendEntry * e = table + lo;
  const uint32_t i = (b - e->first_block) * kMapAppendThreads + threadIdx.x;
  if (i < e->count) {
    dst[e->dst + i] = pcl_transform_record(e->m, src[(size_t)e->src + i]);
  }
}

}  // namespace lfx
