// lfx_kernels_occvalue.hpp -- what every reader of an occupancy grid's counts shares (include/lfx.h, the occupancy section,
// EMIT): a cell's nav_msgs/OccupancyGrid byte from its two counts, and the per-wave sum behind a counter.  The emit kernel
// (lfx_kernels_occupancy.hpp) and the distance field's classes (lfx_kernels_distance.hpp) both go through occ_value.
#pragma once

#include "lfx_kernels_common.hpp"

namespace lfx
{

// the sum of v over the workgroup's lanes added to *counter: a shuffle tree per wave, one atomic per wave that has any
__device__ inline void occ_count(unsigned long long * counter, uint32_t v)
{
  for (int d = 32; d; d >>= 1) {v += __shfl_down(v, d);}
  if ((threadIdx.x & 63u) == 0u && v) {atomicAdd(counter, (unsigned long long)v);}
}

struct OccEmitArgs
{
  const uint32_t * hits, * misses;
  uint64_t cells;
  int64_t w_hit, w_miss, l_min, l_max;
  uint32_t min_observations;
  const int8_t * lut;                   // [l_max - l_min + 1]: lfx_occupancy_emit_table's bytes
  int8_t * out;                         // device memory or a pinned block
  bool words;                           // out is 4-byte aligned: four cells leave as one word
};

__device__ inline int8_t occ_value(const OccEmitArgs & A, uint64_t cell)
{
  const uint32_t h = A.hits[cell], m = A.misses[cell];
  if ((uint64_t)h + (uint64_t)m < (uint64_t)A.min_observations) {return (int8_t)-1;}
  int64_t l = (int64_t)h * A.w_hit - (int64_t)m * A.w_miss;
  l = l < A.l_min ? A.l_min : (l > A.l_max ? A.l_max : l);
  return A.lut[l - A.l_min];
}

}  // namespace lfx
