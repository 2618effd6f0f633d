// lfx_kernels_kfrange.hpp -- how the kernels that walk a keyframe store's records address them, and no kernel of its own (the
// store's, lfx_kernels_keyframes.hpp; the voxel filter's add from the store, lfx_kernels_voxelfilter.hpp): the shape of a
// launch, the range it works on and the search for a record's keyframe.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace lfx
{

constexpr int kKfThreads = 256;
constexpr int kKfPerLane = 4;                                    // whole 16-byte records per lane
constexpr uint32_t kKfRun = kKfThreads * kKfPerLane;             // source records per workgroup of the transform: 1024
constexpr uint32_t kKfWave = 64;
constexpr uint64_t kKfNone = ~0ull;                              // out_begin of a keyframe that is not written
constexpr uint32_t kKfNoId = 0xFFFFFFFFu;

// What a transform launch works on: the source records [rec_lo, rec_hi) of one kind, which lie in the keyframes
// [k_lo, k_hi): begin[k_lo] <= rec_lo and rec_hi <= begin[k_hi].
struct KfRange
{
  uint64_t rec_lo, rec_hi;
  uint32_t k_lo, k_hi, first, pad;          // first: out_begin is indexed k - first (selected form)
};

// the keyframe that holds record `run` of [begin[k_lo], begin[k_hi]): the last that begins at or before it (it is not empty)
__device__ inline uint32_t kf_keyframe_of(const uint64_t * __restrict__ begin, uint32_t k_lo, uint32_t k_hi, uint64_t run)
{
  uint32_t lo = k_lo, hi = k_hi;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (begin[mid] <= run) {lo = mid;} else {hi = mid;}
  }
  return lo;
}

}  // namespace lfx
