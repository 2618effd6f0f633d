// lfx_kernels_voxel.hpp -- what the kernels that work on voxels share and no kernel of its own (the rolling voxel map,
// lfx_kernels_rolling.hpp; the voxel filter, lfx_kernels_voxelfilter.hpp): the voxel coordinate of a record, the key of a
// voxel, and the count and the scan over a workgroup that both extractions place their output with.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace lfx
{

constexpr int kRollThreads = 256;
constexpr float kRollVoxelLimit = 1048576.f;      // |voxel| < 2^20 per axis: 21 bits of the key

// The voxel coordinate of p along one axis: floorf(p * inv); false where that is not finite or not below 2^20 in size
__host__ __device__ inline bool roll_voxel(float p, float inv, int32_t & v)
{
  const float f = floorf(p * inv);
  if (!(fabsf(f) < kRollVoxelLimit)) {return false;}
  v = (int32_t)f;
  return true;
}

__host__ __device__ inline uint64_t roll_key(int32_t vx, int32_t vy, int32_t vz)
{
  return (1ull << 63) | (uint64_t)((uint32_t)vx & 0x1FFFFFu) | ((uint64_t)((uint32_t)vy & 0x1FFFFFu) << 21) |
         ((uint64_t)((uint32_t)vz & 0x1FFFFFu) << 42);
}

// how many threads of the workgroup say `flag`, into counters[word]: a ballot per wave, one atomic per workgroup
__device__ inline void roll_count(bool flag, uint32_t * sh, unsigned long long * counter)
{
  const uint32_t n = (uint32_t)__popcll(__ballot(flag));
  if ((threadIdx.x & 63) == 0) {sh[threadIdx.x >> 6] = n;}
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < kRollThreads / 64; w++) {t += sh[w];}
    if (t) {atomicAdd(counter, (unsigned long long)t);}
  }
  __syncthreads();
}

// exclusive scan of one value per thread over the workgroup; sh: 2 * (kRollThreads / 64) + 1 words; the total in `total`
__device__ inline uint32_t roll_block_scan(uint32_t v, uint32_t * sh, uint32_t & total)
{
  constexpr int W = kRollThreads / 64;
  const int tid = threadIdx.x;
  uint32_t incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)incl, off, 64);
    if ((tid & 63) >= off) {incl += o;}
  }
  if ((tid & 63) == 63) {sh[tid >> 6] = incl;}
  __syncthreads();
  if (tid == 0) {
    uint32_t run = 0;
    for (int w = 0; w < W; w++) {sh[W + w] = run; run += sh[w];}
    sh[2 * W] = run;
  }
  __syncthreads();
  total = sh[2 * W];
  const uint32_t r = sh[W + (tid >> 6)] + incl - v;
  __syncthreads();
  return r;
}

}  // namespace lfx
