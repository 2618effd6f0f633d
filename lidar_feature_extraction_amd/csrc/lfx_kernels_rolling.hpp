// lfx_kernels_rolling.hpp -- the device side of the rolling voxel map (lfx_rolling.hip): a direct-mapped, tagged voxel
// array per kind of cloud.  Slot of voxel v: (v mod N) per axis; the slot's key says which voxel it holds, so moving the
// window touches nothing on the device (include/lfx.h has the contract).  No probing, no spin, no grid-wide barrier:
// an insert is two launches (claim, commit), an extraction three (count, scan of the counts, write).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "lfx_kernels_transform.hpp"
#include "lfx_kernels_voxel.hpp"

namespace lfx
{

constexpr int kRollCells = 4 * kRollThreads;      // cells of a box one workgroup of the extraction looks at

// One store as the kernels see it.  o: the window's first voxel per axis; n: its size in voxels.
struct RollStore
{
  uint64_t * keys, * stamps;
  float4 * points;
  int32_t o[3];
  uint32_t n[3];
  float inv;                                      // 1.0f / leaf
};

// v mod n, the non-negative one
__host__ __device__ inline uint32_t roll_mod(int32_t v, uint32_t n)
{
  const int64_t r = (int64_t)v % (int64_t)n;
  return (uint32_t)(r < 0 ? r + (int64_t)n : r);
}

__host__ __device__ inline uint32_t roll_slot(const RollStore & s, int32_t vx, int32_t vy, int32_t vz)
{
  return (roll_mod(vz, s.n[2]) * s.n[1] + roll_mod(vy, s.n[1])) * s.n[0] + roll_mod(vx, s.n[0]);
}

// One cloud of an insert: `count` records from record `src` of the caller's points, transformed by `m`; its workgroups are
// [first_block, first_block + ceil(count / kRollThreads)); rank: the rank of its first record, (cloud, index in cloud)
// counted through the call.  128 bytes.
struct RollInsertEntry
{
  double m[12];
  uint32_t src, count, first_block, rank, pad[4];
};
static_assert(sizeof(RollInsertEntry) == 128, "RollInsertEntry is 128 bytes");

enum : int {kRollNone = -1, kRollInside = 0, kRollOutside = 1, kRollNonFinite = 2};
// words of a store's counters (uint64 each): records committed, records that fell inside the window (a live voxel's and a
// call's losers among them), outside it, dropped as not finite
enum : int {kRollInserted = 0, kRollInsideCount = 1, kRollOutsideCount = 2, kRollNonFiniteCount = 3, kRollCounters = 4};

// The record of this thread (workgroups map to clouds as map_append_kernel's do), transformed, and where it falls
__device__ inline int roll_locate(const RollStore & s, const RollInsertEntry * __restrict__ table, uint32_t n_entries,
  const float4 * __restrict__ src, float4 & q, uint32_t & slot, uint64_t & key, uint32_t & rank)
{
  const uint32_t b = blockIdx.x;
  uint32_t lo = 0u, hi = n_entries;         // table[lo].first_block <= b < table[hi].first_block
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (table[mid].first_block <= b) {lo = mid;} else {hi = mid;}
  }
  const RollInsertEntry * e = table + lo;
  const uint32_t i = (b - e->first_block) * kRollThreads + threadIdx.x;
  if (i >= e->count) {return kRollNone;}
  rank = e->rank + i;
  q = pcl_transform_record(e->m, src[(size_t)e->src + i]);
  int32_t vx, vy, vz;
  if (!roll_voxel(q.x, s.inv, vx) || !roll_voxel(q.y, s.inv, vy) || !roll_voxel(q.z, s.inv, vz)) {return kRollNonFinite;}
  const int64_t dx = (int64_t)vx - s.o[0], dy = (int64_t)vy - s.o[1], dz = (int64_t)vz - s.o[2];
  if (dx < 0 || dx >= (int64_t)s.n[0] || dy < 0 || dy >= (int64_t)s.n[1] || dz < 0 || dz >= (int64_t)s.n[2]) {return kRollOutside;}
  slot = roll_slot(s, vx, vy, vz);
  key = roll_key(vx, vy, vz);
  return kRollInside;
}

__device__ inline uint64_t roll_stamp(uint32_t epoch, uint32_t rank) {return ((uint64_t)epoch << 32) | (uint64_t)(0xFFFFFFFFu - rank);}

// Insert, first launch: every record that falls in a voxel of the window that is not live bids for the voxel's slot with
// (epoch, lowest rank wins).  The epoch is the store's count of insert calls: a bid of this call beats every older stamp,
// so the stamps are never cleared.  Inside the window voxel -> slot is injective: only records of one voxel meet in a slot.
__global__ __launch_bounds__(kRollThreads) void rolling_claim_kernel(
  RollStore s, const RollInsertEntry * __restrict__ table, uint32_t n_entries, const float4 * __restrict__ src, uint32_t epoch,
  unsigned long long * __restrict__ counters)
{
  __shared__ uint32_t sh[kRollThreads / 64];
  float4 q;
  uint32_t slot = 0u, rank = 0u;
  uint64_t key = 0u;
  const int what = roll_locate(s, table, n_entries, src, q, slot, key, rank);
  if (what == kRollInside && s.keys[slot] != key) {
    atomicMax(reinterpret_cast<unsigned long long *>(s.stamps + slot), (unsigned long long)roll_stamp(epoch, rank));
  }
  roll_count(what == kRollInside, sh, counters + kRollInsideCount);
  roll_count(what == kRollOutside, sh, counters + kRollOutsideCount);
  roll_count(what == kRollNonFinite, sh, counters + kRollNonFiniteCount);
}

// Insert, second launch (behind the first in stream order): the record whose bid stands writes point and key.  A record of
// a live voxel made no bid and its stamp carries this call's epoch, which no older stamp does: it writes nothing.
__global__ __launch_bounds__(kRollThreads) void rolling_commit_kernel(
  RollStore s, const RollInsertEntry * __restrict__ table, uint32_t n_entries, const float4 * __restrict__ src, uint32_t epoch,
  unsigned long long * __restrict__ counters)
{
  __shared__ uint32_t sh[kRollThreads / 64];
  float4 q;
  uint32_t slot = 0u, rank = 0u;
  uint64_t key = 0u;
  const int what = roll_locate(s, table, n_entries, src, q, slot, key, rank);
  const bool won = what == kRollInside && s.stamps[slot] == roll_stamp(epoch, rank);
  if (won) {
    s.points[slot] = q;
    s.keys[slot] = key;
  }
  roll_count(won, sh, counters + kRollInserted);
}

// A box of voxels inside the window: cell i is voxel lo + (i % b[0], (i / b[0]) % b[1], i / (b[0] * b[1])), x fastest.
struct RollBox
{
  int32_t lo[3];
  uint32_t b[3];
  uint32_t cells;                                 // <= 2^31: the box lies inside the window
};

// whether cell i of the box is live, and its slot (consecutive cells of a row are consecutive slots but for the wrap)
__device__ inline bool roll_live(const RollStore & s, const RollBox & box, uint32_t i, uint32_t & slot)
{
  const uint32_t x = i % box.b[0], t = i / box.b[0], y = t % box.b[1], z = t / box.b[1];
  const int32_t vx = box.lo[0] + (int32_t)x, vy = box.lo[1] + (int32_t)y, vz = box.lo[2] + (int32_t)z;
  slot = roll_slot(s, vx, vy, vz);
  return s.keys[slot] == roll_key(vx, vy, vz);
}

// Extraction, first launch: live cells per workgroup (kRollCells cells, 4 consecutive ones per thread)
__global__ __launch_bounds__(kRollThreads) void rolling_block_count_kernel(RollStore s, RollBox box, uint32_t * __restrict__ partial)
{
  __shared__ uint32_t sh[2 * (kRollThreads / 64) + 1];
  const uint32_t base = blockIdx.x * (uint32_t)kRollCells + 4u * threadIdx.x;
  uint32_t v = 0, slot;
#pragma unroll
  for (uint32_t a = 0; a < 4u; a++) {
    if (base + a < box.cells && roll_live(s, box, base + a, slot)) {v++;}
  }
  uint32_t total;
  (void)roll_block_scan(v, sh, total);
  if (threadIdx.x == 0) {partial[blockIdx.x] = total;}
}

// Extraction, second launch (one workgroup): the workgroups' counts to their exclusive prefix sums; the sum to *total
__global__ __launch_bounds__(kRollThreads) void rolling_partial_scan_kernel(uint32_t * __restrict__ partial, uint32_t n_blocks, uint64_t * __restrict__ total_out)
{
  __shared__ uint32_t sh[2 * (kRollThreads / 64) + 1];
  const uint32_t per = (n_blocks + kRollThreads - 1) / kRollThreads;
  const uint32_t a = min(threadIdx.x * per, n_blocks), b = min(a + per, n_blocks);
  uint32_t v = 0;
  for (uint32_t i = a; i < b; i++) {v += partial[i];}
  uint32_t total;
  uint32_t run = roll_block_scan(v, sh, total);
  for (uint32_t i = a; i < b; i++) {const uint32_t c = partial[i]; partial[i] = run; run += c;}
  if (threadIdx.x == 0) {*total_out = total;}
}

// Extraction, third launch: the live cells' points in the order of the cells; nothing at or past `capacity`
__global__ __launch_bounds__(kRollThreads) void rolling_write_kernel(
  RollStore s, RollBox box, const uint32_t * __restrict__ partial, float4 * __restrict__ out, uint64_t capacity)
{
  __shared__ uint32_t sh[2 * (kRollThreads / 64) + 1];
  const uint32_t base = blockIdx.x * (uint32_t)kRollCells + 4u * threadIdx.x;
  uint32_t slot[4];
  bool live[4];
  uint32_t v = 0;
#pragma unroll
  for (uint32_t a = 0; a < 4u; a++) {
    live[a] = base + a < box.cells && roll_live(s, box, base + a, slot[a]);
    v += live[a] ? 1u : 0u;
  }
  uint32_t total;
  uint64_t at = (uint64_t)partial[blockIdx.x] + roll_block_scan(v, sh, total);
#pragma unroll
  for (uint32_t a = 0; a < 4u; a++) {
    if (live[a]) {
      if (at < capacity) {out[at] = s.points[slot[a]];}
      at++;
    }
  }
}

}  // namespace lfx
