// lfx_kernels_voxelfilter.hpp -- the device side of the voxel filter (lfx_voxelfilter.hip; include/lfx.h has the model): an
// open-addressing hash table of voxels on a grid anchored at the world origin.  A voxel's entry is one 64-byte line: key,
// least rank, count and three integer sums, all written with 64-bit integer atomics and nothing else, so what a table holds
// does not depend on the order its records arrived in -- only which entry a voxel took does, and nothing reads that.  An
// insert never waits on another thread: a compare-and-swap on the key, at most `slots` probes, then the record is counted as
// lost.  An add merges before it goes to memory, twice: equal neighbours among a wave's 64 records, then everything a
// workgroup's 1 024 records hold of one voxel in a table in LDS -- integer sums, so the global table ends up with the same
// words.  An emit is three passes over entries and rank bitmap (mark, scan, write) with no sort and no pass over the input.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "lfx_kernels_kfrange.hpp"
#include "lfx_kernels_transform.hpp"
#include "lfx_kernels_voxel.hpp"

#ifndef LFX_VF_MERGE
#define LFX_VF_MERGE 1                              // 0: every record does its own atomics (the A/B build of DESIGN.md section 7)
#endif

#ifndef LFX_VF_BLOCK
#define LFX_VF_BLOCK 1                              // 0: runs go to the global table directly, no table of the workgroup's own (A/B)
#endif

namespace lfx
{

constexpr int kVfThreads = 256;
constexpr uint32_t kVfWave = 64;
constexpr uint32_t kVfPerLane = 4;
constexpr uint32_t kVfRun = kVfThreads * kVfPerLane;              // records per workgroup of an add: 1024
constexpr uint32_t kVfTileWords = kVfThreads * 4u;                // words of the rank bitmap per workgroup of the scan: 1024
constexpr uint32_t kVfScanTile = 32u * kVfTileWords;              // ... which is 32 768 ranks
constexpr uint64_t kVfNoRank = ~0ull;
constexpr double kVfScale = 16777216.0;                           // 2^24: the fixed point of a record's place inside its voxel
static_assert(kVfRun == kKfRun && kVfThreads == kKfThreads, "an add walks the store as the keyframe transform does");
static_assert(kVfThreads == kRollThreads, "roll_count and roll_block_scan are written for the rolling map's workgroup");

// One voxel.  key: roll_key of the voxel, 0 = empty (roll_key has bit 63 set).  rank: the least rank that reached it.
// s[a]: the sum of q over its records, two's complement.
struct VfEntry
{
  uint64_t key, rank, count;
  int64_t s[3];
  uint64_t pad[2];
};
static_assert(sizeof(VfEntry) == 64, "a voxel is one 64-byte line");

// words of a filter's counters (uint64 each): records with a voxel (accumulated + lost), not finite, out of range, lost to
// a full table; then what an emit counts: occupied entries, voxels written
enum : int {kVfValid = 0, kVfNonFinite = 1, kVfOutOfRange = 2, kVfTableFull = 3, kVfVoxels = 4, kVfWritten = 5, kVfCounters = 8};

// where a voxel's probe starts: the top log2_slots bits of key * 2^64 / phi (tests/voxel_filter_restatement.py states it too)
__host__ __device__ inline uint64_t vf_home(uint64_t key, uint32_t log2_slots) {return (key * 0x9E3779B97F4A7C15ull) >> (64u - log2_slots);}

// one axis of the voxel a key names: 21 bits, sign-extended
__device__ inline int32_t vf_unkey(uint64_t key, int axis) {return ((int32_t)((uint32_t)(key >> (21 * axis)) << 11)) >> 11;}

// q of the model: the record's place inside voxel v along one axis, in units of 2^-24 leaf.  Separate double operations
// (the units are compiled with -ffp-contract=off); rint rounds to nearest even.
__device__ inline int64_t vf_q(float p, float inv, int32_t v) {return (int64_t)rint((((double)p * (double)inv) - (double)v) * kVfScale);}

// What a wave has seen of its records, uniform over the wave (valid, not finite, out of range), and its one trip to the
// counters at the end of the kernel.
struct VfTally
{
  uint32_t n[3] = {0u, 0u, 0u};
};
__device__ inline void vf_flush(const VfTally & t, unsigned long long * __restrict__ counters)
{
  if ((threadIdx.x & (kVfWave - 1u)) != 0u) {return;}
  if (t.n[0]) {atomicAdd(counters + kVfValid, (unsigned long long)t.n[0]);}
  if (t.n[1]) {atomicAdd(counters + kVfNonFinite, (unsigned long long)t.n[1]);}
  if (t.n[2]) {atomicAdd(counters + kVfOutOfRange, (unsigned long long)t.n[2]);}
}

// n records of one voxel into the table: the probe is bounded by the slots, nobody is waited for.
__device__ inline void vf_insert(VfEntry * __restrict__ table, uint32_t log2_slots, unsigned long long * __restrict__ counters, uint64_t key,
  uint64_t rank, uint32_t n, int64_t sx, int64_t sy, int64_t sz)
{
  const uint64_t slots = 1ull << log2_slots, mask = slots - 1u;
  uint64_t at = vf_home(key, log2_slots);
  for (uint64_t probe = 0; probe < slots; probe++, at = (at + 1u) & mask) {
    VfEntry * e = table + at;
    unsigned long long * k = reinterpret_cast<unsigned long long *>(&e->key);
    unsigned long long seen = __hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (seen == 0ull) {seen = atomicCAS(k, 0ull, (unsigned long long)key); if (seen == 0ull) {seen = key;}}
    if (seen == key) {
      // (the least rank only falls: where the value read, stale or not, is already at or below this one, the minimum stands)
      unsigned long long * r = reinterpret_cast<unsigned long long *>(&e->rank);
      if (__hip_atomic_load(r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (unsigned long long)rank) {atomicMin(r, (unsigned long long)rank);}
      atomicAdd(reinterpret_cast<unsigned long long *>(&e->count), (unsigned long long)n);
      atomicAdd(reinterpret_cast<unsigned long long *>(&e->s[0]), (unsigned long long)sx);
      atomicAdd(reinterpret_cast<unsigned long long *>(&e->s[1]), (unsigned long long)sy);
      atomicAdd(reinterpret_cast<unsigned long long *>(&e->s[2]), (unsigned long long)sz);
      return;
    }
  }
  atomicAdd(counters + kVfTableFull, (unsigned long long)n);
}

// --- the workgroup's own table (LFX_VF_BLOCK) -----------------------------------------------------------------------------
// kVfLdsSlots voxels in LDS, laid out by field; the same insert as the global table's with a probe of kVfLdsProbes entries,
// after which the run goes to the global table directly.  Behind a barrier every occupied entry is flushed as one run.
// Integer adds and minima in both tables: the global table ends up with the same words.
constexpr uint32_t kVfLdsLog2 = 10u, kVfLdsSlots = 1u << kVfLdsLog2, kVfLdsProbes = 8u;
struct VfLds
{
  unsigned long long key[kVfLdsSlots], rank[kVfLdsSlots], s[3][kVfLdsSlots];
  uint32_t count[kVfLdsSlots];
};

__device__ inline void vf_lds_clear(VfLds & t)
{
  for (uint32_t i = threadIdx.x; i < kVfLdsSlots; i += kVfThreads) {
    t.key[i] = 0ull; t.rank[i] = kVfNoRank; t.s[0][i] = 0ull; t.s[1][i] = 0ull; t.s[2][i] = 0ull; t.count[i] = 0u;
  }
  __syncthreads();
}

__device__ inline void vf_lds_insert(VfLds & t, VfEntry * __restrict__ table, uint32_t log2_slots, unsigned long long * __restrict__ counters,
  uint64_t key, uint64_t rank, uint32_t n, int64_t sx, int64_t sy, int64_t sz)
{
  uint32_t at = (uint32_t)vf_home(key, kVfLdsLog2);
  for (uint32_t probe = 0; probe < kVfLdsProbes; probe++, at = (at + 1u) & (kVfLdsSlots - 1u)) {
    unsigned long long seen = t.key[at];
    if (seen == 0ull) {seen = atomicCAS(&t.key[at], 0ull, (unsigned long long)key); if (seen == 0ull) {seen = key;}}
    if (seen == key) {
      atomicMin(&t.rank[at], (unsigned long long)rank);
      atomicAdd(&t.count[at], n);
      atomicAdd(&t.s[0][at], (unsigned long long)sx);
      atomicAdd(&t.s[1][at], (unsigned long long)sy);
      atomicAdd(&t.s[2][at], (unsigned long long)sz);
      return;
    }
  }
  vf_insert(table, log2_slots, counters, key, rank, n, sx, sy, sz);
}

__device__ inline void vf_lds_flush(VfLds & t, VfEntry * __restrict__ table, uint32_t log2_slots, unsigned long long * __restrict__ counters)
{
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < kVfLdsSlots; i += kVfThreads) {
    const uint64_t key = t.key[i];
    if (key != 0ull) {vf_insert(table, log2_slots, counters, key, t.rank[i], t.count[i], (int64_t)t.s[0][i], (int64_t)t.s[1][i], (int64_t)t.s[2][i]);}
  }
}

// One record per lane of a whole wave (every lane calls, `live` says whether it has a record; lane order is rank order).
// Merged form: lanes that follow each other with the same voxel form a run; the sums of a run are added up over the lanes
// by a segmented scan of shuffles -- integers, so exactly what the single adds would give -- and the run's last lane alone
// goes on, with the rank of the run's first: to the workgroup's table where there is one (`block`), else to the global one.
__device__ inline void vf_accumulate(VfEntry * __restrict__ table, uint32_t log2_slots, float inv, unsigned long long * __restrict__ counters,
  const float4 p, uint64_t rank, bool live, VfTally & tally, VfLds * block)
{
  const bool finite = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
  int32_t vx = 0, vy = 0, vz = 0;
  const bool valid = live && finite && roll_voxel(p.x, inv, vx) && roll_voxel(p.y, inv, vy) && roll_voxel(p.z, inv, vz);
  tally.n[0] += (uint32_t)__popcll(__ballot(valid));
  tally.n[1] += (uint32_t)__popcll(__ballot(live && !finite));
  tally.n[2] += (uint32_t)__popcll(__ballot(live && finite && !valid));
  const uint64_t key = valid ? roll_key(vx, vy, vz) : 0ull;
  int64_t sx = 0, sy = 0, sz = 0;
  if (valid) {sx = vf_q(p.x, inv, vx); sy = vf_q(p.y, inv, vy); sz = vf_q(p.z, inv, vz);}
  uint64_t first_rank = rank;
  uint32_t n = 1u;
  bool insert = valid;
#if LFX_VF_MERGE
  const uint32_t lane = threadIdx.x & (kVfWave - 1u);
  const uint64_t before = (uint64_t)__shfl_up((long long)key, 1, kVfWave);
  const uint64_t heads = __ballot(lane == 0u || before != key);                   // bit l: a run starts at lane l
  const uint32_t start = 63u - (uint32_t)__clzll(heads & (~0ull >> (63u - lane)));  // the start of this lane's run (bit 0 is set)
#pragma unroll
  for (uint32_t d = 1u; d < kVfWave; d <<= 1) {
    const int64_t ox = __shfl_up((long long)sx, d, kVfWave), oy = __shfl_up((long long)sy, d, kVfWave), oz = __shfl_up((long long)sz, d, kVfWave);
    if (lane >= start + d) {sx += ox; sy += oy; sz += oz;}
  }
  first_rank = (uint64_t)__shfl((long long)rank, (int)start, kVfWave);
  n = lane - start + 1u;
  insert = valid && (lane == kVfWave - 1u || ((heads >> (lane + 1u)) & 1ull));      // the run's last lane
#endif
  if (insert) {
    if (block) {
      vf_lds_insert(*block, table, log2_slots, counters, key, first_rank, n, sx, sy, sz);
    } else {
      vf_insert(table, log2_slots, counters, key, first_rank, n, sx, sy, sz);
    }
  }
}

// every entry empty
__global__ __launch_bounds__(kVfThreads) void voxel_filter_clear_kernel(VfEntry * __restrict__ table, uint64_t slots)
{
  const uint64_t i = (uint64_t)blockIdx.x * kVfThreads + threadIdx.x;
  if (i >= slots) {return;}
  VfEntry e{};
  e.rank = kVfNoRank;
  table[i] = e;
}

// n records from `src`, ranks rank0 ..: workgroup b has the kVfRun records from b kVfRun, lane t of it the records t, t + 256,
// t + 512, t + 768 of them, so a wave has 64 consecutive records in each of its four steps.
__global__ __launch_bounds__(kVfThreads) void voxel_filter_add_kernel(
  VfEntry * __restrict__ table, uint32_t log2_slots, float inv, unsigned long long * __restrict__ counters, const float4 * __restrict__ src, uint64_t n,
  uint64_t rank0)
{
  const uint64_t run = (uint64_t)blockIdx.x * kVfRun;
  float4 p[kVfPerLane];
#pragma unroll
  for (uint32_t j = 0; j < kVfPerLane; j++) {
    const uint64_t i = run + j * kVfThreads + threadIdx.x;
    p[j] = i < n ? src[i] : float4{0.f, 0.f, 0.f, 0.f};
  }
#if LFX_VF_BLOCK
  __shared__ VfLds lds;
  VfLds * block = &lds;
  vf_lds_clear(lds);
#else
  VfLds * block = nullptr;
#endif
  VfTally tally;
#pragma unroll
  for (uint32_t j = 0; j < kVfPerLane; j++) {
    const uint64_t i = run + j * kVfThreads + threadIdx.x;
    vf_accumulate(table, log2_slots, inv, counters, p[j], rank0 + i, i < n, tally, block);
  }
  vf_flush(tally, counters);
#if LFX_VF_BLOCK
  vf_lds_flush(lds, table, log2_slots, counters);
#endif
}

// The keyframe store's sensor-frame records [a.rec_lo, a.rec_hi) of one kind straight into the table: each is loaded once,
// transformed with the pose of its keyframe as keyframes_transform_kernel transforms it (the same walk over `begin`: the
// wave's keyframe through the scalar path where a step's 64 records lie in one keyframe, a search per lane otherwise) and
// accumulated; no world record is written.  Record i has rank rank0 + (i - rec_lo), flagged or not; with `flags` a record
// whose byte is non-zero is left out.
__global__ __launch_bounds__(kVfThreads) void voxel_filter_add_keyframes_kernel(
  VfEntry * __restrict__ table, uint32_t log2_slots, float inv, unsigned long long * __restrict__ counters, const float4 * __restrict__ src,
  const uint64_t * __restrict__ begin, const double * __restrict__ poses, const uint8_t * __restrict__ flags, uint64_t rank0, const KfRange a)
{
  const uint64_t run = a.rec_lo + (uint64_t)blockIdx.x * kVfRun;
  const uint64_t run_end = run + kVfRun < a.rec_hi ? run + kVfRun : a.rec_hi;
  uint32_t k = kf_keyframe_of(begin, a.k_lo, a.k_hi, run);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & (kVfWave - 1u);
  float4 p[kVfPerLane];
  bool keep[kVfPerLane];
#pragma unroll
  for (uint32_t j = 0; j < kVfPerLane; j++) {
    const uint64_t i = run + j * kVfThreads + threadIdx.x;
    p[j] = i < run_end ? src[i] : float4{0.f, 0.f, 0.f, 0.f};
    keep[j] = i < run_end && (flags == nullptr || flags[i] == 0u);
  }
  uint32_t loaded = kKfNoId;
  double m[12] = {};
#if LFX_VF_BLOCK
  __shared__ VfLds lds;
  VfLds * block = &lds;
  vf_lds_clear(lds);
#else
  VfLds * block = nullptr;
#endif
  VfTally tally;
#pragma unroll
  for (uint32_t j = 0; j < kVfPerLane; j++) {
    const uint64_t iw = run + j * kVfThreads + wave * kVfWave;   // the step's first record: uniform over the wave
    if (iw >= run_end) {break;}
    while (begin[k + 1u] <= iw) {k++;}       // (iw < rec_hi <= begin[k_hi]: k stays below k_hi)
    const uint64_t step_end = iw + kVfWave < run_end ? iw + kVfWave : run_end;
    const uint64_t i = iw + lane;
    float4 q = p[j];
    if (begin[k + 1u] >= step_end) {
      if (k != loaded) {
#pragma unroll
        for (int c = 0; c < 12; c++) {m[c] = poses[12u * (size_t)k + c];}
        loaded = k;
      }
      q = pcl_transform_record(m, p[j]);
    } else if (i < step_end) {
      q = pcl_transform_record(poses + 12u * (size_t)kf_keyframe_of(begin, k, a.k_hi, i), p[j]);
    }
    // (the whole wave is here again: the shuffles of the merge need every lane)
    vf_accumulate(table, log2_slots, inv, counters, q, rank0 + (i - a.rec_lo), keep[j], tally, block);
  }
  vf_flush(tally, counters);
#if LFX_VF_BLOCK
  vf_lds_flush(lds, table, log2_slots, counters);
#endif
}

// --- emit -----------------------------------------------------------------------------------------------------------------------
// Voxels go out in the order of their least ranks.  mark: the bit of every surviving voxel's least rank is set in a bitmap
// over ranks (one bit per rank handed out; least ranks are distinct, a rank belongs to one record).  tile: per word of a tile
// of kVfTileWords words the set bits before it in the tile, and the tile's total.  scan (one workgroup): the totals to
// their exclusive prefix.  write: a voxel's place is its tile's prefix + its word's + the set bits below its own.

__global__ __launch_bounds__(kVfThreads) void voxel_filter_mark_kernel(
  const VfEntry * __restrict__ table, uint64_t slots, uint32_t min_points, uint64_t n_ranks, uint32_t * __restrict__ bitmap,
  unsigned long long * __restrict__ counters)
{
  __shared__ uint32_t sh[kVfThreads / 64];
  const uint64_t i = (uint64_t)blockIdx.x * kVfThreads + threadIdx.x;
  bool used = false;
  if (i < slots) {
    const VfEntry e = table[i];
    used = e.key != 0ull;
    if (used && e.count >= (uint64_t)min_points && e.rank < n_ranks) {atomicOr(bitmap + (e.rank >> 5), 1u << (uint32_t)(e.rank & 31u));}
  }
  roll_count(used, sh, counters + kVfVoxels);
}

__global__ __launch_bounds__(kVfThreads) void voxel_filter_tile_kernel(
  const uint32_t * __restrict__ bitmap, uint64_t n_words, uint32_t * __restrict__ word_before, uint64_t * __restrict__ tile_count)
{
  __shared__ uint32_t sh[2 * (kVfThreads / 64) + 1];
  const uint64_t base = (uint64_t)blockIdx.x * kVfTileWords + 4u * threadIdx.x;
  uint32_t c[4], v = 0u;
#pragma unroll
  for (uint32_t q = 0; q < 4u; q++) {
    c[q] = base + q < n_words ? (uint32_t)__popc(bitmap[base + q]) : 0u;
    v += c[q];
  }
  uint32_t total;
  uint32_t at = roll_block_scan(v, sh, total);
#pragma unroll
  for (uint32_t q = 0; q < 4u; q++) {
    if (base + q < n_words) {word_before[base + q] = at;}
    at += c[q];
  }
  if (threadIdx.x == 0u) {tile_count[blockIdx.x] = total;}
}

// One workgroup: tile_count[0 .. n_tiles) becomes its exclusive prefix, the total goes to the counters.  Shares, an LDS scan
// of their sums and a second pass, as keyframes_mask_scan_kernel does it.
__global__ __launch_bounds__(kVfThreads) void voxel_filter_scan_kernel(uint64_t * __restrict__ tile_count, uint32_t n_tiles, unsigned long long * __restrict__ counters)
{
  __shared__ uint64_t s_sum[kVfThreads];
  const uint32_t t = threadIdx.x;
  const uint32_t share = (n_tiles + kVfThreads - 1u) / kVfThreads;
  const uint32_t lo = t * share < n_tiles ? t * share : n_tiles, hi = lo + share < n_tiles ? lo + share : n_tiles;
  uint64_t sum = 0;
  for (uint32_t b = lo; b < hi; b++) {sum += tile_count[b];}
  s_sum[t] = sum;
  __syncthreads();
  for (uint32_t d = 1u; d < kVfThreads; d <<= 1) {
    const uint64_t v = t >= d ? s_sum[t - d] : 0u;
    __syncthreads();
    s_sum[t] += v;
    __syncthreads();
  }
  uint64_t e = s_sum[t] - sum;
  for (uint32_t b = lo; b < hi; b++) {
    const uint64_t c = tile_count[b];
    tile_count[b] = e;
    e += c;
  }
  if (t == kVfThreads - 1u) {counters[kVfWritten] = s_sum[t];}
}

// the centroid of the model along one axis
__device__ inline float vf_centroid(int32_t v, int64_t s, uint64_t n, float inv)
{
  return (float)((((double)v) + ((double)s / (double)n) * 0x1p-24) / (double)inv);
}

// The surviving voxels whose place lies in [window_lo, window_lo + window) to out[place - window_lo] (counts_out likewise,
// where given): the public emit has the window [0, capacity), the filtered save walks the places in chunks.
__global__ __launch_bounds__(kVfThreads) void voxel_filter_write_kernel(
  const VfEntry * __restrict__ table, uint64_t slots, uint32_t min_points, float inv, uint64_t n_ranks, const uint32_t * __restrict__ bitmap,
  const uint32_t * __restrict__ word_before, const uint64_t * __restrict__ tile_before, float4 * __restrict__ out, uint32_t * __restrict__ counts_out,
  uint64_t window_lo, uint64_t window)
{
  const uint64_t i = (uint64_t)blockIdx.x * kVfThreads + threadIdx.x;
  if (i >= slots) {return;}
  const VfEntry e = table[i];
  if (e.key == 0ull || e.count < (uint64_t)min_points || e.rank >= n_ranks) {return;}
  const uint64_t w = e.rank >> 5;
  const uint64_t at = tile_before[w / kVfTileWords] + word_before[w] + (uint32_t)__popc(bitmap[w] & ((1u << (uint32_t)(e.rank & 31u)) - 1u));
  if (at < window_lo || at - window_lo >= window) {return;}
  float4 c;
  c.x = vf_centroid(vf_unkey(e.key, 0), e.s[0], e.count, inv);
  c.y = vf_centroid(vf_unkey(e.key, 1), e.s[1], e.count, inv);
  c.z = vf_centroid(vf_unkey(e.key, 2), e.s[2], e.count, inv);
  c.w = 1.0f;
  out[at - window_lo] = c;
  if (counts_out) {counts_out[at - window_lo] = e.count > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)e.count;}
}

}  // namespace lfx
