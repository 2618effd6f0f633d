// lfx_kernels_visibility.hpp -- the device side of the visibility votes (lfx_visibility.hip; include/lfx.h, the visibility
// section): every non-empty keyframe of a window becomes a range image of its own records, and every record of the window is
// looked for in the images of the keyframes near its own.  Integer minima and integer counts only: the bytes do not depend on
// the schedule.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "lfx_kernels_image.hpp"
#include "lfx_kernels_transform.hpp"

namespace lfx
{

constexpr int kVisThreads = 256;
constexpr uint32_t kVisWave = 64;
constexpr uint32_t kVisEmpty = 0xFFFFFFFFu;      // a cell without a record (the bits of a positive finite float lie below)
constexpr uint32_t kVisNoCell = 0xFFFFFFFFu;

// the counters of a run, 64-bit, zeroed in-stream ahead of it
enum : uint32_t {kVisPairs = 0, kVisRecords = 1, kVisVoted = 3, kVisDynamic = 5, kVisOccupied = 7, kVisCounters = 8};

// A call's table of doubles: lfx_visibility_tables' values, [0, W) col_cos, [W, 2 W) col_sin, [2 W, 2 W + H + 1) row_tan.
__host__ __device__ inline uint32_t vis_table_doubles(uint32_t H, uint32_t W) {return 2u * W + H + 1u;}

struct VisArgs
{
  const float4 * records[2];            // the store's sensor-frame records
  const uint64_t * begin[2];            // the store's begin tables
  const double * poses;                 // the store's poses
  const double * table;                 // vis_table_doubles(H, W) doubles
  const uint32_t * viewers;             // the window's non-empty keyframes, ascending; the chunk is [chunk_lo, chunk_lo + chunk_n)
  uint32_t * images;                    // [chunk_n][H * W]
  unsigned long long * counters;        // [kVisCounters]
  uint32_t H, W, guard, min_through, agree_weight;
  uint32_t first, count;                // the window
  uint32_t n_viewers, chunk_lo, chunk_n;
  uint32_t first_chunk, last_chunk;     // the first chunk starts the vote words at 0; the last writes the flags and counts
  double min_range, max_range, radius2, margin_abs, margin_rel;
};

// The cell of a point and its range, or kVisNoCell: the header's rule -- the gates and the column are the shared ones
// (lfx_kernels_image.hpp), the range comparison and the row (a search over row_tan) are its own.
__device__ inline uint32_t vis_cell(const VisArgs & A, const double * __restrict__ table, double x, double y, double z, double & r)
{
  double xy2;
  if (!planar_range(x, y, z, xy2, r)) {return kVisNoCell;}
  const double rho = sqrt(xy2);                     // (beside r's: the two square roots overlap)
  if (r < A.min_range || r >= A.max_range) {return kVisNoCell;}
  const double * rt = table + 2u * A.W;
  if (z < rt[0] * rho || z >= rt[A.H] * rho) {return kVisNoCell;}
  const uint32_t col = azimuth_column(table, table + A.W, A.W, x, y, y >= 0.0);
  uint32_t rlo = 0, rhi = A.H - 1u;
  while (rlo < rhi) {
    const uint32_t mid = (rlo + rhi + 1u) >> 1;
    if (z >= rt[mid] * rho) {rlo = mid;} else {rhi = mid - 1u;}
  }
  return rlo * A.W + col;
}

// grid (x, chunk_n): workgroups (., s) walk the records of both kinds of viewer chunk_lo + s with a grid stride, each record
// with a cell taking part in that cell's 32-bit minimum on the bits of (float)r -- positive, so they order as it does.  The
// images were set to kVisEmpty in-stream ahead of the launch.
__global__ __launch_bounds__(kVisThreads) void visibility_image_kernel(const VisArgs A)
{
  const uint32_t s = blockIdx.y, v = A.viewers[A.chunk_lo + s];
  uint32_t * img = A.images + (size_t)s * A.H * A.W;
  for (int kind = 0; kind < 2; kind++) {
    const uint64_t b0 = A.begin[kind][v], n = A.begin[kind][v + 1u] - b0;
    const float4 * __restrict__ rec = A.records[kind] + b0;
    for (uint64_t i = (uint64_t)blockIdx.x * kVisThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kVisThreads) {
      const float4 p = rec[i];
      double r;
      const uint32_t cell = vis_cell(A, A.table, (double)p.x, (double)p.y, (double)p.z, r);
      if (cell != kVisNoCell) {atomicMin(&img[cell], __float_as_uint((float)r));}
    }
  }
}

// One thread per cell of the chunk's images: the occupied ones counted, one integer add per wave.
__global__ __launch_bounds__(kVisThreads) void visibility_occupied_kernel(const VisArgs A, uint64_t cells)
{
  const uint64_t i = (uint64_t)blockIdx.x * kVisThreads + threadIdx.x;
  const bool occupied = i < cells && A.images[i] != kVisEmpty;
  const unsigned long long wave = __ballot(occupied);
  if ((threadIdx.x & (kVisWave - 1u)) == 0u && wave) {atomicAdd(&A.counters[kVisOccupied], (unsigned long long)__popcll(wave));}
}

// One thread per viewer i of the window's list: the viewers j != i within the radius of it, (dx^2 + dy^2) + dz^2 <= radius^2
// in double in that order.  The list holds the window's non-empty keyframes, so the sum is the run's n_pairs.
__global__ __launch_bounds__(kVisThreads) void visibility_pairs_kernel(const VisArgs A)
{
  const uint32_t i = blockIdx.x * kVisThreads + threadIdx.x;
  unsigned long long mine = 0;
  if (i < A.n_viewers) {
    const double * ti = A.poses + 12u * (size_t)A.viewers[i];
    const double x = ti[3], y = ti[7], z = ti[11];
    for (uint32_t j = 0; j < A.n_viewers; j++) {
      const double * tj = A.poses + 12u * (size_t)A.viewers[j];
      const double dx = x - tj[3], dy = y - tj[7], dz = z - tj[11];
      mine += (j != i && (dx * dx + dy * dy) + dz * dz <= A.radius2) ? 1u : 0u;
    }
  }
  for (int d = 32; d > 0; d >>= 1) {mine += __shfl_down(mine, d, 64);}
  if ((threadIdx.x & (kVisWave - 1u)) == 0u && mine) {atomicAdd(&A.counters[kVisPairs], mine);}
}

// The votes of the chunk's viewers on record p of keyframe k (pose mk), added to `word`.  With k and mk uniform over the wave
// the pair test is a uniform branch and the viewer's pose comes through the scalar path.
__device__ __forceinline__ uint32_t vis_votes(const VisArgs & A, const double * __restrict__ poses, const double * __restrict__ table,
  const uint32_t * __restrict__ viewers, const uint32_t * __restrict__ images, uint32_t k, const double * mk, const float4 p, uint32_t word)
{
  const float4 w = pcl_transform_record(mk, p);
  const double wx = (double)w.x, wy = (double)w.y, wz = (double)w.z;
  const double kx = mk[3], ky = mk[7], kz = mk[11];
  const int g = (int)A.guard, H = (int)A.H, W = (int)A.W;
  for (uint32_t s = 0; s < A.chunk_n; s++) {
    const uint32_t v = viewers[A.chunk_lo + s];
    if (v == k) {continue;}
    const double * mv = poses + 12u * (size_t)v;
    const double tx = mv[3], ty = mv[7], tz = mv[11];
    const double ex = kx - tx, ey = ky - ty, ez = kz - tz;
    if (!((ex * ex + ey * ey) + ez * ez <= A.radius2)) {continue;}
    const double dx = wx - tx, dy = wy - ty, dz = wz - tz;
    const double qx = (mv[0] * dx + mv[4] * dy) + mv[8] * dz;
    const double qy = (mv[1] * dx + mv[5] * dy) + mv[9] * dz;
    const double qz = (mv[2] * dx + mv[6] * dy) + mv[10] * dz;
    double rq;
    const uint32_t cell = vis_cell(A, table, qx, qy, qz, rq);
    if (cell == kVisNoCell) {continue;}
    const uint32_t * __restrict__ img = images + (size_t)s * A.H * A.W;
    const uint32_t centre = img[cell];
    if (centre == kVisEmpty) {continue;}
    const double mr = A.margin_rel * rq;
    const double m = A.margin_abs > mr ? A.margin_abs : mr;
    const double r_far = rq + m, r_near = rq - m;
    const int row = (int)(cell / A.W), col = (int)(cell - (uint32_t)row * A.W);
    bool objects = false;
    for (int dr = -g; dr <= g; dr++) {
      const int rr = row + dr;
      if (rr < 0 || rr >= H) {continue;}
      for (int dc = -g; dc <= g; dc++) {
        int cc = col + dc;
        cc = cc < 0 ? cc + W : (cc >= W ? cc - W : cc);
        const uint32_t bits = img[(uint32_t)rr * A.W + (uint32_t)cc];
        objects = objects || (bits != kVisEmpty && (double)__uint_as_float(bits) <= r_far);
      }
    }
    const double rc = (double)__uint_as_float(centre);
    if (!objects) {word += 1u;} else if (r_near <= rc && rc <= r_far) {word += 0x10000u;}
  }
  return word;
}

// One lane per record of one kind of the window, records [rec_lo, rec_hi) of keyframes [first, first + count); `words` is
// addressed by the record's index less word_off.  A wave whose 64 records lie in one keyframe keeps that keyframe uniform;
// where a keyframe boundary falls inside the wave every lane searches for its own.  A lane reads its word (0 on the first
// chunk), adds the chunk's votes and writes it back; on the last chunk it writes the flag byte and the wave adds its counts.
__global__ __launch_bounds__(kVisThreads) void visibility_vote_kernel(const VisArgs A, const float4 * __restrict__ records,
  const uint64_t * __restrict__ begin, const double * __restrict__ poses, const double * __restrict__ table,
  const uint32_t * __restrict__ viewers, const uint32_t * __restrict__ images, int kind, uint64_t rec_lo, uint64_t rec_hi,
  uint32_t * __restrict__ words, uint64_t word_off, uint8_t * __restrict__ flags)
{
  const uint32_t lane = threadIdx.x & (kVisWave - 1u);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t iw = rec_lo + (uint64_t)blockIdx.x * kVisThreads + wave * kVisWave;   // the wave's first record: uniform
  if (iw >= rec_hi) {return;}
  const uint64_t wave_end = iw + kVisWave < rec_hi ? iw + kVisWave : rec_hi;
  const uint64_t i = iw + lane;
  const bool live = i < wave_end;
  const uint32_t k_hi = A.first + A.count;
  uint32_t lo = A.first, hi = k_hi;          // begin[lo] <= iw < begin[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (begin[mid] <= iw) {lo = mid;} else {hi = mid;}
  }
  uint32_t word = 0u;
  if (live) {
    const float4 p = records[i];
    if (words != nullptr && !A.first_chunk) {word = words[i - word_off];}
    if (begin[lo + 1u] >= wave_end) {
      const uint32_t k = __builtin_amdgcn_readfirstlane(lo);
      double mk[12];
#pragma unroll
      for (int q = 0; q < 12; q++) {mk[q] = poses[12u * (size_t)k + q];}
      word = vis_votes(A, poses, table, viewers, images, k, mk, p, word);
    } else {
      uint32_t l = lo, h = k_hi;
      while (h - l > 1u) {
        const uint32_t mid = l + ((h - l) >> 1);
        if (begin[mid] <= i) {l = mid;} else {h = mid;}
      }
      double mk[12];
#pragma unroll
      for (int q = 0; q < 12; q++) {mk[q] = poses[12u * (size_t)l + q];}
      word = vis_votes(A, poses, table, viewers, images, l, mk, p, word);
    }
    if (words != nullptr) {words[i - word_off] = word;}
  }
  if (!A.last_chunk) {return;}
  const uint32_t through = word & 0xFFFFu, agree = word >> 16;
  const bool dynamic = live && through >= A.min_through && (unsigned long long)agree * A.agree_weight < through;
  if (live) {flags[i] = dynamic ? 1 : 0;}
  const unsigned long long b_live = __ballot(live), b_voted = __ballot(live && word != 0u), b_dyn = __ballot(dynamic);
  if (lane == 0u) {
    atomicAdd(&A.counters[kVisRecords + kind], (unsigned long long)__popcll(b_live));
    if (b_voted) {atomicAdd(&A.counters[kVisVoted + kind], (unsigned long long)__popcll(b_voted));}
    if (b_dyn) {atomicAdd(&A.counters[kVisDynamic + kind], (unsigned long long)__popcll(b_dyn));}
  }
}

}  // namespace lfx
