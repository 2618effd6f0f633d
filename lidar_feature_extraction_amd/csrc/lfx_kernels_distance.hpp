// lfx_kernels_distance.hpp -- distance fields and costmaps of 2-D occupancy grids (include/lfx.h, the distance section; no
// reference counterpart, the models are the exact separable Euclidean distance transform and nav2's inflation layer).  The
// transform is integer arithmetic on squared cell distances: a column pass (every cell's class, then its vertical distance
// to the nearest obstacle of its column) and a row pass (per row the lower envelope of the parabolas (x - x')^2 + g(x')^2).
// Both passes are templated on INVERT, which makes the non-obstacle cells the sites: the `inside` field.  Nothing here is
// floating point before distance_metres_kernel, the only atomics are integer minima, maxima and sums, and no workgroup
// waits for another one: the phases are launches of their own.  The same grid gives the same bytes whatever the schedule.
#pragma once

#include "lfx_kernels_occvalue.hpp"

#pragma clang fp contract(off)

namespace lfx
{

constexpr int kDistThreads = 256;
constexpr uint32_t kDistSegRows = 64;          // a y-segment of the column pass: its sites are one 64-bit mask per column
constexpr uint32_t kDistSearchMax = 64;        // caps of 1 .. this many cells: the row pass is the outward search
constexpr int kDistSites = 16;                 // sites (columns of a row) a thread of the envelope kernel owns
constexpr uint32_t kDistFar = 0xFFFFFFFFu;
constexpr uint32_t kDistNoSite = 0xFFFFu;      // a column distance: no site in the column
constexpr uint32_t kDistDead = 0xFFFFFFFFu;    // the envelope kernel: a site that is no interior candidate any more
constexpr uint8_t kDistFree = 0, kDistUnknown = 1, kDistObstacle = 2;
// the stats words, uint64 each
enum DistStat : int {kDistNObstacle, kDistNUnknown, kDistNFar, kDistMaxD2, kDistStats};

// --- classes -----------------------------------------------------------------------------------------------------------------
struct DistClassifyArgs
{
  const int8_t * grid;                  // [H][W] in lfx_occupancy_emit's format (the int8 form)
  OccEmitArgs E;                        // the counts form: the emit's own arguments, out unused
  uint32_t W, H;
  int32_t occupied_percent;
  uint32_t unknown_is_obstacle;
  uint8_t * cls;                        // [H][W]
  unsigned long long * mask;            // [segments][W]: bit j set iff row 64 * segment + j of the column is an obstacle
  unsigned long long * stats;           // [kDistStats]
};

// grid (tiles of W, segments): one thread per column and y-segment walks its 64 rows -- every row access of a wave is one
// run of consecutive cells -- and leaves each cell's class and the segment's obstacle mask.  COUNTS: the cell's value is
// occ_value's, from the two count arrays; no int8 grid exists in between.
template<bool COUNTS>
__global__ __launch_bounds__(kDistThreads) void distance_classify_kernel(const DistClassifyArgs A)
{
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, seg = blockIdx.y;
  uint32_t n_obstacle = 0, n_unknown = 0;
  if (x < A.W) {
    const uint32_t y0 = seg * kDistSegRows, rows = A.H - y0 < kDistSegRows ? A.H - y0 : kDistSegRows;
    unsigned long long m = 0ull;
    for (uint32_t j = 0; j < rows; j++) {
      const uint64_t cell = (uint64_t)(y0 + j) * A.W + x;
      const int v = COUNTS ? (int)occ_value(A.E, cell) : (int)A.grid[cell];
      const bool obstacle = v >= A.occupied_percent || (v < 0 && A.unknown_is_obstacle != 0u);
      A.cls[cell] = obstacle ? kDistObstacle : (v < 0 ? kDistUnknown : kDistFree);
      m |= (unsigned long long)(obstacle ? 1u : 0u) << j;
      n_obstacle += obstacle ? 1u : 0u;
      n_unknown += (!obstacle && v < 0) ? 1u : 0u;
    }
    A.mask[(size_t)seg * A.W + x] = m;
  }
  occ_count(A.stats + kDistNObstacle, n_obstacle);
  occ_count(A.stats + kDistNUnknown, n_unknown);
}

// --- the column pass -----------------------------------------------------------------------------------------------------------
struct DistColumnArgs
{
  const unsigned long long * mask;      // [segments][W]
  uint16_t * below, * above;            // [segments][W]: rows from the segment's first row down to the nearest site under the
                                        // segment, and from its 64th row up to the nearest site over it; kDistNoSite: none
  uint16_t * g;                         // [H][W]: the vertical distance to the nearest site of the column, kDistNoSite: none
  uint32_t W, H, segments;
};

// the sites of a segment of a column: the obstacles, or (INVERT) the cells of the grid that are none
template<bool INVERT>
__device__ inline unsigned long long dist_sites(const DistColumnArgs & A, uint32_t seg, uint32_t x)
{
  unsigned long long m = A.mask[(size_t)seg * A.W + x];
  if (INVERT) {
    const uint32_t rows = A.H - seg * kDistSegRows;
    m = ~m;
    if (rows < kDistSegRows) {m &= (1ull << rows) - 1ull;}
  }
  return m;
}

// The carry: grid (tiles of W, 2), one thread per column walks the segments upwards (blockIdx.y 0: `below`) or downwards
// (1: `above`) with the row of the last site it has seen -- at most 256 masks, whose loads do not depend on each other.
template<bool INVERT>
__global__ __launch_bounds__(kDistThreads) void distance_carry_kernel(const DistColumnArgs A)
{
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= A.W) {return;}
  int32_t seen = -1;
  if (blockIdx.y == 0u) {
    for (uint32_t seg = 0; seg < A.segments; seg++) {
      const int32_t y0 = (int32_t)(seg * kDistSegRows);
      A.below[(size_t)seg * A.W + x] = (uint16_t)(seen < 0 ? kDistNoSite : (uint32_t)(y0 - seen));
      const unsigned long long m = dist_sites<INVERT>(A, seg, x);
      if (m) {seen = y0 + 63 - __clzll((long long)m);}
    }
  } else {
    for (uint32_t seg = A.segments; seg-- > 0u; ) {
      const int32_t y1 = (int32_t)(seg * kDistSegRows + kDistSegRows - 1u);
      A.above[(size_t)seg * A.W + x] = (uint16_t)(seen < 0 ? kDistNoSite : (uint32_t)(seen - y1));
      const unsigned long long m = dist_sites<INVERT>(A, seg, x);
      if (m) {seen = (int32_t)(seg * kDistSegRows) + (__ffsll((long long)m) - 1);}
    }
  }
}

// grid (tiles of W, segments): one thread per column and y-segment; every row's distance comes from the segment's mask (the
// highest site at or under the row, the lowest at or over it) or, where the segment has none on that side, from the carry.
template<bool INVERT>
__global__ __launch_bounds__(kDistThreads) void distance_column_kernel(const DistColumnArgs A)
{
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, seg = blockIdx.y;
  if (x >= A.W) {return;}
  const uint32_t y0 = seg * kDistSegRows, rows = A.H - y0 < kDistSegRows ? A.H - y0 : kDistSegRows;
  const unsigned long long m = dist_sites<INVERT>(A, seg, x);
  const uint32_t below = A.below[(size_t)seg * A.W + x], above = A.above[(size_t)seg * A.W + x];
  for (uint32_t j = 0; j < rows; j++) {
    const unsigned long long low = m & (~0ull >> (63u - j)), high = m >> j;
    const uint32_t down = low ? j - (63u - (uint32_t)__clzll((long long)low)) : (below == kDistNoSite ? kDistNoSite : j + below);
    const uint32_t up = high ? (uint32_t)(__ffsll((long long)high) - 1) : (above == kDistNoSite ? kDistNoSite : (kDistSegRows - 1u - j) + above);
    A.g[(uint64_t)(y0 + j) * A.W + x] = (uint16_t)(down < up ? down : up);
  }
}

// --- the row pass ---------------------------------------------------------------------------------------------------------------
struct DistRowArgs
{
  const uint16_t * g;                   // [H][W]
  uint32_t * out;                       // [H][W]: d2, or i2
  uint32_t W, H;
  uint32_t cap;                         // R in cells, 0: none
  unsigned long long * stats;           // [kDistStats], or nullptr (i2 has none)
};

// (x - j)^2 + g^2 of a site: both squares are at most 16383^2, their sum fits 32 bits with a bit to spare
__device__ inline uint32_t dist_eval(uint32_t x, uint32_t j, uint32_t g)
{
  const uint32_t dx = x > j ? x - j : j - x;
  return dx * dx + g * g;
}

// the cap: a minimum above R^2 is FAR (R <= 32767: R^2 fits; compared in 64 bits all the same)
__device__ inline uint32_t dist_capped(uint32_t v, uint32_t cap)
{
  return (cap != 0u && v != kDistFar && (uint64_t)v > (uint64_t)cap * (uint64_t)cap) ? kDistFar : v;
}

// n_far and max_d2 of the workgroup's cells: every thread of the workgroup calls it
__device__ inline void dist_row_stats(unsigned long long * stats, uint32_t n_far, uint32_t most)
{
  if (stats == nullptr) {return;}
  occ_count(stats + kDistNFar, n_far);
  for (int d = 32; d; d >>= 1) {const uint32_t o = __shfl_down(most, d); most = o > most ? o : most;}
  if ((threadIdx.x & 63u) == 0u && most) {atomicMax(stats + kDistMaxD2, (unsigned long long)most);}
}

// One workgroup per row, the row of g in LDS (2 W bytes, dynamic); a cap of 1 .. kDistSearchMax cells.  Per cell the outward
// search: columns x - k and x + k for k = 1, 2, ... until k^2 >= the best so far or k > R.  Exact under the cap: a column more
// than R away gives more than R^2, which is FAR whatever it is.
__global__ __launch_bounds__(kDistThreads) void distance_row_search_kernel(const DistRowArgs A)
{
  extern __shared__ unsigned long long dist_lds[];
  uint16_t * row = reinterpret_cast<uint16_t *>(dist_lds);
  const uint32_t y = blockIdx.x;
  const uint16_t * g = A.g + (uint64_t)y * A.W;
  for (uint32_t x = threadIdx.x; x < A.W; x += blockDim.x) {row[x] = g[x];}
  __syncthreads();
  uint32_t n_far = 0, most = 0;
  for (uint32_t x = threadIdx.x; x < A.W; x += blockDim.x) {
    const uint32_t g0 = row[x];
    uint32_t best = g0 == kDistNoSite ? kDistFar : g0 * g0;
    for (uint32_t k = 1; k <= A.cap && k * k < best; k++) {
      if (x >= k) {
        const uint32_t gl = row[x - k];
        if (gl != kDistNoSite) {const uint32_t v = k * k + gl * gl; best = v < best ? v : best;}
      }
      if (x + k < A.W) {
        const uint32_t gr = row[x + k];
        if (gr != kDistNoSite) {const uint32_t v = k * k + gr * gr; best = v < best ? v : best;}
      }
    }
    best = dist_capped(best, A.cap);
    A.out[(uint64_t)y * A.W + x] = best;
    n_far += best == kDistFar ? 1u : 0u;
    most = (best != kDistFar && best > most) ? best : most;
  }
  dist_row_stats(A.stats, n_far, most);
}

// One workgroup of T threads per row, W <= 16 T; any cap.  The row's minimum as a monotone-argmin divide and conquer whose
// work is shared by SITE, so that no row makes a thread do more than another:
//   every argmin of a cell x > a is >= every argmin of a (for sites j < i the difference f_j - f_i grows with x), so with the
//   cells at the multiples of S solved, the cell in the middle of two of them has its argmins between theirs.  A level solves
//   all those middle cells at once: a thread per cell evaluates the two end sites, and every site that lies strictly between
//   the argmins of two neighbouring solved cells -- it lies in one such interval, whose index it keeps in a register --
//   enters the 64-bit minimum of that interval's middle cell, (value << 16 | site).  Then the site moves into the left or
//   the right half of its interval, or, being the argmin itself, stops being an interior candidate.
// log2(W) + 1 levels of W evaluations: O(W log W) for any row, no search whose length depends on the input.  LDS (dynamic):
// the minima [(W + 1) / 2 + 1] uint64, then g [W] and the argmins [W] uint16 -- 128 KiB at W = 16384.
template<int T>
__global__ __launch_bounds__(T) void distance_row_envelope_kernel(const DistRowArgs A)
{
  extern __shared__ unsigned long long dist_lds[];
  const uint32_t W = A.W, y = blockIdx.x, tid = threadIdx.x;
  unsigned long long * key = dist_lds;
  uint16_t * grow = reinterpret_cast<uint16_t *>(dist_lds + ((W + 1u) / 2u + 1u));
  uint16_t * srow = grow + ((W + 3u) & ~3u);
  const uint16_t * g = A.g + (uint64_t)y * W;
  uint32_t * out = A.out + (uint64_t)y * W;
  uint32_t gj[kDistSites], at[kDistSites];        // a site's g and its interval (kDistDead: none)
#pragma unroll
  for (int m = 0; m < kDistSites; m++) {
    const uint32_t j = (uint32_t)m * T + tid;
    const uint32_t v = j < W ? (uint32_t)g[j] : kDistNoSite;
    if (j < W) {grow[j] = (uint16_t)v;}
    gj[m] = v;
    at[m] = v == kDistNoSite ? kDistDead : 0u;
  }
  if (tid == 0u) {key[0] = ~0ull;}
  __syncthreads();
  // cell 0: every site is a candidate
#pragma unroll
  for (int m = 0; m < kDistSites; m++) {
    if (at[m] != kDistDead) {
      const uint32_t j = (uint32_t)m * T + tid;
      const unsigned long long k = ((unsigned long long)dist_eval(0u, j, gj[m]) << 16) | j;
      if (k < key[0]) {atomicMin(&key[0], k);}
    }
  }
  __syncthreads();
  const unsigned long long k0 = key[0];
  if (k0 == ~0ull) {                              // (the whole workgroup: a row without a site)
    for (uint32_t x = tid; x < W; x += T) {out[x] = kDistFar;}
    if (A.stats != nullptr && tid == 0u) {atomicAdd(A.stats + kDistNFar, (unsigned long long)W);}
    return;
  }
  const uint32_t s0 = (uint32_t)(k0 & 0xFFFFu);
  if (tid == 0u) {srow[0] = (uint16_t)s0;}
#pragma unroll
  for (int m = 0; m < kDistSites; m++) {
    const uint32_t j = (uint32_t)m * T + tid;
    if (at[m] != kDistDead && j <= s0) {at[m] = kDistDead;}
  }
  __syncthreads();
  uint32_t P = 1u;
  while (P < W) {P <<= 1;}
  for (uint32_t h = P >> 1; h >= 1u; h >>= 1) {
    // solved: the multiples of S; this level: the cells c * S + h below W
    const uint32_t S = 2u * h, cells = W > h ? (W - h - 1u) / S + 1u : 0u;
    for (uint32_t c = tid; c < cells; c += T) {
      const uint32_t x = c * S + h, lo = srow[x - h];
      unsigned long long k = ((unsigned long long)dist_eval(x, lo, grow[lo]) << 16) | lo;
      if (x + h < W) {
        const uint32_t hi = srow[x + h];
        const unsigned long long kh = ((unsigned long long)dist_eval(x, hi, grow[hi]) << 16) | hi;
        k = kh < k ? kh : k;
      }
      key[c] = k;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < kDistSites; m++) {
      const uint32_t c = at[m];
      if (c != kDistDead && c < cells) {
        const uint32_t j = (uint32_t)m * T + tid;
        const unsigned long long k = ((unsigned long long)dist_eval(c * S + h, j, gj[m]) << 16) | j;
        if (k < key[c]) {atomicMin(&key[c], k);}
      }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < kDistSites; m++) {
      const uint32_t c = at[m];
      if (c != kDistDead) {
        if (c < cells) {
          const uint32_t j = (uint32_t)m * T + tid, s = (uint32_t)(key[c] & 0xFFFFu);
          at[m] = j < s ? 2u * c : (j > s ? 2u * c + 1u : kDistDead);
        } else {
          at[m] = 2u * c;                          // (the interval's middle cell lies beyond the row)
        }
      }
    }
    for (uint32_t c = tid; c < cells; c += T) {srow[c * S + h] = (uint16_t)(key[c] & 0xFFFFu);}
    __syncthreads();
  }
  uint32_t n_far = 0, most = 0;
  for (uint32_t x = tid; x < W; x += T) {
    const uint32_t j = srow[x];
    const uint32_t best = dist_capped(dist_eval(x, j, grow[j]), A.cap);
    out[x] = best;
    n_far += best == kDistFar ? 1u : 0u;
    most = (best != kDistFar && best > most) ? best : most;
  }
  dist_row_stats(A.stats, n_far, most);
}

// --- metres and costs --------------------------------------------------------------------------------------------------------------
struct DistOutArgs
{
  const uint8_t * cls;
  const uint32_t * d2, * i2;            // i2: nullptr without `inside`
  uint64_t cells;
  double res;
  float * metres;                       // device memory or a pinned block
  const uint8_t * lut;                  // [rc2 + 1]: lfx_distance_cost_table's bytes
  uint32_t rc2;                         // Rc^2
  uint32_t track_unknown;
  uint8_t * cost;                       // device memory or a pinned block
  bool words;                           // the output is 4-byte aligned
};

// sqrt of a double is the correctly rounded one here as everywhere in HIP device code (the f64 square root is not among the
// operations fast-math flags or the f32 switch relax); tests/test_distance_gpu.py holds every value to numpy's bit for bit
__device__ inline float dist_metres(const DistOutArgs & A, uint64_t c)
{
  if (A.cls[c] != kDistObstacle) {
    const uint32_t d = A.d2[c];
    return d == kDistFar ? __builtin_inff() : (float)(sqrt((double)d) * A.res);
  }
  if (A.i2 == nullptr) {return 0.0f;}
  const uint32_t i = A.i2[c];
  return i == kDistFar ? -__builtin_inff() : -(float)(sqrt((double)i) * A.res);
}

// one cell per thread: a float is a word already; an output that is not 4-byte aligned is written byte by byte
__global__ __launch_bounds__(kDistThreads) void distance_metres_kernel(const DistOutArgs A)
{
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= A.cells) {return;}
  const float v = dist_metres(A, c);
  if (A.words) {
    A.metres[c] = v;
  } else {
    const uint32_t bits = __float_as_uint(v);
    uint8_t * p = reinterpret_cast<uint8_t *>(A.metres) + 4u * c;
    for (uint32_t b = 0; b < 4u; b++) {p[b] = (uint8_t)(bits >> (8u * b));}
  }
}

__device__ inline uint8_t dist_cost(const DistOutArgs & A, uint64_t c)
{
  const uint8_t cl = A.cls[c];
  if (cl == kDistObstacle) {return (uint8_t)254;}
  if (cl == kDistUnknown && A.track_unknown != 0u) {return (uint8_t)255;}
  const uint32_t d = A.d2[c];
  if (d == kDistFar || d > A.rc2) {return (uint8_t)0;}
  return A.lut[d];
}

// four consecutive cells per thread, as occupancy_emit_kernel
__global__ __launch_bounds__(kDistThreads) void distance_costmap_kernel(const DistOutArgs A)
{
  const uint64_t c0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4u;
  if (c0 >= A.cells) {return;}
  if (A.words && c0 + 4u <= A.cells) {
    uint32_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {v |= (uint32_t)dist_cost(A, c0 + j) << (8u * j);}
    *reinterpret_cast<uint32_t *>(A.cost + c0) = v;
  } else {
    for (uint64_t c = c0; c < A.cells && c < c0 + 4u; c++) {A.cost[c] = dist_cost(A, c);}
  }
}

}  // namespace lfx
