// lfx_kernels_occupancy.hpp -- 2-D occupancy grids (include/lfx.h, the occupancy section; no reference counterpart, the model is
// the ray-cast grid of Cartographer / slam_toolbox / gmapping): every scan of a batch reduced to W virtual beams from its
// input records, the beams cast through the grid at the poses of the moment with an integer Bresenham, and the votes turned
// into nav_msgs/OccupancyGrid bytes.  The arithmetic is the header's, in double, unfused; the only atomics are 64-bit integer
// minima and maxima, 32-bit ORs and integer sums, so the same beams and poses give the same bytes whatever the schedule.
// No workgroup waits for another one anywhere: the phases are launches of their own.
#pragma once

#include "lfx_kernels_image.hpp"
#include "lfx_kernels_occvalue.hpp"

#pragma clang fp contract(off)

namespace lfx
{

constexpr int kOccThreads = 256;
constexpr uint32_t kOccNone = 0u, kOccHit = 1u, kOccClear = 2u;   // a beam's kind (the w of its uint4 / float4)
constexpr uint64_t kOccNoMin = ~0ull, kOccNoMax = 0ull;           // a column no candidate has reached
constexpr double kOccCellLimit = 1073741824.0;                    // 2^30: a cell coordinate is below it in size
// the counters block, uint64 each
enum OccCounter : int {kOccHitBeams, kOccClearBeams, kOccSkippedBeams, kOccOccupiedVotes, kOccFreeVotes, kOccWindowMiss, kOccCounters};

// --- reduce ---------------------------------------------------------------------------------------------------------------
struct OccReduceArgs
{
  const uint8_t * pts;                  // the batch's input records
  Layout L;
  const uint32_t * scan_begin;          // [scans + 1] of the batch, in records
  const uint32_t * src;                 // [the add's scans]: the batch scan of every scan added
  const double * poses;                 // the store's poses from the add's first scan on
  const double * table;                 // col_cos [W], col_sin [W]
  const uint8_t * cls;                  // per input record of the batch, or nullptr
  uint32_t obstacle_mask, clear_mask;
  uint32_t first;                       // the chunk's first scan among the add's; the keys hold the chunk's scans only
  uint32_t scans;                       // of the chunk
  uint32_t W;
  double min_range, max_range, z_min, z_max;
  unsigned long long * kmin, * kmax;    // [chunk scans][W] each
  uint4 * beams;                        // the store's beams from the add's first scan on
};

// grid (chunks, the chunk's scans) as segment_project_kernel's; a grid-stride walk over the scan's input records, each
// candidate taking part in its column's 64-bit minimum (obstacles: least kf, then lower index) or maximum (clear: greatest
// kf, then lower index -- the index enters complemented).  The workgroup keeps both tables in LDS (16 W bytes, dynamic) and
// sends what it found to the global tables once, a column that no record of its reached not at all: a scan's records meet
// in W columns, 64 to a column for a 64-ring sensor, and the global atomics were what the kernel waited for.  Minima of
// minima and maxima of maxima: the same keys win.  XYZ16: the canonical records, read with one load.
template<bool XYZ16>
__global__ __launch_bounds__(kOccThreads) void occupancy_reduce_kernel(const OccReduceArgs A)
{
  extern __shared__ unsigned long long occ_keys[];                 // [2][W]
  const uint32_t ls = blockIdx.y, k = A.first + ls, s = A.src[k];
  const uint32_t b0 = A.scan_begin[s], n = A.scan_begin[s + 1] - b0;
  if (blockIdx.x * blockDim.x >= n) {return;}                      // (the whole workgroup)
  const uint8_t * base = A.pts + (size_t)b0 * A.L.step;
  const double * m = A.poses + 12u * (size_t)k;
  const double r0 = m[0], r1 = m[1], r2 = m[2], r4 = m[4], r5 = m[5], r6 = m[6], r8 = m[8], r9 = m[9], r10 = m[10];
  unsigned long long * kmin = occ_keys, * kmax = occ_keys + A.W;
  for (uint32_t c = threadIdx.x; c < A.W; c += blockDim.x) {kmin[c] = kOccNoMin; kmax[c] = kOccNoMax;}
  __syncthreads();
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    float xf, yf, zf;
    load_xyz<XYZ16>(base + (size_t)i * A.L.step, A.L, xf, yf, zf);
    const double x = (double)xf, y = (double)yf, z = (double)zf;
    double xy2, r;
    if (!planar_range(x, y, z, xy2, r)) {continue;}
    if (r < A.min_range || r >= A.max_range) {continue;}
    const double dx = (r0 * x + r1 * y) + r2 * z, dy = (r4 * x + r5 * y) + r6 * z, dz = (r8 * x + r9 * y) + r10 * z;
    const double h2 = dx * dx + dy * dy;
    if (h2 == 0.0) {continue;}
    const unsigned long long kf = (unsigned long long)__float_as_uint((float)h2) << 32;
    const uint32_t col = azimuth_column(A.table, A.table + A.W, A.W, dx, dy, dy >= 0.0);
    bool obstacle_ok = true, clear_ok = true;
    if (A.cls != nullptr) {
      const uint32_t c = A.cls[(size_t)b0 + i];
      obstacle_ok = c < 4u && ((A.obstacle_mask >> c) & 1u);
      clear_ok = c < 4u && ((A.clear_mask >> c) & 1u);
    }
    if (A.z_min <= dz && dz <= A.z_max && obstacle_ok) {
      atomicMin(kmin + col, kf | (unsigned long long)i);
    } else if (clear_ok) {
      atomicMax(kmax + col, kf | (unsigned long long)(0xFFFFFFFFu - i));
    }
  }
  __syncthreads();
  unsigned long long * gmin = A.kmin + (size_t)ls * A.W, * gmax = A.kmax + (size_t)ls * A.W;
  for (uint32_t c = threadIdx.x; c < A.W; c += blockDim.x) {
    const unsigned long long lo = kmin[c], hi = kmax[c];
    if (lo != kOccNoMin) {atomicMin(gmin + c, lo);}
    if (hi != kOccNoMax) {atomicMax(gmax + c, hi);}
  }
}

// One thread per (scan of the chunk, column): the winner's x, y, z fetched from its record bit for bit, and its kind.
__global__ __launch_bounds__(kOccThreads) void occupancy_resolve_kernel(const OccReduceArgs A)
{
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= A.scans * A.W) {return;}
  const uint32_t ls = t / A.W, k = A.first + ls, s = A.src[k];
  const unsigned long long lo = A.kmin[t], hi = A.kmax[t];
  uint4 beam = make_uint4(0u, 0u, 0u, kOccNone);
  if (lo != kOccNoMin || hi != kOccNoMax) {
    const uint32_t i = lo != kOccNoMin ? (uint32_t)lo : 0xFFFFFFFFu - (uint32_t)hi;
    const uint8_t * rec = A.pts + ((size_t)A.scan_begin[s] + i) * A.L.step;
    float x, y, z;
    load_xyz<false>(rec, A.L, x, y, z);
    beam = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), lo != kOccNoMin ? kOccHit : kOccClear);
  }
  A.beams[(size_t)k * A.W + (t - ls * A.W)] = beam;
}

// --- render ----------------------------------------------------------------------------------------------------------------
struct OccRenderArgs
{
  const uint4 * beams;                  // the store's
  const double * poses;
  uint32_t first, scans;                // the chunk: scans [first, first + scans) of the store
  uint32_t W, width, height;
  int64_t side, reach;                  // the window's side in cells, and the origin cell's distance from its lower edges
  uint32_t words;                       // 32-bit words of one bitmap (a multiple of 4)
  double origin_x, origin_y, inv_res;
  uint32_t * free_bits, * hit_bits;     // [chunk scans][words] each: all zero between two chunks
  uint32_t * hits, * misses;            // [height][width]
  unsigned long long * counters;        // [kOccCounters]
};

// floor((v - origin) * inv_res) as a cell coordinate: false where it is not finite or not below 2^30 in size
__device__ inline bool occ_cell(double v, double origin, double inv_res, int64_t & out)
{
  const double c = floor((v - origin) * inv_res);
  if (!(fabs(c) < kOccCellLimit)) {return false;}
  out = (int64_t)c;
  return true;
}

__device__ inline bool occ_in_grid(const OccRenderArgs & A, int64_t x, int64_t y)
{
  return x >= 0 && x < (int64_t)A.width && y >= 0 && y < (int64_t)A.height;
}

// one bit of a scan's bitmap: tested with a plain load first -- near the sensor most bits are set already
__device__ inline void occ_set(uint32_t * bits, int64_t bit)
{
  uint32_t * word = bits + (bit >> 5);
  const uint32_t mask = 1u << (uint32_t)(bit & 31);
  if (!(*word & mask)) {atomicOr(word, mask);}
}

// The walk's state after k steps, 0 <= k <= max(ax, ay), without walking them.  The major axis moves at every step; along
// it err stays within one major length of its start (x major: ax/2 - ay <= err < 3 ax/2 - ay; y major: ax - 3 ay/2 < err <=
// ax - ay/2), which leaves one value for the minor steps so far: ceil((2 k minor - major) / (2 major)).  Products stay
// below 2^63: a coordinate is below 2^30 in size, so ax, ay and k are at most 2^31.
__device__ inline void occ_jump(int64_t ox, int64_t oy, int64_t ax, int64_t ay, int64_t sx, int64_t sy, int64_t k, int64_t & cx, int64_t & cy, int64_t & err)
{
  if (k == 0) {return;}
  const bool x_major = ax >= ay;
  const uint64_t major = (uint64_t)(x_major ? ax : ay), minor = (uint64_t)(x_major ? ay : ax);
  const uint64_t twice = 2u * (uint64_t)k * minor;
  const int64_t j = twice <= major ? 0 : (int64_t)((twice + major - 1u) / (2u * major));
  if (x_major) {
    cx = ox + k * sx; cy = oy + j * sy; err = (ax - ay) - k * ay + j * ax;
  } else {
    cx = ox + j * sx; cy = oy + k * sy; err = (ax - ay) + k * ax - j * ay;
  }
}

// The first step of a walk at which its major coordinate lies in the grid's range, or `steps` where it never does: no cell
// before it is a cell of the grid, so the walk may start there -- a sensor far outside the grid costs no more than one inside,
// and what is left is at most the grid's extent along the major axis plus one step (the early exit below ends it).
__device__ inline int64_t occ_first_step(const OccRenderArgs & A, int64_t ox, int64_t oy, int64_t ax, int64_t ay, int64_t sx, int64_t sy, int64_t steps)
{
  const bool x_major = ax >= ay;
  const int64_t o = x_major ? ox : oy, s = x_major ? sx : sy, extent = (int64_t)(x_major ? A.width : A.height);
  int64_t k = 0;
  if (o < 0) {k = s > 0 ? -o : steps;} else if (o >= extent) {k = s < 0 ? o - (extent - 1) : steps;}
  return k < steps ? k : steps;
}

// grid (tiles of W, the chunk's scans): one thread per beam walks its line from the scan's origin cell to the beam's end
// cell and sets the bit of every cell of the grid it visits in the scan's bitmaps -- passed cells and the end of a CLEAR beam
// in free_bits, the end of a HIT beam in hit_bits.  The walk is a counted loop over max(ax, ay) + 1 cells; it starts at the
// first step whose major coordinate is in the grid's range (occ_first_step, occ_jump) and leaves once no later cell can lie
// in the grid (x and y are monotone): neither drops a cell, and a thread walks at most max(width, height) + 1 steps.
__global__ __launch_bounds__(kOccThreads) void occupancy_cast_kernel(const OccRenderArgs A)
{
  const uint32_t ls = blockIdx.y, k = A.first + ls;
  const uint32_t col = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t n_hit = 0, n_clear = 0, n_skipped = 0, n_miss = 0;
  if (col < A.W) {
    const uint4 beam = A.beams[(size_t)k * A.W + col];
    if (beam.w != kOccNone) {
      const double * m = A.poses + 12u * (size_t)k;
      const double x = (double)__uint_as_float(beam.x), y = (double)__uint_as_float(beam.y), z = (double)__uint_as_float(beam.z);
      const double wx = ((m[0] * x + m[1] * y) + m[2] * z) + m[3], wy = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
      int64_t ox = 0, oy = 0, ex = 0, ey = 0;
      const bool ok = occ_cell(m[3], A.origin_x, A.inv_res, ox) && occ_cell(m[7], A.origin_y, A.inv_res, oy) &&
        occ_cell(wx, A.origin_x, A.inv_res, ex) && occ_cell(wy, A.origin_y, A.inv_res, ey);
      if (!ok) {
        n_skipped = 1u;
      } else {
        const bool hit = beam.w == kOccHit;
        n_hit = hit ? 1u : 0u;
        n_clear = hit ? 0u : 1u;
        uint32_t * free_bits = A.free_bits + (size_t)ls * A.words, * hit_bits = A.hit_bits + (size_t)ls * A.words;
        const int64_t ax = ex > ox ? ex - ox : ox - ex, ay = ey > oy ? ey - oy : oy - ey;
        const int64_t sx = ex > ox ? 1 : (ex < ox ? -1 : 0), sy = ey > oy ? 1 : (ey < oy ? -1 : 0);
        const int64_t wx0 = ox - A.reach, wy0 = oy - A.reach;
        const int64_t steps = (ax > ay ? ax : ay) + 1;
        int64_t err = ax - ay, cx = ox, cy = oy;
        const int64_t first = occ_first_step(A, ox, oy, ax, ay, sx, sy, steps);
        occ_jump(ox, oy, ax, ay, sx, sy, first, cx, cy, err);
        for (int64_t step = first; step < steps; step++) {
          if (occ_in_grid(A, cx, cy)) {
            const int64_t lx = cx - wx0, ly = cy - wy0;
            if (lx < 0 || lx >= A.side || ly < 0 || ly >= A.side) {
              n_miss += 1u;
            } else {
              occ_set((step + 1 == steps && hit) ? hit_bits : free_bits, ly * A.side + lx);
            }
          } else if ((cx < 0 && sx <= 0) || (cx >= (int64_t)A.width && sx >= 0) || (cy < 0 && sy <= 0) || (cy >= (int64_t)A.height && sy >= 0)) {
            break;                                           // (outside and moving away, or not moving: nothing more in the grid)
          }
          const int64_t e2 = 2 * err;
          if (e2 > -ay) {err -= ay; cx += sx;}
          if (e2 < ax) {err += ax; cy += sy;}
        }
      }
    }
  }
  occ_count(A.counters + kOccHitBeams, n_hit);
  occ_count(A.counters + kOccClearBeams, n_clear);
  occ_count(A.counters + kOccSkippedBeams, n_skipped);
  occ_count(A.counters + kOccWindowMiss, n_miss);
}

// grid (tiles of words / 4, the chunk's scans): four words of both bitmaps per thread; the scan's votes -- OCCUPIED where a HIT
// beam ended, otherwise FREE where a beam passed or a CLEAR beam ended -- added to the cells' counts, and the words zeroed
// for the next chunk.  A scan with a set bit has finite origin cells (the cast checked them) and only cells of the grid were
// set; the fold checks the cell again all the same, so that no state of the bitmaps can make it write outside the counts.
__global__ __launch_bounds__(kOccThreads) void occupancy_fold_kernel(const OccRenderArgs A)
{
  const uint32_t ls = blockIdx.y, k = A.first + ls;
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;          // the group of four words
  uint32_t n_occupied = 0, n_free = 0;
  if (q < A.words / 4u) {
    uint4 * fp = reinterpret_cast<uint4 *>(A.free_bits + (size_t)ls * A.words) + q, * hp = reinterpret_cast<uint4 *>(A.hit_bits + (size_t)ls * A.words) + q;
    const uint4 f4 = *fp, h4 = *hp;
    if (f4.x | f4.y | f4.z | f4.w | h4.x | h4.y | h4.z | h4.w) {
      const double * m = A.poses + 12u * (size_t)k;
      int64_t ox = 0, oy = 0;
      (void)occ_cell(m[3], A.origin_x, A.inv_res, ox);
      (void)occ_cell(m[7], A.origin_y, A.inv_res, oy);
      const int64_t wx0 = ox - A.reach, wy0 = oy - A.reach;
      const uint32_t f[4] = {f4.x, f4.y, f4.z, f4.w}, h[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
      for (uint32_t w = 0; w < 4u; w++) {
        const int64_t bit0 = ((int64_t)q * 4 + w) * 32;
        uint32_t occupied = h[w], free_ = f[w] & ~h[w];
        n_occupied += (uint32_t)__popc(occupied);
        n_free += (uint32_t)__popc(free_);
        while (occupied) {
          const int64_t bit = bit0 + (__ffs((int)occupied) - 1);
          occupied &= occupied - 1u;
          const int64_t ly = bit / A.side, lx = bit - ly * A.side;
          if (occ_in_grid(A, wx0 + lx, wy0 + ly)) {atomicAdd(A.hits + (size_t)(wy0 + ly) * A.width + (size_t)(wx0 + lx), 1u);}
        }
        while (free_) {
          const int64_t bit = bit0 + (__ffs((int)free_) - 1);
          free_ &= free_ - 1u;
          const int64_t ly = bit / A.side, lx = bit - ly * A.side;
          if (occ_in_grid(A, wx0 + lx, wy0 + ly)) {atomicAdd(A.misses + (size_t)(wy0 + ly) * A.width + (size_t)(wx0 + lx), 1u);}
        }
      }
      *fp = make_uint4(0u, 0u, 0u, 0u);
      *hp = make_uint4(0u, 0u, 0u, 0u);
    }
  }
  occ_count(A.counters + kOccOccupiedVotes, n_occupied);
  occ_count(A.counters + kOccFreeVotes, n_free);
}

// --- emit -------------------------------------------------------------------------------------------------------------------
// four consecutive cells per thread
__global__ __launch_bounds__(kOccThreads) void occupancy_emit_kernel(const OccEmitArgs A)
{
  const uint64_t c0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4u;
  if (c0 >= A.cells) {return;}
  if (A.words && c0 + 4u <= A.cells) {
    uint32_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {v |= (uint32_t)(uint8_t)occ_value(A, c0 + j) << (8u * j);}
    *reinterpret_cast<uint32_t *>(A.out + c0) = v;
  } else {
    for (uint64_t c = c0; c < A.cells && c < c0 + 4u; c++) {A.out[c] = occ_value(A, c);}
  }
}

}  // namespace lfx
