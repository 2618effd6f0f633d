// lfx_kernels_gridmatch.hpp -- scan matching in occupancy grids (include/lfx.h, the grid-match section; no reference
// counterpart, the models are AMCL's likelihood field and the correlative scan matcher).  A score field S (uint16 per cell, a
// table look-up of the distance field's d2), every scan's HIT beams levelled to 2-D points once, and two gathers over them:
// arbitrary candidate poses (lanes along candidates) and an exhaustive window of whole-cell shifts and headings (lanes along
// ix, a few iy per thread, a (scan, heading)'s base cells in LDS).  The only floating point is the candidate arithmetic of a
// point's cell, double and unfused; every sum and every maximum is an integer, and no workgroup waits for another one: the
// same field, scans and candidates give the same bytes whatever the schedule.
#pragma once

#include "lfx_kernels_common.hpp"

#pragma clang fp contract(off)

namespace lfx
{

constexpr int kGmThreads = 256;
constexpr uint32_t kGmFar = 0xFFFFFFFFu;       // LFX_DISTANCE_FAR
constexpr uint32_t kGmHit = 1u;                // LFX_OCCUPANCY_HIT
constexpr uint32_t kGmMaxTable = 64u * 64u + 1u;
constexpr double kGmCellLimit = 1073741824.0;  // 2^30: a cell coordinate is below it in size
constexpr uint32_t kGmTileX = 64;              // a search workgroup's tile of candidates: a wave's lanes along ix ...
constexpr uint32_t kGmRows = 4;                // ... iy per thread ...
constexpr uint32_t kGmTileY = kGmRows * (kGmThreads / 64);   // ... and its four waves one above the other
constexpr uint32_t kGmScoreChunk = 1024;       // points of a scan the score kernel holds in LDS at once
constexpr uint32_t kGmFieldBlocks = 2048;      // the field kernel's grid at most: a workgroup's table serves many cells

struct GmGeom
{
  double origin_x, origin_y, inv_res;
  uint32_t W, H;
};

// floor((w - origin) * inv_res) as a cell coordinate: false where it is not finite or not below 2^30 in size
__device__ inline bool gm_axis(double w, double origin, double inv_res, int32_t & out)
{
  const double c = floor((w - origin) * inv_res);
  if (!(fabs(c) < kGmCellLimit)) {return false;}
  out = (int32_t)c;
  return true;
}

// the cell of point (px, py) under candidate (tx, ty, c, s); false: OUTSIDE by the size rule
__device__ inline bool gm_cell(const GmGeom & G, double px, double py, double c, double s, double tx, double ty, int32_t & ex, int32_t & ey)
{
  const double wx = (c * px - s * py) + tx;
  const double wy = (s * px + c * py) + ty;
  const bool okx = gm_axis(wx, G.origin_x, G.inv_res, ex);
  const bool oky = gm_axis(wy, G.origin_y, G.inv_res, ey);
  return okx && oky;
}

__device__ inline bool gm_in_grid(const GmGeom & G, int32_t x, int32_t y)
{
  return x >= 0 && x < (int32_t)G.W && y >= 0 && y < (int32_t)G.H;
}

// --- the field --------------------------------------------------------------------------------------------------------------
struct GmFieldArgs
{
  const uint32_t * d2;                  // [H][W]
  const uint16_t * lut;                 // [n]
  uint32_t n;
  uint64_t cells;
  uint16_t * S;                         // [H][W]
};

__device__ inline uint32_t gm_value(const uint16_t * lut, uint32_t n, uint32_t d2)
{
  return d2 < n ? (uint32_t)lut[d2] : 0u;          // (FAR is above every n)
}

// A stream: 4 B in, 2 B out, four cells per thread and step; the table (at most 8 KB and two bytes) in LDS.
__global__ __launch_bounds__(kGmThreads) void gridmatch_field_kernel(GmFieldArgs A)
{
  __shared__ uint16_t lut[kGmMaxTable + 1u];
  for (uint32_t i = threadIdx.x; i < A.n; i += kGmThreads) {lut[i] = A.lut[i];}
  __syncthreads();
  const uint64_t quads = (A.cells + 3u) / 4u;
  for (uint64_t q = (uint64_t)blockIdx.x * kGmThreads + threadIdx.x; q < quads; q += (uint64_t)gridDim.x * kGmThreads) {
    const uint64_t first = 4u * q;
    if (first + 4u <= A.cells) {
      const uint4 d = reinterpret_cast<const uint4 *>(A.d2)[q];
      uint2 o;
      o.x = gm_value(lut, A.n, d.x) | (gm_value(lut, A.n, d.y) << 16);
      o.y = gm_value(lut, A.n, d.z) | (gm_value(lut, A.n, d.w) << 16);
      reinterpret_cast<uint2 *>(A.S)[q] = o;
    } else {
      for (uint64_t i = first; i < A.cells; i++) {A.S[i] = (uint16_t)gm_value(lut, A.n, A.d2[i]);}
    }
  }
}

// --- the scans --------------------------------------------------------------------------------------------------------------
struct GmScanArgs
{
  const uint4 * beams;                  // [scans][W]: x, y, z and the kind's bits
  uint32_t W;
  const double * lev;                   // null: identity; else scan s's rows 0 and 1 at lev + s * lev_stride and + row_stride
  uint32_t lev_stride, row_stride;      // ([.][9] levels: 9, 3; [.][12] poses: 12, 4)
  double2 * points;                     // [max_scans][max_beams]
  uint32_t * n_points;                  // [max_scans]
  uint32_t max_beams;
};

// One workgroup per scan: the HIT beams levelled and kept in beam order (a ballot per wave, the waves' counts through LDS).
__global__ __launch_bounds__(kGmThreads) void gridmatch_scans_kernel(GmScanArgs A)
{
  __shared__ uint32_t wave_n[kGmThreads / 64];
  const uint32_t s = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  double l0 = 1.0, l1 = 0.0, l2 = 0.0, l3 = 0.0, l4 = 1.0, l5 = 0.0;
  if (A.lev) {
    const double * L = A.lev + (size_t)s * A.lev_stride;
    l0 = L[0]; l1 = L[1]; l2 = L[2];
    l3 = L[A.row_stride]; l4 = L[A.row_stride + 1u]; l5 = L[A.row_stride + 2u];
  }
  double2 * out = A.points + (size_t)s * A.max_beams;
  uint32_t base = 0;
  for (uint32_t b0 = 0; b0 < A.W; b0 += kGmThreads) {
    const uint32_t i = b0 + threadIdx.x;
    bool keep = false;
    double px = 0.0, py = 0.0;
    if (i < A.W) {
      const uint4 b = A.beams[(size_t)s * A.W + i];
      if (b.w == kGmHit) {
        const double x = (double)__uint_as_float(b.x), y = (double)__uint_as_float(b.y), z = (double)__uint_as_float(b.z);
        px = (l0 * x + l1 * y) + l2 * z;
        py = (l3 * x + l4 * y) + l5 * z;
        keep = isfinite(px) && isfinite(py);
      }
    }
    const unsigned long long mask = __ballot(keep);
    if (lane == 0u) {wave_n[wave] = (uint32_t)__popcll(mask);}
    __syncthreads();
    uint32_t at = base, total = 0;
    for (uint32_t w = 0; w < kGmThreads / 64; w++) {
      if (w < wave) {at += wave_n[w];}
      total += wave_n[w];
    }
    if (keep) {out[at + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = make_double2(px, py);}
    base += total;
    __syncthreads();
  }
  if (threadIdx.x == 0u) {A.n_points[s] = base;}
}

// --- score ------------------------------------------------------------------------------------------------------------------
struct GmScoreArgs
{
  GmGeom G;
  const uint16_t * S;
  const double2 * points;               // the scan's
  const uint32_t * n_points;            // the scan's count
  const double * cand;                  // [P][4]: tx, ty, c, s
  uint32_t P;
  uint32_t * score, * inside;           // [P]; inside may be null
};

// Lanes along candidates, the scan's points through LDS a chunk at a time: every lane reads the same point (a broadcast) and
// gathers its own cell -- scattered by nature.
__global__ __launch_bounds__(kGmThreads) void gridmatch_score_kernel(GmScoreArgs A)
{
  __shared__ double2 pts[kGmScoreChunk];
  const uint32_t p = blockIdx.x * kGmThreads + threadIdx.x;
  const bool valid = p < A.P;
  double tx = 0.0, ty = 0.0, c = 1.0, s = 0.0;
  if (valid) {
    const double2 a = reinterpret_cast<const double2 *>(A.cand)[2u * (size_t)p], b = reinterpret_cast<const double2 *>(A.cand)[2u * (size_t)p + 1u];
    tx = a.x; ty = a.y; c = b.x; s = b.y;
  }
  const uint32_t n = *A.n_points;
  uint32_t sum = 0, in = 0;
  for (uint32_t b0 = 0; b0 < n; b0 += kGmScoreChunk) {
    const uint32_t m = min(kGmScoreChunk, n - b0);
    for (uint32_t i = threadIdx.x; i < m; i += kGmThreads) {pts[i] = A.points[b0 + i];}
    __syncthreads();
    if (valid) {
      for (uint32_t i = 0; i < m; i++) {
        const double2 q = pts[i];
        int32_t ex, ey;
        if (gm_cell(A.G, q.x, q.y, c, s, tx, ty, ex, ey) && gm_in_grid(A.G, ex, ey)) {
          sum += A.S[(uint32_t)ey * A.G.W + (uint32_t)ex];
          in++;
        }
      }
    }
    __syncthreads();
  }
  if (valid) {
    A.score[p] = sum;
    if (A.inside) {A.inside[p] = in;}
  }
}

// --- search -----------------------------------------------------------------------------------------------------------------
struct GmSearchArgs
{
  GmGeom G;
  const uint16_t * S;
  const double2 * points;               // [max_scans][max_beams]
  const uint32_t * n_points;            // [max_scans]
  uint32_t max_beams, first;            // the call's scan k is the object's scan first + k
  const double * rot;                   // [scans][T][2]: cos, sin
  const double * centres;               // [scans][2]: x0, y0
  uint32_t Nx, Ny, T, half_x, half_y, step;
  uint32_t tiles_x;                     // tiles of kGmTileX candidates along ix
  unsigned long long * slice_key;       // [scans][T]: the greatest (score << 32) | ~index of the heading, 0 before
  uint32_t * volume;                    // [scans][T][Ny][Nx] or null
  uint32_t * best, * slice_best;        // the best kernel's outputs: [scans][4], [scans][T][2] or null
};

__device__ inline unsigned long long gm_key(uint32_t score, uint32_t index) {return ((unsigned long long)score << 32) | (unsigned long long)(~index);}

// One workgroup per (tile of 64 x 16 candidates, heading, scan).  Head: the scan's base cells under this heading, shifted to
// the tile's first candidate and sorted into LDS by what the tile can do to them -- points no candidate of the tile brings into
// the grid are dropped, points every candidate keeps inside go to the front as one linear index (the common case: no bounds
// check in their loop), the rest to the back as (x, y).  The lists' order is whatever the LDS atomics gave: the sums are
// integers.  Body: a thread owns one ix and kGmRows iy, so a wave's loads for a point are 64 * step consecutive uint16 of a
// row of S, kGmRows times, off one LDS broadcast.  Threads past the window's edge repeat its last candidate and write nothing.
__global__ __launch_bounds__(kGmThreads) void gridmatch_search_kernel(GmSearchArgs A)
{
  extern __shared__ int2 gm_cells[];                 // [the scan's points]
  __shared__ uint32_t n_fast, n_slow;
  __shared__ unsigned long long wave_key[kGmThreads / 64];
  const uint32_t scan = blockIdx.z, j = blockIdx.y;
  const uint32_t ix0 = (blockIdx.x % A.tiles_x) * kGmTileX, iy0 = (blockIdx.x / A.tiles_x) * kGmTileY;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t n = A.n_points[A.first + scan];
  const double2 * pts = A.points + (size_t)(A.first + scan) * A.max_beams;
  const double c = A.rot[2u * ((size_t)scan * A.T + j)], s = A.rot[2u * ((size_t)scan * A.T + j) + 1u];
  const double x0 = A.centres[2u * (size_t)scan], y0 = A.centres[2u * (size_t)scan + 1u];
  const int32_t W = (int32_t)A.G.W, H = (int32_t)A.G.H, step = (int32_t)A.step;
  // the tile's first candidate's shift, and how far its valid candidates reach beyond it
  const int32_t shift_x = ((int32_t)ix0 - (int32_t)A.half_x) * step, shift_y = ((int32_t)iy0 - (int32_t)A.half_y) * step;
  const int32_t span_x = (int32_t)(min(kGmTileX, A.Nx - ix0) - 1u) * step, span_y = (int32_t)(min(kGmTileY, A.Ny - iy0) - 1u) * step;
  if (threadIdx.x == 0u) {n_fast = 0u; n_slow = 0u;}
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n; i += kGmThreads) {
    const double2 q = pts[i];
    int32_t bx, by;
    if (!gm_cell(A.G, q.x, q.y, c, s, x0, y0, bx, by)) {continue;}
    const int32_t cx = bx + shift_x, cy = by + shift_y;       // (below 2^30 + 2^13 in size)
    if (cx + span_x < 0 || cx >= W || cy + span_y < 0 || cy >= H) {continue;}
    if (cx >= 0 && cx + span_x < W && cy >= 0 && cy + span_y < H) {
      gm_cells[atomicAdd(&n_fast, 1u)] = make_int2(cy * W + cx, 0);
    } else {
      gm_cells[n - 1u - atomicAdd(&n_slow, 1u)] = make_int2(cx, cy);
    }
  }
  __syncthreads();
  const uint32_t fast = n_fast, slow = n_slow;
  const uint32_t ix = min(ix0 + lane, A.Nx - 1u);
  const int32_t dx = (int32_t)(ix - ix0) * step;
  uint32_t iy[kGmRows], acc[kGmRows];
  int32_t dy[kGmRows], lin[kGmRows];
#pragma unroll
  for (uint32_t r = 0; r < kGmRows; r++) {
    iy[r] = min(iy0 + wave * kGmRows + r, A.Ny - 1u);
    dy[r] = (int32_t)(iy[r] - iy0) * step;
    lin[r] = dy[r] * W + dx;
    acc[r] = 0u;
  }
#pragma unroll 4
  for (uint32_t k = 0; k < fast; k++) {
    const int32_t at = gm_cells[k].x;
#pragma unroll
    for (uint32_t r = 0; r < kGmRows; r++) {acc[r] += A.S[at + lin[r]];}
  }
  for (uint32_t k = 0; k < slow; k++) {
    const int2 cell = gm_cells[n - 1u - k];
    const int32_t x = cell.x + dx;
    if (x < 0 || x >= W) {continue;}
#pragma unroll
    for (uint32_t r = 0; r < kGmRows; r++) {
      const int32_t y = cell.y + dy[r];
      if (y >= 0 && y < H) {acc[r] += A.S[y * W + x];}
    }
  }
  unsigned long long key = 0ull;
  if (ix0 + lane < A.Nx) {
#pragma unroll
    for (uint32_t r = 0; r < kGmRows; r++) {
      if (iy0 + wave * kGmRows + r < A.Ny) {
        const uint32_t index = (j * A.Ny + iy[r]) * A.Nx + ix;
        if (A.volume) {A.volume[(size_t)scan * A.T * A.Ny * A.Nx + index] = acc[r];}
        key = max(key, gm_key(acc[r], index));
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {key = max(key, (unsigned long long)__shfl_xor((long long)key, off));}
  if (lane == 0u) {wave_key[wave] = key;}
  __syncthreads();
  if (threadIdx.x == 0u) {
    for (uint32_t w = 1; w < kGmThreads / 64; w++) {key = max(key, wave_key[w]);}
    atomicMax(&A.slice_key[(size_t)scan * A.T + j], key);
  }
}

// One workgroup per scan: the headings' keys to slice_best and their maximum to best, with the points the best candidate has
// inside the grid counted here, once, instead of beside every candidate's score.
__global__ __launch_bounds__(kGmThreads) void gridmatch_best_kernel(GmSearchArgs A)
{
  __shared__ unsigned long long keys[kGmThreads];
  __shared__ uint32_t counts[kGmThreads];
  const uint32_t scan = blockIdx.x;
  unsigned long long key = 0ull;
  for (uint32_t j = threadIdx.x; j < A.T; j += kGmThreads) {
    const unsigned long long k = A.slice_key[(size_t)scan * A.T + j];
    if (A.slice_best) {
      A.slice_best[2u * ((size_t)scan * A.T + j)] = (uint32_t)(k >> 32);
      A.slice_best[2u * ((size_t)scan * A.T + j) + 1u] = ~(uint32_t)k;
    }
    key = max(key, k);
  }
  keys[threadIdx.x] = key;
  __syncthreads();
  for (uint32_t half = kGmThreads / 2; half > 0u; half >>= 1) {
    if (threadIdx.x < half) {keys[threadIdx.x] = max(keys[threadIdx.x], keys[threadIdx.x + half]);}
    __syncthreads();
  }
  key = keys[0];
  // (every heading's key has been raised by at least one candidate; a key still 0 would decode to no candidate at all)
  const uint32_t score = (uint32_t)(key >> 32), index = key ? ~(uint32_t)key : 0u;
  const uint32_t ix = index % A.Nx, iy = (index / A.Nx) % A.Ny, j = index / (A.Nx * A.Ny);
  const int32_t shift_x = ((int32_t)ix - (int32_t)A.half_x) * (int32_t)A.step, shift_y = ((int32_t)iy - (int32_t)A.half_y) * (int32_t)A.step;
  const uint32_t n = A.n_points[A.first + scan];
  const double2 * pts = A.points + (size_t)(A.first + scan) * A.max_beams;
  const double c = A.rot[2u * ((size_t)scan * A.T + j)], s = A.rot[2u * ((size_t)scan * A.T + j) + 1u];
  const double x0 = A.centres[2u * (size_t)scan], y0 = A.centres[2u * (size_t)scan + 1u];
  uint32_t in = 0;
  for (uint32_t i = threadIdx.x; i < n; i += kGmThreads) {
    const double2 q = pts[i];
    int32_t bx, by;
    if (gm_cell(A.G, q.x, q.y, c, s, x0, y0, bx, by) && gm_in_grid(A.G, bx + shift_x, by + shift_y)) {in++;}
  }
  counts[threadIdx.x] = in;
  __syncthreads();
  for (uint32_t half = kGmThreads / 2; half > 0u; half >>= 1) {
    if (threadIdx.x < half) {counts[threadIdx.x] += counts[threadIdx.x + half];}
    __syncthreads();
  }
  if (threadIdx.x == 0u) {
    uint32_t * out = A.best + 4u * (size_t)scan;
    out[0] = score; out[1] = index; out[2] = counts[0]; out[3] = n;
  }
}

}  // namespace lfx
