// lfx_kernels_segment.hpp -- scan segmentation (include/lfx.h, the segmentation section; no reference counterpart, the model is
// LeGO-LOAM's image projection): every scan of a batch projected to an H x W range image from its input records, the
// ground labelled by the slope between vertically adjacent cells, the rest clustered by connected components under an
// angle test, and every record given the class and the label of its cell; then the feature clouds packed through a class
// mask.  The arithmetic is the header's, in double, unfused; the only atomics are integer minima, maxima and sums, so the
// same inputs give the same bytes whatever the schedule.  No workgroup waits for another one anywhere: the phases are
// launches of their own, and the hook loop retries its own atomicMin only.
#pragma once

#include "lfx_kernels_image.hpp"

#pragma clang fp contract(off)

namespace lfx
{

constexpr int kSegThreads = 256;
constexpr uint32_t kSegNoCell = 0xFFFFFFFFu;
constexpr uint64_t kSegEmpty = ~0ull;                   // a cell of the image no record has reached (as a double: a NaN)
// bits of a cell's flag word (the w of its float4)
constexpr uint32_t kSegOccupied = 1u, kSegGround = 2u;

// A call's table of doubles: lfx_segment_tables' values, [0, W) col_cos, [W, 2 W) col_sin, then sin and cos of the column
// step and sin and cos of the row step.
__host__ __device__ inline uint32_t seg_table_doubles(uint32_t W) {return 2u * W + 4u;}

struct SegmentArgs
{
  const uint8_t * pts;                  // the batch's input records
  Layout L;
  const uint32_t * scan_begin;          // [scans + 1] of the batch, in records
  const uint16_t * ring_slot;           // ring id -> slot, or nullptr: the id is the slot
  const double * table;                 // seg_table_doubles(W) doubles
  uint32_t first_scan;                  // the chunk's first scan; the image arrays below hold the chunk's scans only
  uint32_t H, W, max_rings;
  double min_range, max_range, ground_tan2, segment_tan;
  uint32_t ground_first, ground_last;
  uint32_t segment_min_points, small_min_points, small_min_rows;
  // per cell of the chunk, [chunk scans][H * W]
  uint64_t * image;                     // the least (float bits of r << 32 | record) until segment_cell_kernel, then the bits of the winner's r
  float4 * cell;                        // the winner's x, y, z and the cell's flag word
  uint32_t * parent;                    // union-find over the chunk's cells (an index into the chunk); kSegNoCell: not a node
  uint32_t * csize, * crowmax;          // at a root: cells of its component, their largest row
  // per record of the batch
  uint8_t * class_out;
  uint32_t * id_out;                    // or nullptr
  uint32_t * counts_out;                // [scans][4], zeroed in-stream ahead of the launch, or nullptr
};

// The cell of one record and its range, or kSegNoCell: the header's projection -- the gates and the column are the shared
// ones (lfx_kernels_image.hpp), the range comparison and the row (the record's ring slot) are its own.
template<bool XYZ16>
__device__ inline uint32_t seg_project(const SegmentArgs & A, const uint8_t * rec, float & x, float & y, float & z, double & r)
{
  load_xyz<XYZ16>(rec, A.L, x, y, z);
  uint32_t row = load_ring(rec + A.L.oring, A.L.rtype, A.L.be);
  if (A.ring_slot != nullptr) {row = row < 65536u ? A.ring_slot[row] : 0xFFFFu;}
  if (row >= A.H || row >= A.max_rings) {return kSegNoCell;}
  const double xd = (double)x, yd = (double)y;
  double xy2;
  if (!planar_range(xd, yd, (double)z, xy2, r)) {return kSegNoCell;}
  if (r < A.min_range || r >= A.max_range) {return kSegNoCell;}
  return row * A.W + azimuth_column(A.table, A.table + A.W, A.W, xd, yd, y >= 0.0f);
}

// grid (chunks, the chunk's scans) as scan_context_kernel's; a grid-stride walk over the scan's input records, each with a
// cell taking part in that cell's 64-bit minimum.  (float)r is positive, so its bits order as it does; equal floats go to
// the lower record.  XYZ16: the canonical records, read with one load.
template<bool XYZ16>
__global__ __launch_bounds__(kSegThreads) void segment_project_kernel(const SegmentArgs A)
{
  const uint32_t ls = blockIdx.y, s = A.first_scan + ls;
  const uint32_t b0 = A.scan_begin[s], n = A.scan_begin[s + 1] - b0;
  const uint8_t * base = A.pts + (size_t)b0 * A.L.step;
  unsigned long long * img = reinterpret_cast<unsigned long long *>(A.image) + (size_t)ls * A.H * A.W;
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
    float x, y, z;
    double r;
    const uint32_t cell = seg_project<XYZ16>(A, base + (size_t)k * A.L.step, x, y, z, r);
    if (cell == kSegNoCell) {continue;}
    atomicMin(&img[cell], ((unsigned long long)__float_as_uint((float)r) << 32) | (unsigned long long)k);
  }
}

// One thread per cell of the chunk: the winner's x, y, z fetched from its record and its r put in the key's place (an
// empty cell keeps its NaN), the statistics cleared.
__global__ __launch_bounds__(kSegThreads) void segment_cell_kernel(const SegmentArgs A, uint32_t total)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) {return;}
  const uint32_t cells = A.H * A.W;
  const uint64_t key = A.image[i];
  float4 v = make_float4(0.f, 0.f, 0.f, __uint_as_float(0u));
  if (key != kSegEmpty) {
    const uint32_t s = A.first_scan + i / cells;
    const uint8_t * rec = A.pts + ((size_t)A.scan_begin[s] + (uint32_t)key) * A.L.step;
    load_xyz<false>(rec, A.L, v.x, v.y, v.z);
    v.w = __uint_as_float(kSegOccupied);
    const double xd = (double)v.x, yd = (double)v.y, zd = (double)v.z;
    A.image[i] = (uint64_t)__double_as_longlong(sqrt((xd * xd + yd * yd) + zd * zd));
  }
  A.cell[i] = v;
  A.csize[i] = 0u;
  A.crowmax[i] = 0u;
}

__device__ inline bool seg_ground_pair(const float4 a, const float4 b, double g2)
{
  const double dx = (double)b.x - (double)a.x, dy = (double)b.y - (double)a.y, dz = (double)b.z - (double)a.z;
  return dz * dz <= g2 * (dx * dx + dy * dy);
}

// One thread per cell: ground if the pair with the row above or the pair with the row below passes the slope test (each
// cell decides for itself: nothing is written twice), and the union-find's first state -- a node is its own parent.
__global__ __launch_bounds__(kSegThreads) void segment_ground_kernel(const SegmentArgs A, uint32_t total)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) {return;}
  const uint32_t cells = A.H * A.W, in_scan = i % cells, row = in_scan / A.W;
  const float4 v = A.cell[i];
  uint32_t flags = __float_as_uint(v.w);
  if (flags & kSegOccupied) {
    bool ground = false;
    if (row >= A.ground_first && row < A.ground_last) {           // the pair (row, row + 1)
      const float4 o = A.cell[i + A.W];
      ground = (__float_as_uint(o.w) & kSegOccupied) && seg_ground_pair(v, o, A.ground_tan2);
    }
    if (!ground && row > A.ground_first && row <= A.ground_last) {   // the pair (row - 1, row)
      const float4 o = A.cell[i - A.W];
      ground = (__float_as_uint(o.w) & kSegOccupied) && seg_ground_pair(o, v, A.ground_tan2);
    }
    if (ground) {
      flags |= kSegGround;
      A.cell[i].w = __uint_as_float(flags);
    }
  }
  A.parent[i] = (flags & (kSegOccupied | kSegGround)) == kSegOccupied ? i : kSegNoCell;
}

// Parents change under a launch's feet, in other workgroups: read them past this CU's L1.  A parent only ever decreases
// and stays an ancestor, so an older value is still a valid step of the walk.
__device__ inline uint32_t seg_parent(const uint32_t * parent, uint32_t i) {return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);}
__device__ inline uint32_t seg_find(const uint32_t * parent, uint32_t i)
{
  for (;;) {
    const uint32_t p = seg_parent(parent, i);
    if (p == i) {return i;}
    i = p;
  }
}

// a and b into one tree.  The larger root is hooked under the smaller one with atomicMin: a root is its tree's least index
// at all times.  Where the atomic finds that the larger one had a parent already (another hook came first), that parent
// and the smaller root are what is left to join: the loop goes on with them.  Every retry follows a hook that some thread
// has completed, and a parent never rises: the loop ends.
__device__ inline void seg_union(uint32_t * parent, uint32_t a, uint32_t b)
{
  for (;;) {
    a = seg_find(parent, a);
    b = seg_find(parent, b);
    if (a == b) {return;}
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const uint32_t old = atomicMin(parent + hi, lo);
    if (old == hi) {return;}
    a = old; b = lo;
  }
}

__device__ inline bool seg_joined(double ra, double rb, double sin_a, double cos_a, double seg_tan)
{
  const double d1 = ra > rb ? ra : rb, d2 = ra > rb ? rb : ra;
  return d2 * sin_a > seg_tan * (d1 - d2 * cos_a);          // (an empty cell's r is a NaN: never)
}

// One thread per cell: its edge to the next column (the last column's goes round the seam to column 0) and its edge to the
// next row, each hooked where both ends are nodes and the angle test joins them.
__global__ __launch_bounds__(kSegThreads) void segment_hook_kernel(const SegmentArgs A, uint32_t total)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) {return;}
  if (A.parent[i] == kSegNoCell) {return;}                 // (written by the launch before: kSegNoCell or i, whoever hooks meanwhile)
  const uint32_t cells = A.H * A.W, in_scan = i % cells, row = in_scan / A.W, col = in_scan - row * A.W;
  const double * c = A.table + 2u * A.W;
  const double r = __longlong_as_double((long long)A.image[i]);
  const uint32_t right = col + 1u < A.W ? i + 1u : i + 1u - A.W;
  if ((__float_as_uint(A.cell[right].w) & (kSegOccupied | kSegGround)) == kSegOccupied &&
    seg_joined(r, __longlong_as_double((long long)A.image[right]), c[0], c[1], A.segment_tan))
  {
    seg_union(A.parent, i, right);
  }
  if (row + 1u < A.H) {
    const uint32_t down = i + A.W;
    if ((__float_as_uint(A.cell[down].w) & (kSegOccupied | kSegGround)) == kSegOccupied &&
      seg_joined(r, __longlong_as_double((long long)A.image[down]), c[2], c[3], A.segment_tan))
    {
      seg_union(A.parent, i, down);
    }
  }
}

// One thread per cell: its parent becomes its root (no hook runs beside this launch, so the root is final; a walk that
// passes a cell already flattened takes a shortcut to the same root).
__global__ __launch_bounds__(kSegThreads) void segment_flatten_kernel(const SegmentArgs A, uint32_t total)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) {return;}
  if (A.parent[i] == kSegNoCell) {return;}
  const uint32_t root = seg_find(A.parent, i);
  if (root != i) {__hip_atomic_store(A.parent + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);}
}

// One thread per cell: a component's size and largest row at its root (its least row is the root's own: the root is the
// component's least index).  Neighbouring lanes hold neighbouring columns, mostly of one component: the first lane of
// every run of equal roots adds for the run.
__global__ __launch_bounds__(kSegThreads) void segment_stats_kernel(const SegmentArgs A, uint32_t total)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t cells = A.H * A.W;
  const uint32_t root = i < total ? A.parent[i] : kSegNoCell;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t before = __shfl_up(root, 1);
  const bool head = lane == 0u || before != root;
  const unsigned long long heads = __ballot(head);
  if (root == kSegNoCell || !head) {return;}
  // the run reaches to the lane in front of the next head
  const unsigned long long above = lane == 63u ? 0ull : heads >> (lane + 1u);
  const uint32_t len = above ? (uint32_t)__builtin_ctzll(above) + 1u : 64u - lane;
  atomicAdd(A.csize + root, len);
  atomicMax(A.crowmax + root, ((i + len - 1u) % cells) / A.W);
}

// grid (chunks, the chunk's scans): every record of the scan gets the class of its cell and, for a cluster, its label;
// the scan's counts by class: a ballot per wave and class, one atomic per workgroup and class.
template<bool XYZ16>
__global__ __launch_bounds__(kSegThreads) void segment_record_kernel(const SegmentArgs A)
{
  __shared__ uint32_t tally[4];
  const uint32_t ls = blockIdx.y, s = A.first_scan + ls, cells = A.H * A.W;
  const uint32_t b0 = A.scan_begin[s], n = A.scan_begin[s + 1] - b0;
  if (blockIdx.x * blockDim.x >= n) {return;}              // (the whole workgroup)
  if (threadIdx.x < 4u) {tally[threadIdx.x] = 0u;}
  __syncthreads();
  const uint8_t * base = A.pts + (size_t)b0 * A.L.step;
  const size_t c0 = (size_t)ls * cells;
  uint32_t mine[4] = {0u, 0u, 0u, 0u};                      // lane 0 of each wave: its wave's records by class
  // (whole waves walk together so that every lane takes part in the ballots)
  for (uint32_t k0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); k0 < n; k0 += gridDim.x * blockDim.x) {
    const uint32_t k = k0 + (threadIdx.x & 63u);
    uint32_t cls = 4u, id = kSentinel;
    if (k < n) {
      float x, y, z;
      double r;
      const uint32_t cell = seg_project<XYZ16>(A, base + (size_t)k * A.L.step, x, y, z, r);
      cls = LFX_SEG_NONE;
      if (cell != kSegNoCell) {
        if (__float_as_uint(A.cell[c0 + cell].w) & kSegGround) {
          cls = LFX_SEG_GROUND;
        } else {
          const uint32_t root = A.parent[c0 + cell];
          const uint32_t size = A.csize[root], rows = A.crowmax[root] - (root % cells) / A.W + 1u;
          const bool segment = size >= A.segment_min_points || (size >= A.small_min_points && rows >= A.small_min_rows);
          cls = segment ? LFX_SEG_SEGMENT : LFX_SEG_CLUTTER;
          id = root % cells;
        }
      }
      A.class_out[(size_t)b0 + k] = (uint8_t)cls;
      if (A.id_out) {A.id_out[(size_t)b0 + k] = id;}
    }
    if (A.counts_out) {
#pragma unroll
      for (uint32_t t = 0; t < 4u; t++) {mine[t] += (uint32_t)__popcll(__ballot(cls == t));}
    }
  }
  if (!A.counts_out) {return;}
  if ((threadIdx.x & 63u) == 0u) {
    for (uint32_t t = 0; t < 4u; t++) {if (mine[t]) {atomicAdd(&tally[t], mine[t]);}}
  }
  __syncthreads();
  if (threadIdx.x < 4u && tally[threadIdx.x]) {atomicAdd(A.counts_out + (size_t)s * 4u + threadIdx.x, tally[threadIdx.x]);}
}

// ------------------------------------------------------------------------------------------
// lfx_pack_features_segmented: lfx_pack_features through a class mask.
struct SegmentPackArgs
{
  const uint32_t * scan_begin, * scan_info;
  const float4 * edge_pts, * surf_pts;
  const uint32_t * edge_idx, * surf_idx;            // a feature's original index within its scan
  const uint8_t * cls;                              // per input record, by scan_begin[s] + index
  uint32_t edge_mask, surf_mask, batch, capacity;
  uint32_t * counts;                                // [2][batch]: what the masks keep of every scan's clouds
  uint32_t * offsets;                               // [2][batch + 1]
  float4 * edge_out, * surf_out;
};

__device__ inline bool seg_kept(const SegmentPackArgs & A, bool edge, size_t b, uint32_t k)
{
  const uint32_t orig = edge ? A.edge_idx[b + k] : A.surf_idx[b + k];
  return ((edge ? A.edge_mask : A.surf_mask) >> A.cls[b + orig]) & 1u;
}

// grid (2, batch): the records the mask keeps of one cloud of one scan
__global__ __launch_bounds__(kSegThreads) void segment_pack_count_kernel(const SegmentPackArgs A)
{
  __shared__ uint32_t total;
  const bool edge = blockIdx.x == 0u;
  const uint32_t s = blockIdx.y;
  const uint32_t n = A.scan_info[s * 4u + (edge ? kInfoEdge : kInfoSurface)];
  const size_t b = A.scan_begin[s];
  if (threadIdx.x == 0u) {total = 0u;}
  __syncthreads();
  uint32_t mine = 0;
  for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) {mine += seg_kept(A, edge, b, k) ? 1u : 0u;}
  for (int d = 32; d; d >>= 1) {mine += __shfl_down(mine, d);}
  if ((threadIdx.x & 63u) == 0u && mine) {atomicAdd(&total, mine);}
  __syncthreads();
  if (threadIdx.x == 0u) {A.counts[blockIdx.x * A.batch + s] = total;}
}

// grid (2, batch): one workgroup carries one cloud of one scan across in order, 256 records at a time -- a record's place
// is the scan's offset, what the tiles before kept and what the lanes and waves in front of it keep.
__global__ __launch_bounds__(kSegThreads) void segment_pack_kernel(const SegmentPackArgs A)
{
  __shared__ uint32_t wave_kept[kSegThreads / 64];
  const bool edge = blockIdx.x == 0u;
  const uint32_t s = blockIdx.y;
  const uint32_t n = A.scan_info[s * 4u + (edge ? kInfoEdge : kInfoSurface)];
  const size_t b = A.scan_begin[s];
  const float4 * src = edge ? A.edge_pts : A.surf_pts;
  float4 * dst = edge ? A.edge_out : A.surf_out;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t at = A.offsets[edge ? s : A.batch + 1u + s];
  for (uint32_t k0 = 0; k0 < n; k0 += blockDim.x) {
    const uint32_t k = k0 + threadIdx.x;
    const bool keep = k < n && seg_kept(A, edge, b, k);
    const unsigned long long kept = __ballot(keep);
    if (lane == 0u) {wave_kept[wave] = (uint32_t)__popcll(kept);}
    __syncthreads();
    uint32_t front = 0, all = 0;
    for (uint32_t w = 0; w < kSegThreads / 64; w++) {
      const uint32_t c = wave_kept[w];
      front += w < wave ? c : 0u;
      all += c;
    }
    const uint32_t to = at + front + (uint32_t)__popcll(kept & ((1ull << lane) - 1ull));
    if (keep && to < A.capacity) {dst[to] = src[b + k];}
    at += all;
    __syncthreads();                                       // (wave_kept is rewritten by the next tile)
  }
}

}  // namespace lfx
