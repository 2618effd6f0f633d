// lfx_kernels_place.hpp -- place recognition (include/lfx.h, the place recognition section; no reference counterpart, the
// model is Scan Context): the descriptor of every scan of a batch from its input records, and the brute-force comparison of
// query descriptors with the entries of a place index under every column shift -- of every entry of a range, or of the
// entries a gate per query leaves eligible (a limit and a distance between poses, decided on the device).  The arithmetic
// is the header's, in double, unfused where a fused form would give other bits; every sum runs in a fixed order, the
// gate's lists are written in a fixed order and the only atomics are integer maxima, so the same inputs give the same bytes.
#pragma once

#include "lfx_kernels_image.hpp"

#pragma clang fp contract(off)

namespace lfx
{

constexpr int kPlaceThreads = 256;
constexpr int kScMaxRings = LFX_SCAN_CONTEXT_MAX_RINGS, kScMaxSectors = LFX_SCAN_CONTEXT_MAX_SECTORS;
constexpr int kScMaxCells = kScMaxRings * kScMaxSectors;             // 4 800 cells: 19 KB of keys

// A call's table of doubles (lfx_scan_context_tables' values, then the square of min_radius):
// [0, S) sector_cos, [S, 2 S) sector_sin, [2 S, 2 S + R + 1) ring_r2, [2 S + R + 1] min_radius^2
__host__ __device__ inline uint32_t sc_table_doubles(uint32_t R, uint32_t S) {return 2u * S + R + 2u;}

struct ScanContextArgs
{
  const uint8_t * pts;                  // the batch's input records
  Layout L;
  const uint32_t * scan_begin;          // [scans + 1], in records
  const double * table;                 // sc_table_doubles(R, S) doubles
  uint32_t * keys;                      // [scans][R * S], zeroed in-stream ahead of the launch
  uint32_t R, S;
};

// grid (chunks, scans) as deskew_kernel's; a grid-stride walk over the scan's input records.  A workgroup keeps one array
// of cells in LDS, each the largest float_order(z) of its records (0: no record -- no float has that key), filled with LDS
// integer max; its non-empty cells then go to the scan's keys with a global integer max.  XYZ16: load_xyz's
// (lfx_kernels_image.hpp).  The sector is the COUNT of the half's directions the record has passed (include/lfx.h: the
// counts are the definition), not azimuth_column's search.
template<bool XYZ16>
__global__ __launch_bounds__(kPlaceThreads) void scan_context_kernel(const ScanContextArgs A)
{
  __shared__ uint32_t cell[kScMaxCells];
  __shared__ double tab[2 * kScMaxSectors + kScMaxRings + 2];
  const uint32_t s = blockIdx.y, R = A.R, S = A.S, cells = R * S;
  const uint32_t b0 = A.scan_begin[s], n = A.scan_begin[s + 1] - b0;
  if (blockIdx.x * blockDim.x >= n) {return;}            // (the whole workgroup: no record, nothing to flush)
  for (uint32_t i = threadIdx.x; i < cells; i += blockDim.x) {cell[i] = 0u;}
  for (uint32_t i = threadIdx.x; i < sc_table_doubles(R, S); i += blockDim.x) {tab[i] = A.table[i];}
  __syncthreads();
  const double * cs = tab, * sn = tab + S, * r2tab = tab + 2u * S;
  const double min_r2 = r2tab[R + 1u], max_r2 = r2tab[R];
  const uint32_t half = S / 2u;
  const uint8_t * base = A.pts + (size_t)b0 * A.L.step;
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
    const uint8_t * rec = base + (size_t)k * A.L.step;
    float x, y, z;
    load_xyz<XYZ16>(rec, A.L, x, y, z);
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) {continue;}
    const double xd = (double)x, yd = (double)y;
    const double r2 = xd * xd + yd * yd;
    if (r2 < min_r2 || r2 >= max_r2) {continue;}
    uint32_t ring = 0;
    for (uint32_t j = 1; j < R; j++) {ring += r2 >= r2tab[j] ? 1u : 0u;}
    // the half of the circle the record lies in, then the sectors of that half whose first direction it has passed
    const uint32_t m0 = y >= 0.0f ? half : 0u;
    uint32_t sector = m0;
    for (uint32_t i = 1; i < half; i++) {
      const double cross = cs[m0 + i] * yd - sn[m0 + i] * xd;
      sector += cross >= 0.0 ? 1u : 0u;
    }
    atomicMax(&cell[ring * S + sector], float_order(z));
  }
  __syncthreads();
  uint32_t * out = A.keys + (size_t)s * cells;
  for (uint32_t i = threadIdx.x; i < cells; i += blockDim.x) {
    const uint32_t key = cell[i];
    if (key) {atomicMax(&out[i], key);}
  }
}

// keys -> the caller's floats, every cell of every scan: v = zmax + sensor_height where v > 0, else +0.0f
__global__ __launch_bounds__(kPlaceThreads) void scan_context_finish_kernel(const uint32_t * keys, float * out, size_t total, float sensor_height)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) {return;}
  const uint32_t key = keys[i];
  float v = 0.0f;
  if (key) {
    const float zmax = __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
    const float t = zmax + sensor_height;
    v = t > 0.0f ? t : 0.0f;
  }
  out[i] = v;
}

// The column norms of n descriptors ([n][R][S] floats): norms[e][j] = sqrt(sum_i d[e][i][j]^2), i ascending, in double
// (the squares of floats are exact there; sqrt is correctly rounded).  One thread per column.
__global__ __launch_bounds__(kPlaceThreads) void place_norms_kernel(const float * desc, double * norms, uint32_t n, uint32_t R, uint32_t S)
{
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)n * S) {return;}
  const size_t e = t / S;
  const uint32_t j = (uint32_t)(t - e * S);
  const float * d = desc + e * R * S + j;
  double sum = 0.0;
  for (uint32_t i = 0; i < R; i++) {
    const double v = (double)d[(size_t)i * S];
    sum = fma(v, v, sum);                                // (exact product: the fused form rounds as the unfused one)
  }
  norms[t] = sqrt(sum);
}

struct PlaceCompareArgs
{
  const float * query;                  // [queries][R][S]
  const double * query_norms;           // [queries][S]
  const float * entries;                // the range's first entry: [count][R][S]
  const double * entry_norms;           // [count][S]
  double * best_distance;               // [queries][count]
  uint32_t * best_shift;                // [queries][count]
  uint32_t count, R, S;
  uint32_t tile;                        // entries per workgroup: place_tile()
};

constexpr uint32_t kPlaceTile = 64;     // entries per workgroup, at most
// LDS of place_compare_kernel in bytes: the query in double, its norms, one pass of entries in float with their norms, the
// pass's distances
__host__ __device__ inline uint32_t place_pass_entries(uint32_t S) {return (uint32_t)kPlaceThreads / S;}
// Entries per workgroup for `pairs` (query, entry) pairs: whole passes, at most kPlaceTile entries, and few enough that a
// small index still spreads over the device (a pass is a chain of dependent sums: one workgroup alone takes its time)
__host__ __device__ inline uint32_t place_tile(uint32_t S, size_t pairs)
{
  const uint32_t epp = place_pass_entries(S);
  const size_t passes = pairs / ((size_t)epp * 2048u);
  const uint32_t most = kPlaceTile / epp ? kPlaceTile / epp : 1u;
  return epp * (uint32_t)(passes < 1u ? 1u : (passes > most ? most : passes));
}
__host__ __device__ inline size_t place_compare_lds(uint32_t R, uint32_t S)
{
  const size_t epp = place_pass_entries(S);
  return sizeof(double) * ((size_t)R * S + S + epp * S + epp * S) + sizeof(float) * epp * R * S;
}

// One (query, tile) of the comparison, the one copy of the shift-distance routine: place_compare_kernel hands it a tile of
// the range's entries, place_compare_gated_kernel (GATED) a tile of the query's list, whose slot l is entry A.list[l].  The
// query is staged in LDS (in double, with its norms) where `stage` says so -- once per workgroup: a workgroup that takes
// several tiles stages with its first -- and the tile's entries follow in passes of floor(256 / S) entries,
// S threads to an entry, one per shift: a thread walks the columns j ascending and, per column, the rings i ascending -- the
// order of the header -- reading the query's value as a broadcast and the entry's along a row, neighbouring shifts from
// neighbouring banks.  The entry's least d(s) and the lowest s that reaches it are picked by one thread walking the S
// distances in LDS in ascending s.  The results go to [query][stride] at the tile's own positions.  No atomics.
template<bool GATED>
__device__ __forceinline__ void place_compare_tile(const PlaceCompareArgs & A, const uint32_t * list, uint32_t stride, uint32_t query,
  uint32_t tile0, uint32_t tile1, bool stage)
{
  extern __shared__ double place_lds[];
  const uint32_t R = A.R, S = A.S, cells = R * S, epp = place_pass_entries(S);
  double * q = place_lds, * nq = q + cells, * nc = nq + S, * dist = nc + (size_t)epp * S;
  float * ent = reinterpret_cast<float *>(dist + (size_t)epp * S);
  if (stage) {
    const float * qg = A.query + (size_t)query * cells;
    for (uint32_t i = threadIdx.x; i < cells; i += blockDim.x) {q[i] = (double)qg[i];}
    for (uint32_t i = threadIdx.x; i < S; i += blockDim.x) {nq[i] = A.query_norms[(size_t)query * S + i];}
  }
  const uint32_t le = threadIdx.x / S, shift = threadIdx.x - le * S;     // (threads past epp * S stage, and wait)
  for (uint32_t e0 = tile0; e0 < tile1; e0 += epp) {
    const uint32_t ne = min(epp, tile1 - e0);
    __syncthreads();                                     // (the pass before has been read; the query is staged)
    if (GATED) {
      // (a pass's entries lie anywhere in the index: one entry after the other, each read along its cells)
      for (uint32_t l = 0; l < ne; l++) {
        const size_t e = list[e0 + l];
        const float * eg = A.entries + e * cells;
        for (uint32_t i = threadIdx.x; i < cells; i += blockDim.x) {ent[(size_t)l * cells + i] = eg[i];}
        for (uint32_t i = threadIdx.x; i < S; i += blockDim.x) {nc[(size_t)l * S + i] = A.entry_norms[e * S + i];}
      }
    } else {
      const float * eg = A.entries + (size_t)e0 * cells;
      for (uint32_t i = threadIdx.x; i < ne * cells; i += blockDim.x) {ent[i] = eg[i];}
      for (uint32_t i = threadIdx.x; i < ne * S; i += blockDim.x) {nc[i] = A.entry_norms[(size_t)e0 * S + i];}
    }
    __syncthreads();
    if (le < ne) {
      const float * c = ent + (size_t)le * cells;
      const double * ncl = nc + (size_t)le * S;
      double sum = 0.0;
      uint32_t valid = 0;
      for (uint32_t j = 0; j < S; j++) {
        uint32_t col = j + shift;
        col = col >= S ? col - S : col;
        const double a = nq[j], b = ncl[col];
        if (a > 0.0 && b > 0.0) {
          double g = 0.0;
#pragma unroll 4
          for (uint32_t i = 0; i < R; i++) {g = fma(q[i * S + j], (double)c[i * S + col], g);}   // (exact products)
          sum += g / (a * b);
          valid++;
        }
      }
      dist[le * S + shift] = valid ? 1.0 - sum / (double)valid : 1.0;
    }
    __syncthreads();
    if (threadIdx.x < ne) {
      const double * d = dist + (size_t)threadIdx.x * S;
      double best = d[0];
      uint32_t at = 0;
      for (uint32_t sft = 1; sft < S; sft++) {
        // (a NaN distance is never less; a NaN in front stays: such an entry is never a match)
        if (d[sft] < best) {best = d[sft]; at = sft;}
      }
      const size_t o = (size_t)query * stride + e0 + threadIdx.x;
      A.best_distance[o] = best;
      A.best_shift[o] = at;
    }
  }
}

// grid (tiles of A.tile entries, queries): every entry of the range [A.entries, + A.count)
__global__ __launch_bounds__(kPlaceThreads) void place_compare_kernel(const PlaceCompareArgs A)
{
  const uint32_t tile0 = blockIdx.x * A.tile;
  place_compare_tile<false>(A, nullptr, A.count, blockIdx.y, tile0, min(tile0 + A.tile, A.count), true);
}

// --- the gated query: a list of eligible entries per query, the comparison over the lists -------------------------------
struct PlaceGate { uint32_t limit, pose; };              // lfx_place_gate
constexpr uint32_t kPlaceNoPose = 0xFFFFFFFFu;           // LFX_PLACE_NO_POSE

// One workgroup per query: list[query][0 .. n) = the entries e < limit that pass the position test, ascending, and
// n_eligible[query] = n.  The test is lfx_keyframes_submap's: (dx^2 + dy^2) + dz^2 <= r2 in double, in that order, d = the
// translation of poses[e] minus that of poses[gate.pose]; no poses, or a gate without one, passes every entry.  The
// workgroup walks the entries in steps of kGateRounds rounds of 256 -- a thread's loads of a step are all in flight before
// the first is used, and a step costs one barrier.  An entry's slot is the number of passing entries before it: those of
// the wave's lower lanes in its round (a 64-bit ballot), of the lower waves of the round and of the rounds before in the
// step (their ballots' counts, through LDS), and of the steps before -- so the list is ascending and the same whatever the
// schedule.  No atomics.
constexpr uint32_t kGateRounds = 8;
__global__ __launch_bounds__(kPlaceThreads) void place_gate_kernel(const PlaceGate * gates, const double * poses, double r2, uint32_t stride,
  uint32_t * list, uint32_t * n_eligible)
{
  constexpr uint32_t kWaves = kPlaceThreads / 64, kStep = kGateRounds * kPlaceThreads;
  __shared__ uint32_t wave_n[2][kGateRounds][kWaves];
  const uint32_t query = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const PlaceGate g = gates[query];
  const uint32_t limit = min(g.limit, stride);           // (the host has checked limit <= stride: the list is never overrun)
  const bool test = poses != nullptr && g.pose != kPlaceNoPose;
  double cx = 0.0, cy = 0.0, cz = 0.0;
  if (test) {
    const double * t = poses + 12u * (size_t)g.pose;
    cx = t[3]; cy = t[7]; cz = t[11];
  }
  uint32_t * out = list + (size_t)query * stride;
  uint32_t base = 0, flip = 0;
  for (uint32_t e0 = 0; e0 < limit; e0 += kStep, flip ^= 1u) {
    double x[kGateRounds], y[kGateRounds], z[kGateRounds];
    if (test) {
#pragma unroll
      for (uint32_t r = 0; r < kGateRounds; r++) {
        const uint32_t e = min(e0 + r * kPlaceThreads + threadIdx.x, limit - 1u);   // (past the limit: a pose that is there, not used)
        const double * t = poses + 12u * (size_t)e;
        x[r] = t[3]; y[r] = t[7]; z[r] = t[11];
      }
    }
    unsigned long long ballot[kGateRounds];
#pragma unroll
    for (uint32_t r = 0; r < kGateRounds; r++) {
      bool pass = e0 + r * kPlaceThreads + threadIdx.x < limit;
      if (test) {
        const double dx = x[r] - cx, dy = y[r] - cy, dz = z[r] - cz;
        pass = pass && (dx * dx + dy * dy) + dz * dz <= r2;
      }
      ballot[r] = __ballot(pass);
      if (lane == 0) {wave_n[flip][r][wave] = (uint32_t)__popcll(ballot[r]);}
    }
    __syncthreads();                                     // (two sets of counts: the next step writes the other one)
    const unsigned long long below = (1ull << lane) - 1ull, mine = 1ull << lane;
#pragma unroll
    for (uint32_t r = 0; r < kGateRounds; r++) {
      uint32_t before = base;
      for (uint32_t w = 0; w < kWaves; w++) {
        const uint32_t c = wave_n[flip][r][w];
        before += w < wave ? c : 0u;
        base += c;
      }
      if (ballot[r] & mine) {out[before + (uint32_t)__popcll(ballot[r] & below)] = e0 + r * kPlaceThreads + threadIdx.x;}
    }
  }
  if (threadIdx.x == 0) {n_eligible[query] = base;}
}

// grid (workgroups to a query, queries): workgroup b takes the tiles b, b + gridDim.x, ... of A.tile slots of the query's
// list and stops at the list's end -- the lists' lengths are known on the device only, and a launch sized by the largest
// limit in workgroups of one tile each would spend its time starting workgroups that have nothing to do.  Results at
// [query][stride] by slot.
__global__ __launch_bounds__(kPlaceThreads) void place_compare_gated_kernel(const PlaceCompareArgs A, const uint32_t * list, const uint32_t * n_eligible,
  uint32_t stride)
{
  const uint32_t query = blockIdx.y, n = n_eligible[query];
  // (n is the whole workgroup's: every thread makes the same trips.  The query is staged by the first trip and only read
  // afterwards; a trip's first barrier stands between the trip before's reads of its last pass's distances -- the one
  // thing a later trip writes that an earlier one may still be reading -- and this trip's writes of them)
  const uint32_t first = blockIdx.x * A.tile;
  for (uint32_t tile0 = first; tile0 < n; tile0 += gridDim.x * A.tile) {
    place_compare_tile<true>(A, list + (size_t)query * stride, stride, query, tile0, min(tile0 + A.tile, n), tile0 == first);
  }
}

struct PlaceMatchDevice { uint32_t entry, shift; double distance; };

// One workgroup per query: the k best of its `count` distances, ascending, equal distances by the lower entry, in k rounds
// of "the least (distance, entry) pair above the one taken last" -- a strict total order, so nothing depends on how the
// threads share the walk.  Rounds that find nothing leave {UINT32_MAX, 0, +inf}.
// The gated query (list, n_eligible not null): a query's distances are those of its list's slots, [query][count] with its own
// n_eligible[query] of them in use; the walk is over slots -- the list is ascending, so the lower slot is the lower entry --
// and the winner's entry is its slot's.
__global__ __launch_bounds__(kPlaceThreads) void place_select_kernel(const double * best_distance, const uint32_t * best_shift, uint32_t count,
  uint32_t first, uint32_t k, PlaceMatchDevice * matches, const uint32_t * list, const uint32_t * n_eligible)
{
  __shared__ double sd[kPlaceThreads];
  __shared__ uint32_t se[kPlaceThreads];
  const uint32_t query = blockIdx.x;
  const double * d = best_distance + (size_t)query * count;
  const uint32_t stride = count;
  if (n_eligible) {count = n_eligible[query];}
  double last_d = 0.0;
  uint32_t last_e = kSentinel;                            // (kSentinel: nothing taken yet)
  for (uint32_t r = 0; r < k; r++) {
    double md = __builtin_inf();
    uint32_t me = kSentinel;
    for (uint32_t e = threadIdx.x; e < count; e += blockDim.x) {
      const double v = d[e];
      const bool above = last_e == kSentinel || v > last_d || (v == last_d && e > last_e);
      const bool below = me == kSentinel ? v <= md : (v < md || (v == md && e < me));   // (v <= +inf: a NaN is never taken)
      if (above && below) {md = v; me = e;}
    }
    sd[threadIdx.x] = md; se[threadIdx.x] = me;
    __syncthreads();
    for (uint32_t w = kPlaceThreads / 2; w; w >>= 1) {
      if (threadIdx.x < w) {
        const double od = sd[threadIdx.x + w];
        const uint32_t oe = se[threadIdx.x + w];
        const uint32_t ce = se[threadIdx.x];
        if (oe != kSentinel && (ce == kSentinel || od < sd[threadIdx.x] || (od == sd[threadIdx.x] && oe < ce))) {
          sd[threadIdx.x] = od; se[threadIdx.x] = oe;
        }
      }
      __syncthreads();
    }
    const double wd = sd[0];
    const uint32_t we = se[0];
    __syncthreads();                                     // (everyone has read the winner before the next round writes)
    if (we == kSentinel) {
      // nothing left: this round and every later one
      if (threadIdx.x == 0) {
        for (uint32_t t = r; t < k; t++) {matches[(size_t)query * k + t] = PlaceMatchDevice{kSentinel, 0u, __builtin_inf()};}
      }
      return;
    }
    if (threadIdx.x == 0) {
      const uint32_t entry = list ? list[(size_t)query * stride + we] : first + we;
      matches[(size_t)query * k + r] = PlaceMatchDevice{entry, best_shift[(size_t)query * stride + we], wd};
    }
    last_d = wd; last_e = we;
  }
}

}  // namespace lfx
