// lfx_kernels_keyframes.hpp -- the device side of the keyframe store (lfx_keyframes.hip): sensor-frame records copied in as
// they are, world clouds written from them at the store's current poses, and the selection of a submap around a point.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "lfx_kernels_kfrange.hpp"
#include "lfx_kernels_transform.hpp"

namespace lfx
{

// One cloud of an add: `count` records from record `src` of the caller's points to record `dst` of the store; its
// workgroups are [first_block, first_block + ceil(count / kKfThreads)).  MapAppendEntry without the pose: 32 bytes.
struct KfCopyEntry
{
  uint64_t dst;
  uint32_t src, count, first_block, pad[3];
};
static_assert(sizeof(KfCopyEntry) == 32, "KfCopyEntry is 32 bytes");

// The clouds of one add into the store, bit for bit (-0.0, NaN payloads and all: 16 bytes moved as integers, no
// arithmetic).  Workgroups map to (cloud, chunk) as map_append_kernel's do.
__global__ __launch_bounds__(kKfThreads) void keyframes_copy_kernel(
  const KfCopyEntry * __restrict__ table, uint32_t n_entries, const uint4 * __restrict__ src, uint4 * __restrict__ dst)
{
  const uint32_t b = blockIdx.x;
  uint32_t lo = 0u, hi = n_entries;         // table[lo].first_block <= b < table[hi].first_block
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (table[mid].first_block <= b) {lo = mid;} else {hi = mid;}
  }
  const KfCopyEntry * e = table + lo;
  const uint32_t i = (b - e->first_block) * kKfThreads + threadIdx.x;
  if (i < e->count) {
    dst[e->dst + i] = src[(size_t)e->src + i];
  }
}

// World records from sensor-frame records at the store's poses.  Workgroup b has the kKfRun consecutive source records
// from rec_lo + b kKfRun; lane t of it the records t, t + 256, t + 512, t + 768 of the run, each one 16-byte load and one
// 16-byte store.  The keyframe of the run's first record comes from a binary search over `begin`, uniform over the
// workgroup; each wave then walks forward to the keyframe of the first of the 64 records it has in a step (past empty
// keyframes: a while) and keeps that keyframe's pose until it has walked on.  Where a step's 64 records lie in more
// than one keyframe every lane searches for its own.  Plain form: record i goes to dst[i - rec_lo].  Selected form:
// record i of keyframe k goes to dst[out_begin[k - first] + (i - begin[k])], nowhere if that is kKfNone, and a run
// without a written keyframe returns before it loads a record.  No LDS, no atomics.  (Every array is its own
// parameter, const and restrict: what lets the uniform loads of `begin` and `poses` go through the scalar cache.)
template<bool kSelected>
__global__ __launch_bounds__(kKfThreads) void keyframes_transform_kernel(
  const float4 * __restrict__ src, const uint64_t * __restrict__ begin, const double * __restrict__ poses,
  const uint64_t * __restrict__ out_begin, float4 * __restrict__ dst, const KfRange a)
{
  const uint64_t run = a.rec_lo + (uint64_t)blockIdx.x * kKfRun;
  const uint64_t run_end = run + kKfRun < a.rec_hi ? run + kKfRun : a.rec_hi;
  uint32_t lo = a.k_lo, hi = a.k_hi;        // begin[lo] <= run < begin[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (begin[mid] <= run) {lo = mid;} else {hi = mid;}
  }
  uint32_t k = lo;                          // (the last keyframe that begins at or before `run`: it is not empty)
  if (kSelected) {
    bool any = false;
    for (uint32_t q = k; q < a.k_hi && begin[q] < run_end; q++) {
      any = any || out_begin[q - a.first] != kKfNone;
    }
    if (!any) {return;}
  }
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & (kKfWave - 1u);
  float4 p[kKfPerLane];
#pragma unroll
  for (int j = 0; j < kKfPerLane; j++) {
    const uint64_t i = run + (uint32_t)(j * kKfThreads) + threadIdx.x;
    p[j] = i < run_end ? src[i] : float4{0.f, 0.f, 0.f, 0.f};
  }
  uint32_t loaded = kKfNoId;
  double m[12] = {};
#pragma unroll
  for (int j = 0; j < kKfPerLane; j++) {
    const uint64_t iw = run + (uint32_t)(j * kKfThreads) + wave * kKfWave;   // the step's first record: uniform over the wave
    if (iw >= run_end) {break;}
    while (begin[k + 1u] <= iw) {k++;}     // (iw < rec_hi <= begin[k_hi]: k stays below k_hi)
    const uint64_t step_end = iw + kKfWave < run_end ? iw + kKfWave : run_end;
    const uint64_t i = iw + lane;
    if (begin[k + 1u] >= step_end) {
      // one keyframe for the whole step: its pose through the scalar path, reloaded only when the wave has walked on
      if (k != loaded) {
#pragma unroll
        for (int q = 0; q < 12; q++) {m[q] = poses[12u * (size_t)k + q];}
        loaded = k;
      }
      uint64_t o = i - a.rec_lo;
      if (kSelected) {
        const uint64_t ob = out_begin[k - a.first];
        if (ob == kKfNone) {continue;}
        o = ob + (i - begin[k]);
      }
      if (i < step_end) {dst[o] = pcl_transform_record(m, p[j]);}
    } else if (i < step_end) {
      // a boundary inside the step: the last keyframe that begins at or before this lane's record
      uint32_t l = k, h = a.k_hi;
      while (h - l > 1u) {
        const uint32_t mid = l + ((h - l) >> 1);
        if (begin[mid] <= i) {l = mid;} else {h = mid;}
      }
      uint64_t o = i - a.rec_lo;
      if (kSelected) {
        const uint64_t ob = out_begin[l - a.first];
        if (ob == kKfNone) {continue;}
        o = ob + (i - begin[l]);
      }
      dst[o] = pcl_transform_record(poses + 12u * (size_t)l, p[j]);
    }
  }
}

// flag[k] = keyframe first + k lies within `radius` of the centre: (dx^2 + dy^2) + dz^2 <= r2 in double, in that order
// (the units are compiled with -ffp-contract=off), d = t - centre.  One thread per keyframe of the window.
__global__ __launch_bounds__(kKfThreads) void keyframes_flag_kernel(
  const double * __restrict__ poses, uint32_t first, uint32_t count, double cx, double cy, double cz, double r2,
  uint8_t * __restrict__ flag)
{
  const uint32_t k = blockIdx.x * kKfThreads + threadIdx.x;
  if (k >= count) {return;}
  const double * t = poses + 12u * (size_t)(first + k);
  const double dx = t[3] - cx, dy = t[7] - cy, dz = t[11] - cz;
  flag[k] = ((dx * dx + dy * dy) + dz * dz <= r2) ? 1 : 0;
}

struct KfPlanRecord                         // lfx_keyframes_submap_result, as the plan writes it
{
  uint32_t n_selected, n_written;
  uint64_t n_points;
  uint32_t first_id, last_id;
  int32_t truncated;
  uint32_t pad;
};
static_assert(sizeof(KfPlanRecord) == 32, "the plan's record is the header's result");

// One workgroup.  e[k] = the exclusive sum of flag x count over the window; keyframe k is written iff it is flagged and
// e[k] + count[k] <= capacity (the sum only grows: nothing behind the first keyframe that does not fit is written);
// out_begin[k] = e[k] for a written keyframe, kKfNone otherwise.  Integer sums: the same store gives the same bytes.
// Every thread has a contiguous share of the window, sums it, the shares' sums are scanned in LDS, and a second pass
// over the share writes out_begin.  kKept (the masked submap): the counts are not begin's differences but the kept
// records per keyframe of the window, and `begin` is that table, indexed from the window's first keyframe.
template<bool kKept>
__global__ __launch_bounds__(kKfThreads) void keyframes_plan_kernel(
  const uint8_t * __restrict__ flag, const uint64_t * __restrict__ begin, uint32_t first, uint32_t count, uint64_t capacity,
  uint64_t * __restrict__ out_begin, KfPlanRecord * __restrict__ record)
{
  __shared__ uint64_t s_sum[kKfThreads], s_points[kKfThreads];
  __shared__ uint32_t s_selected[kKfThreads], s_written[kKfThreads], s_first[kKfThreads], s_last[kKfThreads];
  const uint32_t t = threadIdx.x;
  const uint32_t share = (count + kKfThreads - 1u) / kKfThreads;
  const uint32_t lo = t * share < count ? t * share : count, hi = lo + share < count ? lo + share : count;
  uint64_t sum = 0;
  for (uint32_t k = lo; k < hi; k++) {
    if (flag[k]) {sum += kKept ? begin[k] : begin[first + k + 1u] - begin[first + k];}
  }
  s_sum[t] = sum;
  __syncthreads();
  for (uint32_t d = 1u; d < kKfThreads; d <<= 1) {     // inclusive scan of the shares' sums
    const uint64_t v = t >= d ? s_sum[t - d] : 0u;
    __syncthreads();
    s_sum[t] += v;
    __syncthreads();
  }
  uint64_t e = s_sum[t] - sum, points = 0;
  uint32_t selected = 0, written = 0, first_id = kKfNoId, last_id = kKfNoId;
  for (uint32_t k = lo; k < hi; k++) {
    uint64_t ob = kKfNone;
    if (flag[k]) {
      const uint64_t c = kKept ? begin[k] : begin[first + k + 1u] - begin[first + k];
      selected++;
      if (e + c <= capacity) {
        ob = e;
        written++;
        points = e + c;
        if (first_id == kKfNoId) {first_id = first + k;}
        last_id = first + k;
      }
      e += c;
    }
    out_begin[k] = ob;
  }
  s_points[t] = points; s_selected[t] = selected; s_written[t] = written; s_first[t] = first_id; s_last[t] = last_id;
  __syncthreads();
  if (t == 0u) {
    KfPlanRecord r{};
    r.first_id = kKfNoId; r.last_id = kKfNoId;
    for (uint32_t q = 0; q < kKfThreads; q++) {       // ascending shares: ascending ids
      r.n_selected += s_selected[q];
      r.n_written += s_written[q];
      if (s_written[q]) {
        r.n_points = s_points[q];
        if (r.first_id == kKfNoId) {r.first_id = s_first[q];}
        r.last_id = s_last[q];
      }
    }
    r.truncated = r.n_written < r.n_selected ? 1 : 0;
    *record = r;
  }
}

// --- the masked build: a world cloud without the records whose flag byte is set, the order kept ---------------------------
// Three launches over the source records [rec_lo, rec_hi) in runs of kKfRun: the kept records of every run counted; the
// counts turned into their exclusive prefix by one workgroup (the total behind the last); then every run placed from its
// prefix on.  Inside a run lane t has the kKfPerLane CONSECUTIVE records from 4 t, so that lane order is record order: a
// lane's place is the run's prefix + the kept records of the lanes before it (ballot and population count within the wave,
// the waves' sums through LDS) + those of its own before the record.

// the kept records among a lane's four, one bit each, and the lane's place among the run's kept records
__device__ inline uint32_t kf_mask_lane(const uint8_t * __restrict__ flags, uint64_t base, uint64_t run_end, uint32_t * s_wave, uint32_t & before)
{
  uint32_t keep = 0u;
#pragma unroll
  for (int j = 0; j < kKfPerLane; j++) {
    const uint64_t i = base + (uint32_t)j;
    if (i < run_end && flags[i] == 0u) {keep |= 1u << j;}
  }
  const uint32_t mine = __popc(keep), lane = threadIdx.x & (kKfWave - 1u), wave = threadIdx.x >> 6;
  // inclusive sum over the wave's lanes
  uint32_t sum = mine;
#pragma unroll
  for (int d = 1; d < (int)kKfWave; d <<= 1) {
    const uint32_t v = __shfl_up(sum, d, kKfWave);
    if ((int)lane >= d) {sum += v;}
  }
  if (lane == kKfWave - 1u) {s_wave[wave] = sum;}
  __syncthreads();
  uint32_t waves_before = 0u;
  for (uint32_t q = 0; q < wave; q++) {waves_before += s_wave[q];}
  before = waves_before + sum - mine;
  return keep;
}

__global__ __launch_bounds__(kKfThreads) void keyframes_mask_count_kernel(
  const uint8_t * __restrict__ flags, uint64_t rec_lo, uint64_t rec_hi, uint64_t * __restrict__ run_count)
{
  __shared__ uint32_t s_wave[kKfThreads / kKfWave];
  const uint64_t run = rec_lo + (uint64_t)blockIdx.x * kKfRun;
  const uint64_t run_end = run + kKfRun < rec_hi ? run + kKfRun : rec_hi;
  uint32_t before;
  const uint32_t keep = kf_mask_lane(flags, run + (uint64_t)threadIdx.x * kKfPerLane, run_end, s_wave, before);
  if (threadIdx.x == kKfThreads - 1u) {run_count[blockIdx.x] = before + __popc(keep);}
}

// One workgroup: run_count[0 .. n_runs) becomes its exclusive prefix, run_count[n_runs] the total.  Shares, an LDS scan of
// their sums and a second pass, as keyframes_plan_kernel does it.
__global__ __launch_bounds__(kKfThreads) void keyframes_mask_scan_kernel(uint64_t * __restrict__ run_count, uint32_t n_runs)
{
  __shared__ uint64_t s_sum[kKfThreads];
  const uint32_t t = threadIdx.x;
  const uint32_t share = (n_runs + kKfThreads - 1u) / kKfThreads;
  const uint32_t lo = t * share < n_runs ? t * share : n_runs, hi = lo + share < n_runs ? lo + share : n_runs;
  uint64_t sum = 0;
  for (uint32_t b = lo; b < hi; b++) {sum += run_count[b];}
  s_sum[t] = sum;
  __syncthreads();
  for (uint32_t d = 1u; d < kKfThreads; d <<= 1) {
    const uint64_t v = t >= d ? s_sum[t - d] : 0u;
    __syncthreads();
    s_sum[t] += v;
    __syncthreads();
  }
  uint64_t e = s_sum[t] - sum;
  for (uint32_t b = lo; b < hi; b++) {
    const uint64_t c = run_count[b];
    run_count[b] = e;
    e += c;
  }
  if (t == kKfThreads - 1u) {run_count[n_runs] = s_sum[t];}
}

// The kept records of every run to dst, transformed as keyframes_transform_kernel transforms them (every lane searches for
// the keyframe of each record it keeps: poses of neighbouring lanes are the same lines).
__global__ __launch_bounds__(kKfThreads) void keyframes_mask_scatter_kernel(
  const float4 * __restrict__ src, const uint64_t * __restrict__ begin, const double * __restrict__ poses,
  const uint8_t * __restrict__ flags, const uint64_t * __restrict__ run_begin, float4 * __restrict__ dst, const KfRange a)
{
  __shared__ uint32_t s_wave[kKfThreads / kKfWave];
  const uint64_t run = a.rec_lo + (uint64_t)blockIdx.x * kKfRun;
  const uint64_t run_end = run + kKfRun < a.rec_hi ? run + kKfRun : a.rec_hi;
  const uint64_t base = run + (uint64_t)threadIdx.x * kKfPerLane;
  uint32_t before;
  const uint32_t keep = kf_mask_lane(flags, base, run_end, s_wave, before);
  if (keep == 0u) {return;}
  uint64_t o = run_begin[blockIdx.x] + before;
  uint32_t l = a.k_lo, h = a.k_hi;            // begin[l] <= base < begin[h]
  while (h - l > 1u) {
    const uint32_t mid = l + ((h - l) >> 1);
    if (begin[mid] <= base) {l = mid;} else {h = mid;}
  }
#pragma unroll
  for (int j = 0; j < kKfPerLane; j++) {
    if (!(keep & (1u << j))) {continue;}
    const uint64_t i = base + (uint32_t)j;
    while (begin[l + 1u] <= i) {l++;}         // (i < rec_hi <= begin[k_hi]: l stays below k_hi)
    dst[o++] = pcl_transform_record(poses + 12u * (size_t)l, src[i]);
  }
}

// One thread per entry of d_begin_out[0 .. count]: the kept records before the first record of keyframe first + j -- the
// prefix of its run plus the kept records of the run before it.
__global__ __launch_bounds__(kKfThreads) void keyframes_mask_begin_kernel(
  const uint8_t * __restrict__ flags, const uint64_t * __restrict__ begin, const uint64_t * __restrict__ run_begin, uint32_t first,
  uint32_t count, uint64_t rec_lo, uint64_t * __restrict__ begin_out)
{
  const uint32_t j = blockIdx.x * kKfThreads + threadIdx.x;
  if (j > count) {return;}
  const uint64_t i = begin[first + j];
  const uint64_t b = (i - rec_lo) / kKfRun;   // (i == rec_hi on a run boundary: run_begin has the total behind the last run)
  uint64_t o = run_begin[b];
  for (uint64_t q = rec_lo + b * kKfRun; q < i; q++) {o += flags[q] == 0u ? 1u : 0u;}
  begin_out[j] = o;
}

// --- the masked submap: the selected keyframes of a window without their flagged records -------------------------------
// Over the window's source records [rec_lo, rec_hi) = [begin[first], begin[first + count)) in runs of kKfRun, after
// keyframes_flag_kernel: the kept records of every run that touches a selected keyframe counted (the other runs count 0 and
// load no flag); keyframes_mask_scan_kernel turns the counts into G, the kept prefix at every run's first record; per
// selected keyframe G(begin[k]) and the kept records G(begin[k + 1]) - G(begin[k]); keyframes_plan_kernel<true> over the
// kept counts; then record i of written keyframe k goes to out_begin[k] + (G(i) - G(begin[k])).  Integer counts and
// prefixes only, no atomic: the same store, flags, poses and arguments give the same bytes.

// run_count[b] = the kept records of run b where a selected keyframe has records in it (or begins in it), 0 otherwise --
// and then no flag is loaded.  a.first = a.k_lo: the window, which `selected` is indexed from.
__global__ __launch_bounds__(kKfThreads) void keyframes_submask_count_kernel(
  const uint8_t * __restrict__ flags, const uint64_t * __restrict__ begin, const uint8_t * __restrict__ selected,
  uint64_t * __restrict__ run_count, const KfRange a)
{
  __shared__ uint32_t s_wave[kKfThreads / kKfWave];
  const uint64_t run = a.rec_lo + (uint64_t)blockIdx.x * kKfRun;
  const uint64_t run_end = run + kKfRun < a.rec_hi ? run + kKfRun : a.rec_hi;
  bool any = false;
  for (uint32_t q = kf_keyframe_of(begin, a.k_lo, a.k_hi, run); q < a.k_hi && begin[q] < run_end; q++) {
    any = any || selected[q - a.first] != 0u;
  }
  if (!any) {                                 // (uniform over the workgroup: nobody is left at the barrier)
    if (threadIdx.x == 0u) {run_count[blockIdx.x] = 0u;}
    return;
  }
  uint32_t before;
  const uint32_t keep = kf_mask_lane(flags, run + (uint64_t)threadIdx.x * kKfPerLane, run_end, s_wave, before);
  if (threadIdx.x == kKfThreads - 1u) {run_count[blockIdx.x] = before + __popc(keep);}
}

// G(i), by one wave: the kept records of the counted runs before record i -- the prefix of its run plus the kept records
// of the run before it, as keyframes_mask_begin_kernel has it (i == rec_hi on a run boundary reads the total behind the
// last run).  Lane l counts the records l, l + 64, .. of the run below i, at most 16 of them; the lanes' counts are summed
// by a butterfly of shuffles, which leaves the sum in every lane (integers: the order does not matter).
__device__ inline uint64_t kf_kept_before(const uint8_t * __restrict__ flags, const uint64_t * __restrict__ run_begin, uint64_t rec_lo, uint64_t i,
  uint32_t lane)
{
  const uint64_t b = (i - rec_lo) / kKfRun;
  uint32_t n = 0u;
  for (uint64_t q = rec_lo + b * kKfRun + lane; q < i; q += kKfWave) {n += flags[q] == 0u ? 1u : 0u;}
#pragma unroll
  for (int d = (int)kKfWave / 2; d >= 1; d >>= 1) {n += __shfl_xor(n, d, kKfWave);}
  return run_begin[b] + n;
}

// One WAVE per keyframe of the window (four to a workgroup): kept_begin[j] = G(begin[first + j]) and kept[j] = the kept
// records of keyframe first + j, both 0 for a keyframe that is not selected or is empty -- no flag of such a keyframe's runs
// is loaded.
__global__ __launch_bounds__(kKfThreads) void keyframes_submask_kept_kernel(
  const uint8_t * __restrict__ flags, const uint64_t * __restrict__ begin, const uint8_t * __restrict__ selected,
  const uint64_t * __restrict__ run_begin, uint32_t first, uint32_t count, uint64_t rec_lo, uint64_t * __restrict__ kept_begin,
  uint64_t * __restrict__ kept)
{
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & (kKfWave - 1u);
  const uint32_t j = blockIdx.x * (kKfThreads / kKfWave) + wave;
  if (j >= count) {return;}                  // (uniform over the wave, as everything below but the lanes' counts)
  const uint64_t lo = begin[first + j], hi = begin[first + j + 1u];
  uint64_t g = 0u, n = 0u;
  if (selected[j] != 0u && hi > lo) {
    g = kf_kept_before(flags, run_begin, rec_lo, lo, lane);
    n = kf_kept_before(flags, run_begin, rec_lo, hi, lane) - g;
  }
  if (lane == 0u) {
    kept_begin[j] = g;
    kept[j] = n;
  }
}

// The kept records of the written keyframes to dst.  Workgroup b has run run0 + b of the count pass; lane t the four
// consecutive records from 4 t (kf_mask_lane: lane order is record order), so a wave has 256 consecutive records.  A
// run without a written keyframe returns before it loads a flag or a record.  Where a wave's records lie in one keyframe
// (found by a walk that is uniform over the wave) its pose, out_begin and kept_begin come through the scalar path;
// otherwise every lane walks from the wave's keyframe to its own records'.
__global__ __launch_bounds__(kKfThreads) void keyframes_submask_scatter_kernel(
  const float4 * __restrict__ src, const uint64_t * __restrict__ begin, const double * __restrict__ poses,
  const uint8_t * __restrict__ flags, const uint64_t * __restrict__ run_begin, const uint64_t * __restrict__ out_begin,
  const uint64_t * __restrict__ kept_begin, float4 * __restrict__ dst, uint32_t run0, const KfRange a)
{
  __shared__ uint32_t s_wave[kKfThreads / kKfWave];
  const uint32_t b = run0 + blockIdx.x;
  const uint64_t run = a.rec_lo + (uint64_t)b * kKfRun;
  const uint64_t run_end = run + kKfRun < a.rec_hi ? run + kKfRun : a.rec_hi;
  uint32_t k = kf_keyframe_of(begin, a.k_lo, a.k_hi, run);
  bool any = false;
  for (uint32_t q = k; q < a.k_hi && begin[q] < run_end; q++) {
    any = any || out_begin[q - a.first] != kKfNone;
  }
  if (!any) {return;}
  const uint64_t base = run + (uint64_t)threadIdx.x * kKfPerLane;
  uint32_t before;
  const uint32_t keep = kf_mask_lane(flags, base, run_end, s_wave, before);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t iw = run + (uint64_t)wave * (kKfWave * kKfPerLane);          // the wave's first record
  if (iw >= run_end) {return;}
  const uint64_t wave_end = iw + kKfWave * kKfPerLane < run_end ? iw + kKfWave * kKfPerLane : run_end;
  while (begin[k + 1u] <= iw) {k++;}          // (iw < rec_hi <= begin[k_hi]: k stays below k_hi)
  const uint64_t g = run_begin[b] + before;   // G(base)
  if (begin[k + 1u] >= wave_end) {
    const uint64_t ob = out_begin[k - a.first];
    if (ob == kKfNone || keep == 0u) {return;}
    double m[12];
#pragma unroll
    for (int q = 0; q < 12; q++) {m[q] = poses[12u * (size_t)k + q];}
    uint64_t o = ob + (g - kept_begin[k - a.first]);
#pragma unroll
    for (int j = 0; j < kKfPerLane; j++) {
      if (keep & (1u << j)) {dst[o++] = pcl_transform_record(m, src[base + (uint32_t)j]);}
    }
  } else {
    if (keep == 0u) {return;}
    uint32_t l = kf_keyframe_of(begin, k, a.k_hi, base);   // (begin[k] <= iw <= base < run_end)
    uint32_t n = 0u;                          // the lane's kept records before record j
#pragma unroll
    for (int j = 0; j < kKfPerLane; j++) {
      if (!(keep & (1u << j))) {continue;}
      const uint64_t i = base + (uint32_t)j;
      while (begin[l + 1u] <= i) {l++;}       // (i < rec_hi <= begin[k_hi])
      const uint64_t ob = out_begin[l - a.first];
      if (ob != kKfNone) {dst[ob + (g + n - kept_begin[l - a.first])] = pcl_transform_record(poses + 12u * (size_t)l, src[i]);}
      n++;
    }
  }
}

}  // namespace lfx
