// lfx_voxelfilter.hip -- the voxel filter (include/lfx.h, the voxel filter section; lfx_kernels_voxelfilter.hpp): clouds of any
// size thinned to one centroid per voxel of a grid anchored at the world origin, incrementally and to the byte the same
// whatever order the records arrive in.  The table, the rank bitmap and its prefixes are allocated by lfx_voxel_filter_create;
// the host keeps the leaf and the ranks handed out since the reset, which is what a call needs to refuse a request without a
// wait.  lfx_voxel_filter_add_keyframes and lfx_keyframes_save_filtered read a keyframe store where it lies (KeyframesAccess).
#include "lfx_internal.hpp"
#include "lfx_kernels_voxelfilter.hpp"

#include <algorithm>
#include <cstdint>

using namespace lfx_host;

struct lfx_voxel_filter
{
  int device = 0;
  lfx_voxel_filter_config cfg{};
  uint64_t slots = 0;
  float leaf = 0.0f, inv = 0.0f;         // 0 until the first reset
  uint64_t base = 0;                     // ranks handed out since the reset
  uint64_t device_bytes = 0;
  DevBuf<lfx::VfEntry> table;
  DevBuf<uint32_t> bitmap, word_before;  // one bit per rank; per word, the set bits before it in its tile
  DevBuf<uint64_t> tile_before;          // per tile of kVfTileWords words: its set bits, then their exclusive prefix
  DevBuf<unsigned long long> counters;
  DevBuf<float4> staging;                // lfx_voxel_filter_add_host: one chunk of the caller's records
  PinnedBuf readback;                    // an emit's counters
  PinnedBuf upload;                      // add_host's chunk on its way up: rewritten only once the chunk before has passed
  Tail tail;                             // behind the last call that touched the filter
};

namespace
{
constexpr uint64_t kHostChunk = (uint64_t)1 << 16;      // records of `staging`
constexpr uint64_t kMaxRecords = (uint64_t)1 << 40;

int check_filter(lfx_ctx * c, const lfx_voxel_filter * f) {return check_device(c, f->device, "the voxel filter");}

int check_reset(lfx_ctx * c, const lfx_voxel_filter * f)
{
  if (!(f->leaf > 0.0f)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the voxel filter has no leaf: lfx_voxel_filter_reset comes first");}
  return LFX_OK;
}

bool good_leaf(float leaf)
{
  const float inv = 1.0f / leaf;
  return std::isfinite(leaf) && leaf > 0.0f && std::isfinite(inv) && inv > 0.0f;
}

// n more ranks fit behind the ones handed out
int check_ranks(lfx_ctx * c, const lfx_voxel_filter * f, uint64_t n)
{
  if (n > f->cfg.max_records - f->base) {
    return fail(c, LFX_ERR_CAPACITY, "the voxel filter has handed out " + std::to_string(f->base) + " of " + std::to_string(f->cfg.max_records) +
             " ranks: no room for " + std::to_string(n) + " more");
  }
  if ((n + lfx::kVfRun - 1u) / lfx::kVfRun > 0x7FFFFFFFull) {return fail(c, LFX_ERR_CAPACITY, "too many records for one launch");}
  return LFX_OK;
}

uint32_t entry_blocks(const lfx_voxel_filter * f) {return (uint32_t)((f->slots + lfx::kVfThreads - 1u) / lfx::kVfThreads);}

void launch_add(lfx_voxel_filter * f, const float * d_points, uint64_t n, hipStream_t st)
{
  hipLaunchKernelGGL(lfx::voxel_filter_add_kernel, dim3((uint32_t)((n + lfx::kVfRun - 1u) / lfx::kVfRun)), dim3(lfx::kVfThreads), 0, st, f->table.p,
    f->cfg.log2_slots, f->inv, f->counters.p, reinterpret_cast<const float4 *>(d_points), n, f->base);
}

// The passes of an emit up to its only wait: the surviving voxels' least ranks marked, the marks counted and scanned, the
// counters copied down; *r filled.  What voxel_filter_write_kernel places from is left on the device.
int plan_emit(lfx_ctx * c, lfx_voxel_filter * f, uint32_t min_points, lfx_voxel_filter_result * r, hipStream_t st)
{
  const uint64_t n_words = (f->base + 31u) / 32u;
  const uint32_t n_tiles = (uint32_t)((n_words + lfx::kVfTileWords - 1u) / lfx::kVfTileWords);
  LFX_HIP(c, hipMemsetAsync(f->counters.p + lfx::kVfVoxels, 0, 2u * sizeof(unsigned long long), st));
  if (n_words) {LFX_HIP(c, hipMemsetAsync(f->bitmap.p, 0, sizeof(uint32_t) * (size_t)n_words, st));}
  hipLaunchKernelGGL(lfx::voxel_filter_mark_kernel, dim3(entry_blocks(f)), dim3(lfx::kVfThreads), 0, st, f->table.p, f->slots, min_points, f->base,
    f->bitmap.p, f->counters.p);
  LFX_HIP(c, hipGetLastError());
  if (n_tiles) {
    hipLaunchKernelGGL(lfx::voxel_filter_tile_kernel, dim3(n_tiles), dim3(lfx::kVfThreads), 0, st, f->bitmap.p, n_words, f->word_before.p, f->tile_before.p);
    LFX_HIP(c, hipGetLastError());
  }
  hipLaunchKernelGGL(lfx::voxel_filter_scan_kernel, dim3(1), dim3(lfx::kVfThreads), 0, st, f->tile_before.p, n_tiles, f->counters.p);
  LFX_HIP(c, hipGetLastError());
  const uint64_t * h = reinterpret_cast<const uint64_t *>(f->readback.p);
  LFX_TRY(read_block(c, f->readback, f->counters.p, sizeof(uint64_t) * lfx::kVfCounters, st));
  *r = lfx_voxel_filter_result{};
  r->n_records = f->base;
  r->n_accumulated = h[lfx::kVfValid] - h[lfx::kVfTableFull];
  r->n_nonfinite = h[lfx::kVfNonFinite];
  r->n_out_of_range = h[lfx::kVfOutOfRange];
  r->n_table_full = h[lfx::kVfTableFull];
  r->n_voxels = h[lfx::kVfVoxels];
  r->n_written = h[lfx::kVfWritten];
  return LFX_OK;
}

int table_full(lfx_ctx * c, const lfx_voxel_filter * f, const lfx_voxel_filter_result & r)
{
  return fail(c, LFX_ERR_CAPACITY, "the voxel filter's table of " + std::to_string(f->slots) + " entries is full: " + std::to_string(r.n_table_full) +
           " records found no entry for their voxel");
}

// the voxels whose place lies in [lo, lo + window) to d_out[place - lo]
int launch_write(lfx_ctx * c, const lfx_voxel_filter * f, uint32_t min_points, float4 * d_out, uint32_t * d_counts_out, uint64_t lo, uint64_t window,
  hipStream_t st)
{
  hipLaunchKernelGGL(lfx::voxel_filter_write_kernel, dim3(entry_blocks(f)), dim3(lfx::kVfThreads), 0, st, f->table.p, f->slots, min_points, f->inv, f->base,
    f->bitmap.p, f->word_before.p, f->tile_before.p, d_out, d_counts_out, lo, window);
  LFX_HIP(c, hipGetLastError());
  return LFX_OK;
}

}  // namespace

extern "C" {

void lfx_voxel_filter_default_config(lfx_voxel_filter_config * config)
{
  if (!config) {return;}
  *config = lfx_voxel_filter_config{};
}

int lfx_voxel_filter_create(lfx_ctx * c, const lfx_voxel_filter_config * config, lfx_voxel_filter ** out)
{
  if (!c) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!config || !out) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "config and out are required");}
  if (config->log2_slots < 4u || config->log2_slots > 30u) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "log2_slots must be in 4 .. 30");}
  if (config->reserved != 0u) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "reserved must be 0");}
  if (config->max_records < 1u || config->max_records > kMaxRecords) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "max_records must be in 1 .. 2^40");}
  LFX_HIP(c, hipSetDevice(c->device));
  lfx_voxel_filter * f = new (std::nothrow) lfx_voxel_filter();
  if (!f) {return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the voxel filter");}
  f->device = c->device;
  f->cfg = *config;
  f->slots = (uint64_t)1 << config->log2_slots;
  const uint64_t n_words = (config->max_records + 31u) / 32u;
  const uint64_t n_tiles = (n_words + lfx::kVfTileWords - 1u) / lfx::kVfTileWords;
  DevTotal m;
  m.get(f->table, f->slots); m.get(f->bitmap, n_words); m.get(f->word_before, n_words); m.get(f->tile_before, n_tiles + 1u);
  m.get(f->counters, lfx::kVfCounters); m.get(f->staging, std::min(kHostChunk, config->max_records));
  if (!m.ok) {
    lfx_voxel_filter_destroy(f);
    return fail(c, LFX_ERR_OUT_OF_MEMORY, m.refusal("the voxel filter"));
  }
  f->device_bytes = m.bytes;
  if (f->readback.reserve(sizeof(uint64_t) * lfx::kVfCounters) != hipSuccess || f->upload.reserve(sizeof(float4) * f->staging.n) != hipSuccess) {
    (void)hipGetLastError();
    lfx_voxel_filter_destroy(f);
    return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the voxel filter's pinned blocks");
  }
  *out = f;
  return LFX_OK;
}

void lfx_voxel_filter_destroy(lfx_voxel_filter * f) {destroy_on(f);}

int lfx_voxel_filter_info(const lfx_voxel_filter * f, lfx_voxel_filter_info_t * info)
{
  if (!f || !info) {return LFX_ERR_INVALID_ARGUMENT;}
  *info = lfx_voxel_filter_info_t{};
  info->slots = f->slots;
  info->max_records = f->cfg.max_records;
  info->n_records = f->base;
  info->device_bytes = f->device_bytes;
  info->leaf = f->leaf;
  return LFX_OK;
}

int lfx_voxel_filter_reset(lfx_ctx * c, lfx_voxel_filter * f, float leaf, void * stream)
{
  if (!c || !f) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_filter(c, f) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!good_leaf(leaf)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "leaf must be finite and > 0, and so must 1 / leaf");}
  Call k(c, stream);
  hipStream_t st = k.st;
  LFX_TRY(k.open());
  LFX_TRY(k.behind(f->tail));
  hipLaunchKernelGGL(lfx::voxel_filter_clear_kernel, dim3(entry_blocks(f)), dim3(lfx::kVfThreads), 0, st, f->table.p, f->slots);
  LFX_HIP(c, hipGetLastError());
  LFX_HIP(c, hipMemsetAsync(f->counters.p, 0, sizeof(unsigned long long) * lfx::kVfCounters, st));
  f->leaf = leaf;
  f->inv = 1.0f / leaf;
  f->base = 0u;
  return k.finish();
}

int lfx_voxel_filter_add(lfx_ctx * c, lfx_voxel_filter * f, const float * d_points, uint64_t n_points, void * stream)
{
  if (!c || !f) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_filter(c, f) != LFX_OK || check_reset(c, f) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (n_points == 0u) {return LFX_OK;}
  if (!d_points) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "d_points is required");}
  LFX_TRY(check_ranks(c, f, n_points));
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.behind(f->tail));
  launch_add(f, d_points, n_points, k.st);
  LFX_HIP(c, hipGetLastError());
  f->base += n_points;
  return k.finish();
}

int lfx_voxel_filter_add_host(lfx_ctx * c, lfx_voxel_filter * f, const float * points, uint64_t n_points, void * stream)
{
  if (!c || !f) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_filter(c, f) != LFX_OK || check_reset(c, f) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (n_points == 0u) {return LFX_OK;}
  if (!points) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "points is required");}
  LFX_TRY(check_ranks(c, f, n_points));
  Call k(c, stream);
  LFX_TRY(k.open());
  // in chunks of the staging buffer: the pinned block is rewritten once the chunk before has left it, the staging buffer is
  // the stream's from one chunk to the next.  The one call that settles and records once per chunk, not once per call: the
  // tail recorded behind a chunk is what the next chunk's settle waits for before the host writes the block again.
  for (uint64_t lo = 0; lo < n_points; lo += f->staging.n) {
    const uint64_t n = std::min<uint64_t>(f->staging.n, n_points - lo);
    LFX_TRY(k.after(f->tail));
    LFX_TRY(send_block(c, f->upload, f->staging.p, points + 4u * (size_t)lo, sizeof(float4) * (size_t)n, k.st));
    launch_add(f, reinterpret_cast<const float *>(f->staging.p), n, k.st);
    LFX_HIP(c, hipGetLastError());
    f->base += n;
    LFX_TRY(k.finish());
  }
  return LFX_OK;
}

int lfx_voxel_filter_emit(lfx_ctx * c, lfx_voxel_filter * f, uint32_t min_points, float * d_out, uint64_t capacity_points, uint32_t * d_counts_out,
  lfx_voxel_filter_result * result, void * stream)
{
  if (!c || !f || !result) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_filter(c, f) != LFX_OK || check_reset(c, f) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (min_points < 1u) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "min_points must be >= 1");}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.behind(f->tail));
  LFX_TRY(plan_emit(c, f, min_points, result, k.st));
  if (result->n_table_full != 0u) {return table_full(c, f, *result);}
  if (result->n_written > capacity_points) {
    return fail(c, LFX_ERR_CAPACITY, "the filter holds " + std::to_string(result->n_written) + " voxels to write: more than capacity_points (" +
             std::to_string(capacity_points) + ")");
  }
  if (result->n_written > 0u) {
    if (!d_out) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "d_out is required");}
    LFX_TRY(launch_write(c, f, min_points, reinterpret_cast<float4 *>(d_out), d_counts_out, 0u, capacity_points, k.st));
  }
  return k.finish();
}

int lfx_voxel_filter_add_keyframes(lfx_ctx * c, lfx_voxel_filter * f, const lfx_keyframes * kf, int kind, uint32_t first, uint32_t count, int masked,
  void * stream)
{
  if (!c || !f || !kf) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_filter(c, f) != LFX_OK || check_reset(c, f) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  const KeyframesAccess ks = keyframes_access(kf);
  if (check_device(c, ks.device, "the keyframe store") != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (kind != LFX_KEYFRAMES_EDGE && kind != LFX_KEYFRAMES_SURFACE) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "kind must be LFX_KEYFRAMES_EDGE or LFX_KEYFRAMES_SURFACE");}
  if (first > ks.n || count > ks.n - first) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "keyframes outside the store");}
  if (masked && !ks.has_flags) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the store has no flags: lfx_keyframes_reserve_flags comes first");}
  const uint64_t lo = ks.begin[kind][first], hi = ks.begin[kind][first + count];
  if (hi == lo) {return LFX_OK;}
  LFX_TRY(check_ranks(c, f, hi - lo));
  Call k(c, stream);
  hipStream_t st = k.st;
  LFX_TRY(k.open());
  LFX_TRY(k.behind(f->tail));
  LFX_TRY(k.behind(*ks.tail));
  lfx::KfRange a{};
  a.rec_lo = lo; a.rec_hi = hi; a.k_lo = first; a.k_hi = first + count; a.first = first;
  hipLaunchKernelGGL(lfx::voxel_filter_add_keyframes_kernel, dim3((uint32_t)((hi - lo + lfx::kVfRun - 1u) / lfx::kVfRun)), dim3(lfx::kVfThreads), 0, st,
    f->table.p, f->cfg.log2_slots, f->inv, f->counters.p, ks.records[kind], ks.d_begin[kind], ks.poses, masked ? ks.flags[kind] : nullptr, f->base, a);
  LFX_HIP(c, hipGetLastError());
  f->base += hi - lo;
  return k.finish();
}

int lfx_keyframes_save_filtered(lfx_ctx * c, const lfx_keyframes * kf, lfx_voxel_filter * f, const float leaf[2], uint32_t min_points, int masked,
  const char * dirname, int written[2], void * stream)
{
  if (!c || !kf || !f || !leaf || !dirname || !written) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_filter(c, f) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  const KeyframesAccess ks = keyframes_access(kf);
  if (check_device(c, ks.device, "the keyframe store") != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!good_leaf(leaf[0]) || !good_leaf(leaf[1])) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "both leaves must be finite and > 0, and so must 1 / leaf");}
  if (min_points < 1u) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "min_points must be >= 1");}
  if (masked && !ks.has_flags) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the store has no flags: lfx_keyframes_reserve_flags comes first");}
  written[0] = written[1] = 0;
  for (int kind = 0; kind < 2; kind++) {
    if (ks.begin[kind][ks.n] > f->cfg.max_records) {
      return fail(c, LFX_ERR_CAPACITY, std::string("the store's ") + std::to_string(ks.begin[kind][ks.n]) + (kind ? " surface" : " edge") +
               " records are more than the filter's max_records (" + std::to_string(f->cfg.max_records) + ")");
    }
  }
  LFX_HIP(c, hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  for (int kind = 0; kind < 2; kind++) {
    if (ks.begin[kind][ks.n] == 0u) {continue;}
    int rc = lfx_voxel_filter_reset(c, f, leaf[kind], stream);
    if (rc == LFX_OK) {rc = lfx_voxel_filter_add_keyframes(c, f, kf, kind, 0u, ks.n, masked, stream);}
    if (rc != LFX_OK) {return rc;}
    lfx_voxel_filter_result r;
    rc = plan_emit(c, f, min_points, &r, st);     // (behind the add on the same stream; the wait)
    if (rc != LFX_OK) {return rc;}
    if (r.n_table_full != 0u) {return table_full(c, f, r);}
    if (r.n_written == 0u) {continue;}
    // through the store's scratch in chunks of places, as lfx_keyframes_save goes through it in chunks of records
    std::vector<float> host(4u * (size_t)r.n_written);
    for (uint64_t lo = 0; lo < r.n_written; lo += ks.chunk) {
      const uint64_t n = std::min(ks.chunk, r.n_written - lo);
      rc = launch_write(c, f, min_points, ks.scratch, nullptr, lo, n, st);
      if (rc != LFX_OK) {return rc;}
      LFX_HIP(c, hipMemcpyAsync(host.data() + 4u * (size_t)lo, ks.scratch, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, st));
    }
    LFX_HIP(c, hipStreamSynchronize(st));
    LFX_TRY(write_pcd(c, kind_path(dirname, kind), host.data(), r.n_written));
    written[kind] = 1;
  }
  return LFX_OK;
}

}  // extern "C"
