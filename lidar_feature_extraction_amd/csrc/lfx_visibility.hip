// lfx_visibility.hip -- visibility votes over a keyframe store (include/lfx.h, the visibility section;
// lfx_kernels_visibility.hpp): the window's non-empty keyframes become range images, max_resident_images at a time, and every
// record of the window collects the votes of the images near its keyframe.  The host knows from the store's mirror which
// keyframes have records and how many, so nothing is read back but the counters.  Everything on the device is allocated by
// lfx_visibility_create.
#include "lfx_internal.hpp"
#include "lfx_kernels_visibility.hpp"

#include <algorithm>
#include <cstdint>

using namespace lfx_host;

struct lfx_visibility
{
  int device = 0;
  lfx_visibility_config cfg{};
  uint32_t max_window = 0, max_resident = 0;
  uint64_t device_bytes = 0;
  DevBuf<uint32_t> images;               // [max_resident][H * W]
  DevBuf<double> table;                  // lfx_visibility_tables' values
  DevBuf<uint32_t> viewers;              // [max_window]: the window's non-empty keyframes
  DevBuf<unsigned long long> counters;   // [kVisCounters]
  DevBuf<uint32_t> words;                // the vote words of a run whose caller passes none
  PinnedBuf pinned;                      // [the viewer list going up][the counters coming back]
  Tail tail;                             // behind the last run: the images, the list and the words are its
};

namespace
{
constexpr uint32_t kImageBlocks = 8;     // workgroups per viewer of the image launch

size_t counters_at(uint32_t max_window) {return round64(sizeof(uint32_t) * (size_t)max_window);}
}  // namespace

extern "C" {

int lfx_visibility_create(lfx_ctx * c, const lfx_visibility_config * config, uint32_t max_window, uint32_t max_resident_images, lfx_visibility ** out)
{
  if (!c) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!config || !out) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "config and out are required");}
  if (max_resident_images < 1u || max_resident_images > max_window || max_window > LFX_VISIBILITY_MAX_WINDOW) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "1 <= max_resident_images <= max_window <= 65536 is required");
  }
  const uint32_t H = config->n_rows, W = config->n_columns;
  std::vector<double> table;
  if (H <= LFX_SEGMENT_MAX_ROWS && W <= LFX_SEGMENT_MAX_COLUMNS) {table.resize(lfx::vis_table_doubles(H, W));}
  if (table.empty() || lfx_visibility_tables(config, table.data(), table.data() + W, table.data() + 2u * W) != LFX_OK) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "a visibility setting outside its range (include/lfx.h, lfx_visibility_config)");
  }
  LFX_HIP(c, hipSetDevice(c->device));
  lfx_visibility * v = new (std::nothrow) lfx_visibility();
  if (!v) {return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the visibility object");}
  v->device = c->device;
  v->cfg = *config;
  v->max_window = max_window;
  v->max_resident = max_resident_images;
  auto give_up = [&](int code, const std::string & why) {(void)hipGetLastError(); lfx_visibility_destroy(v); return fail(c, code, why);};
  DevTotal m;
  m.get(v->images, (size_t)max_resident_images * H * W); m.get(v->table, table.size()); m.get(v->viewers, max_window);
  m.get(v->counters, lfx::kVisCounters); m.get(v->words, LFX_VISIBILITY_SCRATCH_WORDS);
  if (!m.ok) {return give_up(LFX_ERR_OUT_OF_MEMORY, m.refusal("the visibility object"));}
  v->device_bytes = m.bytes;
  if (v->pinned.reserve(counters_at(max_window) + sizeof(unsigned long long) * lfx::kVisCounters) != hipSuccess) {
    return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the visibility object's pinned block");
  }
  if (hipMemcpy(v->table.p, table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice) != hipSuccess) {
    return give_up(LFX_ERR_HIP, "cannot upload the visibility tables");
  }
  *out = v;
  return LFX_OK;
}

void lfx_visibility_destroy(lfx_visibility * v) {destroy_on(v);}

int lfx_visibility_info(const lfx_visibility * v, lfx_visibility_info_t * info)
{
  if (!v || !info) {return LFX_ERR_INVALID_ARGUMENT;}
  *info = lfx_visibility_info_t{};
  info->config = v->cfg;
  info->max_window = v->max_window;
  info->max_resident_images = v->max_resident;
  info->device_bytes = v->device_bytes;
  return LFX_OK;
}

int lfx_visibility_run(lfx_ctx * c, lfx_visibility * v, const lfx_keyframes * keyframes, uint32_t first, uint32_t count, uint32_t * const d_votes[2],
  uint8_t * const d_flags[2], lfx_visibility_result * result, void * stream)
{
  if (!c || !v || !keyframes || !d_votes || !d_flags || !result) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!d_flags[0] || !d_flags[1]) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "both d_flags entries are required");}
  const KeyframesAccess ks = keyframes_access(keyframes);
  if (check_device(c, v->device, "the visibility object") != LFX_OK || check_device(c, ks.device, "the keyframe store") != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (first > ks.n || count > ks.n - first) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "keyframes outside the store");}
  if (count > v->max_window) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "a window of " + std::to_string(count) + " keyframes: more than max_window (" + std::to_string(v->max_window) + ")");
  }
  *result = lfx_visibility_result{};
  uint64_t lo[2], hi[2];
  for (int kind = 0; kind < 2; kind++) {lo[kind] = ks.begin[kind][first]; hi[kind] = ks.begin[kind][first + count];}
  if (hi[0] == lo[0] && hi[1] == lo[1]) {return LFX_OK;}
  uint32_t n_viewers = 0;
  for (uint32_t k = first; k < first + count; k++) {
    n_viewers += (ks.begin[0][k + 1u] > ks.begin[0][k] || ks.begin[1][k + 1u] > ks.begin[1][k]) ? 1u : 0u;
  }
  const uint32_t M = v->max_resident, n_chunks = blocks_for(n_viewers, M);
  // where the vote words live between chunks: the caller's, or the object's own (edge records first)
  uint32_t * words[2] = {d_votes[0], d_votes[1]};
  uint64_t word_off[2] = {0u, 0u};
  if (n_chunks > 1u) {
    uint64_t used = 0u;
    for (int kind = 0; kind < 2; kind++) {
      if (words[kind]) {continue;}
      words[kind] = v->words.p + used;
      word_off[kind] = lo[kind];
      used += hi[kind] - lo[kind];
    }
    if (used > LFX_VISIBILITY_SCRATCH_WORDS) {
      return fail(c, LFX_ERR_CAPACITY, "a run in " + std::to_string(n_chunks) + " chunks of viewers without d_votes keeps " + std::to_string(used) +
               " vote words of its own: more than " + std::to_string(LFX_VISIBILITY_SCRATCH_WORDS) + " (pass d_votes, or keep more images resident)");
    }
  }
  for (int kind = 0; kind < 2; kind++) {
    if (hi[kind] - lo[kind] > 0x7FFFFFFFull * lfx::kVisThreads) {return fail(c, LFX_ERR_CAPACITY, "too many records for one launch");}
  }
  Call call(c, stream);
  hipStream_t st = call.st;
  LFX_TRY(call.open());
  LFX_TRY(call.after(v->tail));           // the last run's copy of the list has left the pinned block
  uint32_t * list = reinterpret_cast<uint32_t *>(v->pinned.p);
  unsigned long long * back = reinterpret_cast<unsigned long long *>(v->pinned.p + counters_at(v->max_window));
  uint32_t at = 0;
  for (uint32_t k = first; k < first + count; k++) {
    if (ks.begin[0][k + 1u] > ks.begin[0][k] || ks.begin[1][k + 1u] > ks.begin[1][k]) {list[at++] = k;}
  }
  LFX_TRY(call.behind(*ks.tail));
  LFX_HIP(c, hipMemcpyAsync(v->viewers.p, list, sizeof(uint32_t) * n_viewers, hipMemcpyHostToDevice, st));
  LFX_HIP(c, hipMemsetAsync(v->counters.p, 0, sizeof(unsigned long long) * lfx::kVisCounters, st));
  const uint32_t H = v->cfg.n_rows, W = v->cfg.n_columns;
  lfx::VisArgs A{};
  for (int kind = 0; kind < 2; kind++) {A.records[kind] = ks.records[kind]; A.begin[kind] = ks.d_begin[kind];}
  A.poses = ks.poses; A.table = v->table.p; A.viewers = v->viewers.p; A.images = v->images.p; A.counters = v->counters.p;
  A.H = H; A.W = W; A.guard = v->cfg.guard; A.min_through = v->cfg.min_through; A.agree_weight = v->cfg.agree_weight;
  A.first = first; A.count = count; A.n_viewers = n_viewers;
  A.min_range = (double)v->cfg.min_range; A.max_range = (double)v->cfg.max_range;
  A.radius2 = (double)v->cfg.radius * (double)v->cfg.radius;
  A.margin_abs = (double)v->cfg.margin_abs; A.margin_rel = (double)v->cfg.margin_rel;
  hipLaunchKernelGGL(lfx::visibility_pairs_kernel, dim3(blocks_for(n_viewers, lfx::kVisThreads)), dim3(lfx::kVisThreads), 0, st, A);
  LFX_HIP(c, hipGetLastError());
  for (uint32_t chunk = 0; chunk < n_chunks; chunk++) {
    A.chunk_lo = chunk * M;
    A.chunk_n = std::min(M, n_viewers - A.chunk_lo);
    A.first_chunk = chunk == 0u ? 1u : 0u;
    A.last_chunk = chunk + 1u == n_chunks ? 1u : 0u;
    const uint64_t cells = (uint64_t)A.chunk_n * H * W;
    LFX_HIP(c, hipMemsetAsync(v->images.p, 0xFF, sizeof(uint32_t) * cells, st));
    hipLaunchKernelGGL(lfx::visibility_image_kernel, dim3(kImageBlocks, A.chunk_n), dim3(lfx::kVisThreads), 0, st, A);
    LFX_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(lfx::visibility_occupied_kernel, dim3(blocks_for(cells, lfx::kVisThreads)), dim3(lfx::kVisThreads), 0, st, A, cells);
    LFX_HIP(c, hipGetLastError());
    for (int kind = 0; kind < 2; kind++) {
      if (hi[kind] == lo[kind]) {continue;}
      hipLaunchKernelGGL(lfx::visibility_vote_kernel, dim3(blocks_for(hi[kind] - lo[kind], lfx::kVisThreads)), dim3(lfx::kVisThreads), 0, st, A,
        ks.records[kind], ks.d_begin[kind], ks.poses, v->table.p, v->viewers.p, v->images.p, kind, lo[kind], hi[kind], words[kind],
        word_off[kind], d_flags[kind]);
      LFX_HIP(c, hipGetLastError());
    }
  }
  // the call's only wait: the counters
  LFX_HIP(c, hipMemcpyAsync(back, v->counters.p, sizeof(unsigned long long) * lfx::kVisCounters, hipMemcpyDeviceToHost, st));
  LFX_TRY(call.finish());
  LFX_HIP(c, hipStreamSynchronize(st));
  result->n_pairs = back[lfx::kVisPairs];
  for (int kind = 0; kind < 2; kind++) {
    result->n_records[kind] = back[lfx::kVisRecords + kind];
    result->n_voted[kind] = back[lfx::kVisVoted + kind];
    result->n_dynamic[kind] = back[lfx::kVisDynamic + kind];
  }
  result->occupied_cells = back[lfx::kVisOccupied];
  result->total_cells = (uint64_t)n_viewers * H * W;
  result->n_viewer_chunks = n_chunks;
  return LFX_OK;
}

}  // extern "C"
