// lfx_segment.hip -- scan segmentation (include/lfx.h, the segmentation section; lfx_kernels_segment.hpp):
// lfx_segment_batch, the class and the cluster id of every input record of the last device batch, and
// lfx_pack_features_segmented, the batch's feature clouds through a class mask.  The tables come from lfx_segment_tables
// (lfx_pose.cpp) and from nowhere else.
#include "lfx_internal.hpp"
#include "lfx_kernels_segment.hpp"

#include <algorithm>
#include <cstdint>

using namespace lfx_host;

namespace
{
// the workspace for `cells` cells, the call before waited for on the call's stream
int take_workspace(Call & k, size_t cells)
{
  lfx_ctx * c = k.c;
  lfx_ctx::SegmentWork & w = c->seg;
  LFX_TRY(k.behind(w.used));
  if (w.image.n < cells) {
    // (growing frees what the call before may still use; to the size asked for and no further: the budget is the most it takes)
    LFX_TRY(k.after(w.used));
    if (hold(w.image, cells, true) != hipSuccess || hold(w.cell, cells, true) != hipSuccess || hold(w.parent, cells, true) != hipSuccess ||
      hold(w.csize, cells, true) != hipSuccess || hold(w.crowmax, cells, true) != hipSuccess)
    {
      (void)hipGetLastError();
      w.image.release(); w.cell.release(); w.parent.release(); w.csize.release(); w.crowmax.release();
      return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the range images");
    }
  }
  return LFX_OK;
}

// the config's tables on the device (*d_table): those of a config seen lately are there already; a new config's take the
// next slot, whose pinned block is rewritten only once every call that used the workspace has passed (the event), and go up
// on the call's stream without a wait -- the event is recorded again behind the copy, so a later refill waits for it too
int put_tables(Call & k, const lfx_segment_config & cfg, const std::vector<double> & table, const double ** d_table)
{
  lfx_ctx * c = k.c;
  lfx_ctx::SegmentWork & w = c->seg;
  for (lfx_ctx::SegmentWork::Table & t : w.tables) {
    if (t.columns == cfg.n_columns && t.row_step == cfg.row_step) {*d_table = t.d.p; return LFX_OK;}
  }
  lfx_ctx::SegmentWork::Table & t = w.tables[w.table_next];
  const size_t bytes = sizeof(double) * table.size();
  if (t.columns) {LFX_TRY(k.after(w.used));}  // (a refill: what read the slot, and its block, is done)
  t.columns = 0;
  if (t.h.reserve(bytes) != hipSuccess || hold(t.d, table.size()) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the segmentation tables");
  }
  std::memcpy(t.h.p, table.data(), bytes);
  LFX_HIP(c, hipMemcpyAsync(t.d.p, t.h.p, bytes, hipMemcpyHostToDevice, k.st));
  LFX_TRY(k.record());
  t.columns = cfg.n_columns;
  t.row_step = cfg.row_step;
  w.table_next = (w.table_next + 1u) % lfx_ctx::SegmentWork::kSegTables;
  *d_table = t.d.p;
  return LFX_OK;
}
}  // namespace

extern "C" {

int lfx_segment_batch(lfx_ctx * c, const lfx_segment_config * cfg, uint32_t n_scans, uint8_t * d_class_out, uint32_t * d_id_out,
  uint32_t * d_counts_out, void * stream)
{
  if (!c) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!cfg || !d_class_out) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "config and d_class_out are required");}
  // (checked here first: the table below is sized by W)
  if (cfg->n_columns < 4u || cfg->n_columns > LFX_SEGMENT_MAX_COLUMNS) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "n_columns must be even, in 4 .. 4096");}
  const uint32_t H = cfg->n_rows, W = cfg->n_columns;
  std::vector<double> table(lfx::seg_table_doubles(W));
  if (lfx_segment_tables(cfg, table.data(), table.data() + W, table.data() + 2u * W) != LFX_OK) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "the segmentation config is refused: n_rows in 1 .. 128, n_columns even in 4 .. 4096, row_step > 0, "
             "0 < min_range < max_range, ground_first_row <= ground_last_row < n_rows, ground_tan >= 0, segment_tan > 0, point and row counts >= 1");
  }
  if (H > c->max_rings) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "n_rows (" + std::to_string(H) + ") is above the context's max_rings (" + std::to_string(c->max_rings) + ")");
  }
  const int rb = check_last_batch(c, n_scans);
  if (rb != LFX_OK) {return rb;}
  if (!c->last_points) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the last batch's input points are not known");}
  Call k(c, stream);
  hipStream_t st = k.st;
  LFX_TRY(k.open());
  const size_t cells = (size_t)H * W;
  const uint32_t per_chunk = (uint32_t)std::max<size_t>(1, LFX_SEGMENT_BUDGET_CELLS / cells);
  // (the chunk's scans are a grid's y dimension: 65 535 at most, which only images of a few cells reach)
  const uint32_t chunk_scans = std::min(std::min(per_chunk, n_scans), 65535u);
  LFX_TRY(take_workspace(k, cells * chunk_scans));
  const double * d_table = nullptr;
  LFX_TRY(put_tables(k, *cfg, table, &d_table));
  lfx_ctx::SegmentWork & w = c->seg;
  if (d_counts_out) {LFX_HIP(c, hipMemsetAsync(d_counts_out, 0, sizeof(uint32_t) * 4u * n_scans, st));}
  lfx::SegmentArgs a{};
  a.pts = static_cast<const uint8_t *>(c->last_points);
  a.L = c->layout;
  a.scan_begin = c->scan_begin.p;
  a.ring_slot = c->slot_id.empty() ? nullptr : c->ring_slot.p;
  a.table = d_table;
  a.H = H; a.W = W; a.max_rings = c->max_rings;
  a.min_range = (double)cfg->min_range; a.max_range = (double)cfg->max_range;
  a.ground_tan2 = (double)cfg->ground_tan * (double)cfg->ground_tan;
  a.segment_tan = (double)cfg->segment_tan;
  a.ground_first = cfg->ground_first_row; a.ground_last = cfg->ground_last_row;
  a.segment_min_points = cfg->segment_min_points; a.small_min_points = cfg->small_min_points; a.small_min_rows = cfg->small_min_rows;
  a.image = w.image.p; a.cell = w.cell.p; a.parent = w.parent.p; a.csize = w.csize.p; a.crowmax = w.crowmax.p;
  a.class_out = d_class_out; a.id_out = d_id_out; a.counts_out = d_counts_out;
  const bool xyz16 = canonical_xyz16(c->layout, a.pts);
  const dim3 threads(lfx::kSegThreads);
  for (uint32_t first = 0; first < n_scans; first += chunk_scans) {
    const uint32_t scans = std::min(chunk_scans, n_scans - first);
    const uint32_t total = (uint32_t)(cells * scans);        // (at most the budget, or one image: below 2^32 either way)
    a.first_scan = first;
    LFX_HIP(c, hipMemsetAsync(w.image.p, 0xFF, sizeof(uint64_t) * total, st));
    const dim3 by_scan = by_scan_grid(scans), by_cell(blocks_for(total, lfx::kSegThreads));
    hipLaunchKernelGGL(xyz16 ? lfx::segment_project_kernel<true> : lfx::segment_project_kernel<false>, by_scan, threads, 0, st, a);
    hipLaunchKernelGGL(lfx::segment_cell_kernel, by_cell, threads, 0, st, a, total);
    hipLaunchKernelGGL(lfx::segment_ground_kernel, by_cell, threads, 0, st, a, total);
    hipLaunchKernelGGL(lfx::segment_hook_kernel, by_cell, threads, 0, st, a, total);
    hipLaunchKernelGGL(lfx::segment_flatten_kernel, by_cell, threads, 0, st, a, total);
    hipLaunchKernelGGL(lfx::segment_stats_kernel, by_cell, threads, 0, st, a, total);
    hipLaunchKernelGGL(xyz16 ? lfx::segment_record_kernel<true> : lfx::segment_record_kernel<false>, by_scan, threads, 0, st, a);
    LFX_HIP(c, hipGetLastError());
  }
  return k.finish();
}

int lfx_pack_features_segmented(lfx_ctx * c, const uint8_t * d_class, uint32_t edge_mask, uint32_t surface_mask, float * d_edge_out,
  float * d_surface_out, uint32_t * d_offsets_out, uint32_t * d_counts_out, size_t capacity_points, void * stream)
{
  if (!c || !d_class || !d_edge_out || !d_surface_out || !d_offsets_out) {return LFX_ERR_INVALID_ARGUMENT;}
  if (c->last_batch == 0) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "no batch has been extracted yet");}
  if ((edge_mask | surface_mask) > 15u) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "a class mask has bits 0 .. 3 only");}
  Call k(c, stream);
  hipStream_t st = k.st;
  LFX_TRY(k.open());
  const uint32_t batch = c->last_batch;
  lfx_ctx::SegmentWork & w = c->seg;
  lfx::SegmentPackArgs a{};
  if (d_counts_out) {
    a.counts = d_counts_out;
  } else {
    // (the context's own: calls on different streams take them one behind the other, as the images)
    LFX_TRY(k.behind(w.used));
    if (w.pack_counts.n < 2u * (size_t)batch) {
      LFX_TRY(k.after(w.used));
      if (hold(w.pack_counts, 2u * (size_t)batch) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the filtered pack's counts");
      }
    }
    a.counts = w.pack_counts.p;
  }
  a.scan_begin = c->scan_begin.p; a.scan_info = c->scan_info.p;
  a.edge_pts = c->edge_pts.p; a.surf_pts = c->surf_pts.p;
  a.edge_idx = c->edge_idx.p; a.surf_idx = c->surf_idx.p;
  a.cls = d_class;
  a.edge_mask = edge_mask; a.surf_mask = surface_mask; a.batch = batch;
  a.capacity = capacity_points > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)capacity_points;
  a.offsets = d_offsets_out;
  a.edge_out = reinterpret_cast<float4 *>(d_edge_out); a.surf_out = reinterpret_cast<float4 *>(d_surface_out);
  const dim3 grid(2, batch), threads(lfx::kSegThreads);
  hipLaunchKernelGGL(lfx::segment_pack_count_kernel, grid, threads, 0, st, a);
  launch_feature_offsets(a.counts, a.counts + batch, 1u, batch, d_offsets_out, st);
  hipLaunchKernelGGL(lfx::segment_pack_kernel, grid, threads, 0, st, a);
  LFX_HIP(c, hipGetLastError());
  return k.finish();                       // (with the caller's counts the call took no event)
}

}  // extern "C"
