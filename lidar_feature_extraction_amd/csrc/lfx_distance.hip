// lfx_distance.hip -- distance fields and costmaps of occupancy grids (include/lfx.h, the distance section;
// lfx_kernels_distance.hpp): a grid's classes, the exact squared distance of every cell to the nearest obstacle (and, with
// `inside`, to the nearest cell that is none), and from them metres and nav2's inflated costs.  The cost table comes from
// lfx_distance_cost_table (lfx_distmap.cpp) and from nowhere else.  Everything on the device is allocated by
// lfx_distance_create.
#include "lfx_internal.hpp"
#include "lfx_kernels_distance.hpp"

#include <algorithm>
#include <cstdint>

using namespace lfx_host;

static_assert(sizeof(lfx_distance_stats_t) == sizeof(uint64_t) * lfx::kDistStats, "the stats block is the caller's record");
static_assert(lfx::kDistFar == LFX_DISTANCE_FAR && lfx::kDistFree == LFX_DISTANCE_FREE && lfx::kDistUnknown == LFX_DISTANCE_UNKNOWN &&
  lfx::kDistObstacle == LFX_DISTANCE_OBSTACLE, "the kernels' values are the header's");
static_assert(lfx::kDistSites * 1024 >= LFX_OCCUPANCY_MAX_SIDE, "the envelope kernel's largest workgroup owns a whole row");

struct lfx_distance
{
  int device = 0;
  uint32_t W = 0, H = 0, segments = 0;
  uint64_t device_bytes = 0;
  bool transformed = false;              // the last transform's config:
  uint32_t cap = 0;
  bool inside = false;
  DevBuf<uint8_t> cls;                   // [H][W]
  DevBuf<unsigned long long> mask;       // [segments][W]
  DevBuf<uint16_t> below, above;         // [segments][W]
  DevBuf<uint16_t> g;                    // [H][W]
  DevBuf<uint32_t> d2, i2;               // [H][W]
  DevBuf<uint8_t> lut;                   // the cost table, 1024^2 + 1 bytes
  DevBuf<unsigned long long> stats;      // [kDistStats]
  lfx_distance_cost_config lut_cfg{};    // ... of this config and resolution (lut_n 0: none yet)
  float lut_res = 0.0f;
  uint32_t lut_n = 0;
  PinnedBuf upload;                      // the cost table on its way up: rewritten only once the object's last call has passed
  PinnedBuf readback;                    // the stats
  Tail tail;                             // behind the last call that touched the object
};

namespace
{
constexpr uint32_t kLutBytes = LFX_DISTANCE_MAX_COST_CELLS * LFX_DISTANCE_MAX_COST_CELLS + 1u;

int check_field(lfx_ctx * c, const lfx_distance * f) {return check_device(c, f->device, "the distance field");}

bool config_ok(const lfx_distance_config & k)
{
  return k.occupied_percent >= 1 && k.occupied_percent <= 100 && k.unknown_is_obstacle <= 1u && k.max_cells <= 32767u && k.inside <= 1u && k.reserved == 0u;
}
const char * kConfigRefused = "the distance config is refused: occupied_percent in 1 .. 100, unknown_is_obstacle and inside 0 or 1, max_cells 0 or in "
  "1 .. 32767, reserved 0";

// LDS of the envelope kernel for a row of W cells: the minima, then g and the argmins
size_t envelope_lds(uint32_t W) {return 8u * ((size_t)(W + 1u) / 2u + 1u) + 2u * (size_t)((W + 3u) & ~3u) + 2u * (size_t)W;}

template<bool INVERT>
void launch_field(const lfx_distance * f, uint32_t cap, uint32_t * out, unsigned long long * stats, hipStream_t st)
{
  const uint32_t W = f->W, H = f->H;
  lfx::DistColumnArgs a{};
  a.mask = f->mask.p; a.below = f->below.p; a.above = f->above.p; a.g = f->g.p;
  a.W = W; a.H = H; a.segments = f->segments;
  const dim3 threads(lfx::kDistThreads);
  const uint32_t tiles = blocks_for(W, lfx::kDistThreads);
  hipLaunchKernelGGL(lfx::distance_carry_kernel<INVERT>, dim3(tiles, 2u), threads, 0, st, a);
  hipLaunchKernelGGL(lfx::distance_column_kernel<INVERT>, dim3(tiles, f->segments), threads, 0, st, a);
  lfx::DistRowArgs r{};
  r.g = f->g.p; r.out = out; r.W = W; r.H = H; r.cap = cap; r.stats = stats;
  if (cap >= 1u && cap <= lfx::kDistSearchMax) {
    hipLaunchKernelGGL(lfx::distance_row_search_kernel, dim3(H), threads, 2u * (size_t)W, st, r);
  } else if (W <= 64u * lfx::kDistSites) {
    hipLaunchKernelGGL(lfx::distance_row_envelope_kernel<64>, dim3(H), dim3(64), envelope_lds(W), st, r);
  } else if (W <= 256u * lfx::kDistSites) {
    hipLaunchKernelGGL(lfx::distance_row_envelope_kernel<256>, dim3(H), dim3(256), envelope_lds(W), st, r);
  } else {
    hipLaunchKernelGGL(lfx::distance_row_envelope_kernel<1024>, dim3(H), dim3(1024), envelope_lds(W), st, r);
  }
}

// the transform behind the classes' source: `a` holds the grid or the counts
template<bool COUNTS>
int transform(lfx_ctx * c, lfx_distance * f, lfx::DistClassifyArgs & a, const lfx_distance_config & cfg, hipStream_t st)
{
  a.W = f->W; a.H = f->H;
  a.occupied_percent = cfg.occupied_percent;
  a.unknown_is_obstacle = cfg.unknown_is_obstacle;
  a.cls = f->cls.p; a.mask = f->mask.p; a.stats = f->stats.p;
  LFX_HIP(c, hipMemsetAsync(f->stats.p, 0, sizeof(unsigned long long) * lfx::kDistStats, st));
  hipLaunchKernelGGL(lfx::distance_classify_kernel<COUNTS>, dim3(blocks_for(f->W, lfx::kDistThreads), f->segments), dim3(lfx::kDistThreads), 0, st, a);
  launch_field<false>(f, cfg.max_cells, f->d2.p, f->stats.p, st);
  if (cfg.inside) {launch_field<true>(f, cfg.max_cells, f->i2.p, nullptr, st);}
  f->transformed = true;
  f->cap = cfg.max_cells;
  f->inside = cfg.inside != 0u;
  LFX_HIP(c, hipGetLastError());
  return LFX_OK;
}

lfx::DistOutArgs out_args(const lfx_distance * f, const void * out)
{
  lfx::DistOutArgs a{};
  a.cls = f->cls.p; a.d2 = f->d2.p; a.i2 = f->inside ? f->i2.p : nullptr;
  a.cells = (uint64_t)f->W * f->H;
  a.words = (reinterpret_cast<uintptr_t>(out) & 3u) == 0u;
  return a;
}
}  // namespace

namespace lfx_host
{
DistanceAccess distance_access(const lfx_distance * f)
{
  DistanceAccess a;
  a.device = f->device;
  a.width = f->W; a.height = f->H;
  a.transformed = f->transformed;
  a.cap = f->cap;
  a.d2 = f->d2.p;
  a.tail = &f->tail;
  return a;
}
}  // namespace lfx_host

extern "C" {

int lfx_distance_create(lfx_ctx * c, uint32_t width, uint32_t height, lfx_distance ** out)
{
  if (!c) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!out) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "out is required");}
  if (!grid_sides_ok(width, height)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "a distance field has width and height in 1 .. 16384");}
  LFX_HIP(c, hipSetDevice(c->device));
  lfx_distance * f = new (std::nothrow) lfx_distance();
  if (!f) {return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the distance field");}
  f->device = c->device;
  f->W = width; f->H = height;
  f->segments = (height + lfx::kDistSegRows - 1u) / lfx::kDistSegRows;
  const size_t cells = (size_t)width * height, cols = (size_t)f->segments * width;
  auto give_up = [&](int code, const std::string & why) {(void)hipGetLastError(); lfx_distance_destroy(f); return fail(c, code, why);};
  DevTotal m;
  m.get(f->cls, cells); m.get(f->mask, cols); m.get(f->below, cols); m.get(f->above, cols); m.get(f->g, cells); m.get(f->d2, cells); m.get(f->i2, cells);
  m.get(f->lut, kLutBytes); m.get(f->stats, lfx::kDistStats);
  if (!m.ok) {return give_up(LFX_ERR_OUT_OF_MEMORY, m.refusal("the distance field"));}
  f->device_bytes = m.bytes;
  if (hipMemset(f->stats.p, 0, sizeof(unsigned long long) * lfx::kDistStats) != hipSuccess) {return give_up(LFX_ERR_HIP, "cannot clear the distance field");}
  if (f->upload.reserve(kLutBytes) != hipSuccess || f->readback.reserve(sizeof(lfx_distance_stats_t)) != hipSuccess) {
    return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the distance field's pinned blocks");
  }
  // (the widest rows' envelope kernel takes more LDS than a launch is given unasked)
  if (hipFuncSetAttribute(reinterpret_cast<const void *>(&lfx::distance_row_envelope_kernel<1024>), hipFuncAttributeMaxDynamicSharedMemorySize,
      (int)envelope_lds(LFX_OCCUPANCY_MAX_SIDE)) != hipSuccess)
  {
    return give_up(LFX_ERR_HIP, "cannot size the distance field's row kernels");
  }
  *out = f;
  return LFX_OK;
}

void lfx_distance_destroy(lfx_distance * f) {destroy_on(f);}

int lfx_distance_info(const lfx_distance * f, lfx_distance_info_t * info)
{
  if (!f || !info) {return LFX_ERR_INVALID_ARGUMENT;}
  *info = lfx_distance_info_t{};
  info->width = f->W;
  info->height = f->H;
  info->transformed = f->transformed ? 1u : 0u;
  info->max_cells = f->cap;
  info->inside = f->inside ? 1u : 0u;
  info->device_bytes = f->device_bytes;
  return LFX_OK;
}

int lfx_distance_from_grid(lfx_ctx * c, lfx_distance * f, const int8_t * d_grid, const lfx_distance_config * config, void * stream)
{
  if (!c || !f || !d_grid || !config) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_field(c, f) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!config_ok(*config)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, kConfigRefused);}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.behind(f->tail));
  lfx::DistClassifyArgs a{};
  a.grid = d_grid;
  LFX_TRY(transform<false>(c, f, a, *config, k.st));
  return k.finish();
}

int lfx_distance_from_occupancy(lfx_ctx * c, lfx_distance * f, lfx_occupancy * grid, const lfx_occupancy_emit_config * emit_config,
  const lfx_distance_config * config, void * stream)
{
  if (!c || !f || !grid || !emit_config || !config) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_field(c, f) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!config_ok(*config)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, kConfigRefused);}
  const OccupancyAccess src = occupancy_access(grid);
  if (check_device(c, src.device, "the occupancy grid") != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  LFX_TRY(check_same_cells(c, "the occupancy grid", src.width, src.height, "the distance field", f->W, f->H));
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(occupancy_put_table(k, grid, *emit_config));            // (refuses the emit config before anything is queued)
  LFX_TRY(k.behind(*src.tail));
  LFX_TRY(k.behind(f->tail));
  lfx::DistClassifyArgs a{};
  src.emit_args(*emit_config, a.E);
  LFX_TRY(transform<true>(c, f, a, *config, k.st));
  return k.finish();            // (the grid's tail too: its counts are read by the first launch; the whole call is behind it)
}

int lfx_distance_view(lfx_ctx * c, const lfx_distance * f, lfx_distance_view_t * view, void * stream)
{
  if (!c || !f || !view) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_field(c, f) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.read(f->tail));
  *view = lfx_distance_view_t{};
  view->classes = f->cls.p;
  view->d2 = f->d2.p;
  view->i2 = f->inside ? f->i2.p : nullptr;
  return LFX_OK;
}

int lfx_distance_metres(lfx_ctx * c, lfx_distance * f, float resolution, float * out, void * stream)
{
  if (!c || !f || !out) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_field(c, f) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!f->transformed) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the distance field has no transform yet");}
  if (!std::isfinite(resolution) || !(resolution > 0.0f)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the resolution must be finite and > 0");}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.behind(f->tail));
  lfx::DistOutArgs a = out_args(f, out);
  a.res = (double)resolution;
  a.metres = out;
  hipLaunchKernelGGL(lfx::distance_metres_kernel, dim3(blocks_for(a.cells, lfx::kDistThreads)), dim3(lfx::kDistThreads), 0, k.st, a);
  LFX_HIP(c, hipGetLastError());
  return k.finish();
}

int lfx_distance_costmap(lfx_ctx * c, lfx_distance * f, const lfx_distance_cost_config * config, float resolution, uint8_t * out, void * stream)
{
  if (!c || !f || !config || !out) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_field(c, f) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!f->transformed) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the distance field has no transform yet");}
  uint32_t n = 0;
  if (lfx_distance_cost_table_size(config, resolution, &n) != LFX_OK) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "the cost config is refused: radii and scaling finite, 0 <= inscribed_radius <= inflation_radius, cost_scaling_factor "
             ">= 0, track_unknown 0 or 1, a resolution finite and > 0, ceil(inflation_radius / resolution) <= 1024");
  }
  const uint32_t rc_cells = (uint32_t)std::ceil((double)config->inflation_radius / (double)resolution);     // (n is Rc^2 + 1)
  if (f->cap != 0u && f->cap < rc_cells) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "the last transform was capped at " + std::to_string(f->cap) + " cells, the inflation reaches " +
             std::to_string(rc_cells));
  }
  Call k(c, stream);
  LFX_TRY(k.open());
  // the table on the device: the one of the call before is there already (track_unknown is no part of it)
  const bool same = f->lut_n == n && f->lut_res == resolution && f->lut_cfg.inscribed_radius == config->inscribed_radius &&
    f->lut_cfg.inflation_radius == config->inflation_radius && f->lut_cfg.cost_scaling_factor == config->cost_scaling_factor;
  if (!same) {
    LFX_TRY(k.wait(f->tail));
    if (lfx_distance_cost_table(config, resolution, f->upload.p, n) != LFX_OK) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the cost table is refused");}
    f->lut_n = 0;
    LFX_TRY(k.take(f->tail));
    LFX_TRY(send_block(c, f->upload, f->lut.p, nullptr, n, k.st));     // (written in place, into the block lfx_distance_create sized)
    LFX_TRY(k.record());
    f->lut_cfg = *config;
    f->lut_res = resolution;
    f->lut_n = n;
  }
  LFX_TRY(k.behind(f->tail));
  lfx::DistOutArgs a = out_args(f, out);
  a.lut = f->lut.p;
  a.rc2 = n - 1u;
  a.track_unknown = config->track_unknown;
  a.cost = out;
  hipLaunchKernelGGL(lfx::distance_costmap_kernel, dim3(blocks_for((a.cells + 3u) / 4u, lfx::kDistThreads)), dim3(lfx::kDistThreads), 0, k.st, a);
  LFX_HIP(c, hipGetLastError());
  return k.finish();
}

int lfx_distance_stats(lfx_ctx * c, const lfx_distance * f, lfx_distance_stats_t * stats, void * stream)
{
  if (!c || !f || !stats) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_field(c, f) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!f->transformed) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the distance field has no transform yet");}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.read(f->tail));
  LFX_TRY(read_block(c, f->readback, f->stats.p, sizeof(*stats), k.st));
  std::memcpy(stats, f->readback.p, sizeof(*stats));
  return LFX_OK;
}

}  // extern "C"
