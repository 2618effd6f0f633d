// lfx_gridmatch.hip -- scan matching in occupancy grids (include/lfx.h, the grid-match section; lfx_kernels_gridmatch.hpp):
// a score field looked up from a distance field's d2, scans kept as levelled 2-D points, candidate poses scored and a window
// of (x, y, yaw) searched exhaustively.  The score table comes from lfx_grid_match_table and the rotations from
// lfx_grid_match_rotations (lfx_gridmatchmap.cpp) and from nowhere else.  Everything on the device is allocated by
// lfx_grid_match_create.
#include "lfx_internal.hpp"
#include "lfx_kernels_gridmatch.hpp"

#include <algorithm>
#include <cstdint>

using namespace lfx_host;

static_assert(lfx::kGmFar == LFX_DISTANCE_FAR && lfx::kGmHit == LFX_OCCUPANCY_HIT, "the kernels' values are the header's");
static_assert(lfx::kGmMaxTable == LFX_GRID_MATCH_MAX_CELLS * LFX_GRID_MATCH_MAX_CELLS + 1u, "the field kernel's LDS holds the largest table");

struct lfx_grid_match
{
  static constexpr uint32_t kSlots = 4;  // searches whose rotation tables are on their way up or in use at once
  int device = 0;
  lfx_grid_match_config cfg{};
  lfx::GmGeom geom{};
  uint32_t t_max = 0;                    // 2 * max_half_theta + 1
  uint64_t device_bytes = 0;
  bool field_set = false;
  uint32_t rs = 0;                       // the table's Rs
  uint32_t n = 0, beams = 0;             // scans set, and the beams each was given with
  DevBuf<uint16_t> S;                    // [H][W]
  DevBuf<uint16_t> lut;                  // the largest table
  DevBuf<double2> points;                // [max_scans][max_beams]
  DevBuf<uint32_t> n_points;             // [max_scans]
  DevBuf<double> levels;                 // [max_scans][9]
  DevBuf<unsigned long long> keys;       // [max_scans][t_max]
  TableSlot slots[kSlots];               // a search's rotations [n][T][2] and centres [n][2]
  uint32_t next = 0;
  PinnedBuf upload;                      // the table or the levels on their way up: rewritten only once the object's last call has passed
  Tail tail;                             // behind the last call that touched the object
};

namespace
{
constexpr size_t kLutBytes = sizeof(uint16_t) * lfx::kGmMaxTable;

int check_matcher(lfx_ctx * c, const lfx_grid_match * m) {return check_device(c, m->device, "the grid matcher");}

bool config_ok(const lfx_grid_match_config & k)
{
  if (!grid_sides_ok(k.width, k.height)) {return false;}
  if (!std::isfinite(k.resolution) || !(k.resolution > 0.0f) || !std::isfinite(k.origin_x) || !std::isfinite(k.origin_y)) {return false;}
  if (k.max_scans < 1u || k.max_scans > 1024u || k.max_beams < 4u || k.max_beams > LFX_OCCUPANCY_MAX_BEAMS) {return false;}
  return k.max_half_x <= LFX_GRID_MATCH_MAX_HALF && k.max_half_y <= LFX_GRID_MATCH_MAX_HALF && k.max_half_theta <= LFX_GRID_MATCH_MAX_HALF_THETA;
}
const char * kConfigRefused = "the grid-match config is refused: width and height in 1 .. 16384, resolution finite and > 0, a finite origin, max_scans in "
  "1 .. 1024, max_beams in 4 .. 4096, max_half_x and max_half_y in 0 .. 256, max_half_theta in 0 .. 180";

size_t slot_doubles(uint32_t scans, uint32_t T) {return (size_t)scans * (2u * (size_t)T + 2u);}

// scans [0, n) of the object from `beams`, levelled by what `a` names; the caller has ordered the stream
int launch_scans(lfx_ctx * c, lfx_grid_match * m, lfx::GmScanArgs & a, uint32_t n, hipStream_t st)
{
  a.points = m->points.p;
  a.n_points = m->n_points.p;
  a.max_beams = m->cfg.max_beams;
  hipLaunchKernelGGL(lfx::gridmatch_scans_kernel, dim3(n), dim3(lfx::kGmThreads), 0, st, a);
  LFX_HIP(c, hipGetLastError());
  m->n = n;
  m->beams = a.W;
  return LFX_OK;
}
}  // namespace

extern "C" {

int lfx_grid_match_create(lfx_ctx * c, const lfx_grid_match_config * config, lfx_grid_match ** out)
{
  if (!c) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!config || !out) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "config and out are required");}
  if (!config_ok(*config)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, kConfigRefused);}
  LFX_HIP(c, hipSetDevice(c->device));
  lfx_grid_match * m = new (std::nothrow) lfx_grid_match();
  if (!m) {return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the grid matcher");}
  m->device = c->device;
  m->cfg = *config;
  m->geom.origin_x = config->origin_x; m->geom.origin_y = config->origin_y;
  m->geom.inv_res = 1.0 / (double)config->resolution;
  m->geom.W = config->width; m->geom.H = config->height;
  m->t_max = 2u * config->max_half_theta + 1u;
  const size_t cells = (size_t)config->width * config->height, K = config->max_scans;
  auto give_up = [&](int code, const std::string & why) {(void)hipGetLastError(); lfx_grid_match_destroy(m); return fail(c, code, why);};
  DevTotal t;
  t.get(m->S, cells); t.get(m->lut, lfx::kGmMaxTable); t.get(m->points, K * config->max_beams); t.get(m->n_points, K); t.get(m->levels, 9u * K);
  t.get(m->keys, K * m->t_max);
  for (uint32_t k = 0; t.ok && k < lfx_grid_match::kSlots; k++) {
    hipError_t mem = hipSuccess;
    t.ok = m->slots[k].take(c, slot_doubles(config->max_scans, m->t_max), mem) == LFX_OK && mem == hipSuccess;
    t.bytes += (uint64_t)m->slots[k].d.n * sizeof(double);
  }
  if (!t.ok) {return give_up(LFX_ERR_OUT_OF_MEMORY, t.refusal("the grid matcher"));}
  m->device_bytes = t.bytes;
  if (hipMemset(m->S.p, 0, sizeof(uint16_t) * cells) != hipSuccess || hipMemset(m->n_points.p, 0, sizeof(uint32_t) * K) != hipSuccess) {
    return give_up(LFX_ERR_HIP, "cannot clear the grid matcher");
  }
  if (m->upload.reserve(std::max(kLutBytes, sizeof(double) * 9u * K)) != hipSuccess) {
    return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the grid matcher's pinned block");
  }
  *out = m;
  return LFX_OK;
}

void lfx_grid_match_destroy(lfx_grid_match * m) {destroy_on(m);}

int lfx_grid_match_info(const lfx_grid_match * m, lfx_grid_match_info_t * info)
{
  if (!m || !info) {return LFX_ERR_INVALID_ARGUMENT;}
  *info = lfx_grid_match_info_t{};
  info->width = m->cfg.width; info->height = m->cfg.height;
  info->max_scans = m->cfg.max_scans; info->max_beams = m->cfg.max_beams;
  info->max_half_x = m->cfg.max_half_x; info->max_half_y = m->cfg.max_half_y; info->max_half_theta = m->cfg.max_half_theta;
  info->field_set = m->field_set ? 1u : 0u;
  info->table_cells = m->rs;
  info->n_scans = m->n; info->n_beams = m->beams;
  info->device_bytes = m->device_bytes;
  return LFX_OK;
}

int lfx_grid_match_view(lfx_ctx * c, const lfx_grid_match * m, lfx_grid_match_view_t * view, void * stream)
{
  if (!c || !m || !view) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_matcher(c, m) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.read(m->tail));
  *view = lfx_grid_match_view_t{};
  view->field = m->S.p;
  view->points = reinterpret_cast<const double *>(m->points.p);
  view->n_points = m->n_points.p;
  return LFX_OK;
}

int lfx_grid_match_set_field(lfx_ctx * c, lfx_grid_match * m, lfx_distance * field, const uint16_t * lut, uint32_t n, void * stream)
{
  if (!c || !m || !field || !lut) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_matcher(c, m) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  const DistanceAccess src = distance_access(field);
  if (check_device(c, src.device, "the distance field") != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  LFX_TRY(check_same_cells(c, "the distance field", src.width, src.height, "the grid matcher", m->cfg.width, m->cfg.height));
  if (!src.transformed) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the distance field has no transform yet");}
  uint32_t rs = 0;
  while (rs < LFX_GRID_MATCH_MAX_CELLS && rs * rs + 1u < n) {rs++;}
  if (n == 0u || rs * rs + 1u != n) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "a score table has Rs*Rs + 1 entries, Rs in 0 .. 64");}
  if (src.cap != 0u && src.cap < rs) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "the last transform was capped at " + std::to_string(src.cap) + " cells, the score table reaches " + std::to_string(rs));
  }
  Call k(c, stream);
  hipStream_t st = k.st;
  LFX_TRY(k.open());
  LFX_TRY(k.after(m->tail));                                      // (the pinned block is rewritten)
  LFX_TRY(k.behind(*src.tail));
  LFX_TRY(send_block(c, m->upload, m->lut.p, lut, sizeof(uint16_t) * n, st));
  lfx::GmFieldArgs a{};
  a.d2 = src.d2; a.lut = m->lut.p; a.n = n;
  a.cells = (uint64_t)m->cfg.width * m->cfg.height;
  a.S = m->S.p;
  const uint32_t blocks = std::min(blocks_for((a.cells + 3u) / 4u, lfx::kGmThreads), lfx::kGmFieldBlocks);
  hipLaunchKernelGGL(lfx::gridmatch_field_kernel, dim3(blocks), dim3(lfx::kGmThreads), 0, st, a);
  LFX_HIP(c, hipGetLastError());
  m->field_set = true;
  m->rs = rs;
  return k.finish();
}

int lfx_grid_match_set_scans(lfx_ctx * c, lfx_grid_match * m, const float * d_beams, uint32_t n_scans, uint32_t n_beams, const double * levels, void * stream)
{
  if (!c || !m || !d_beams) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_matcher(c, m) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (n_scans == 0u || n_beams == 0u) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "n_scans and n_beams must be at least 1");}
  if (n_scans > m->cfg.max_scans || n_beams > m->cfg.max_beams) {
    return fail(c, LFX_ERR_CAPACITY, std::to_string(n_scans) + " scans of " + std::to_string(n_beams) + " beams: the grid matcher holds " +
             std::to_string(m->cfg.max_scans) + " of " + std::to_string(m->cfg.max_beams));
  }
  Call k(c, stream);
  LFX_TRY(k.open());
  lfx::GmScanArgs a{};
  a.beams = reinterpret_cast<const uint4 *>(d_beams);
  a.W = n_beams;
  if (levels) {
    LFX_TRY(k.after(m->tail));                                    // (the pinned block is rewritten)
    LFX_TRY(send_block(c, m->upload, m->levels.p, levels, sizeof(double) * 9u * n_scans, k.st));
    a.lev = m->levels.p; a.lev_stride = 9u; a.row_stride = 3u;
  } else {
    LFX_TRY(k.behind(m->tail));
  }
  LFX_TRY(launch_scans(c, m, a, n_scans, k.st));
  return k.finish();
}

int lfx_grid_match_set_scans_occupancy(lfx_ctx * c, lfx_grid_match * m, lfx_occupancy * grid, uint32_t first, uint32_t count, int use_rotation, void * stream)
{
  if (!c || !m || !grid) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_matcher(c, m) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  const OccupancyAccess src = occupancy_access(grid);
  if (check_device(c, src.device, "the occupancy grid") != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (count == 0u || first > src.n_scans || count > src.n_scans - first) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "scans outside the occupancy grid's store");}
  if (count > m->cfg.max_scans || src.n_beams > m->cfg.max_beams) {
    return fail(c, LFX_ERR_CAPACITY, std::to_string(count) + " scans of " + std::to_string(src.n_beams) + " beams: the grid matcher holds " +
             std::to_string(m->cfg.max_scans) + " of " + std::to_string(m->cfg.max_beams));
  }
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.behind(*src.tail));
  LFX_TRY(k.behind(m->tail));
  lfx::GmScanArgs a{};
  a.beams = src.beams + (size_t)first * src.n_beams;
  a.W = src.n_beams;
  if (use_rotation) {a.lev = src.poses + 12u * (size_t)first; a.lev_stride = 12u; a.row_stride = 4u;}
  LFX_TRY(launch_scans(c, m, a, count, k.st));
  return k.finish();
}

int lfx_grid_match_score(lfx_ctx * c, lfx_grid_match * m, uint32_t scan, const double * d_candidates, uint32_t n_candidates, uint32_t * d_score,
  uint32_t * d_inside, void * stream)
{
  if (!c || !m || !d_candidates || !d_score) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_matcher(c, m) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!m->field_set) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the grid matcher has no field yet");}
  if (scan >= m->n) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "scan " + std::to_string(scan) + " is not set: the grid matcher holds " + std::to_string(m->n));}
  if (n_candidates < 1u || n_candidates > (1u << 24)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "a score call takes 1 .. 2^24 candidates");}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.behind(m->tail));
  lfx::GmScoreArgs a{};
  a.G = m->geom; a.S = m->S.p;
  a.points = m->points.p + (size_t)scan * m->cfg.max_beams;
  a.n_points = m->n_points.p + scan;
  a.cand = d_candidates; a.P = n_candidates;
  a.score = d_score; a.inside = d_inside;
  hipLaunchKernelGGL(lfx::gridmatch_score_kernel, dim3(blocks_for(n_candidates, lfx::kGmThreads)), dim3(lfx::kGmThreads), 0, k.st, a);
  LFX_HIP(c, hipGetLastError());
  return k.finish();
}

int lfx_grid_match_search(lfx_ctx * c, lfx_grid_match * m, uint32_t first, uint32_t n_scans, const double * centres,
  const lfx_grid_match_search_config * search, uint32_t * d_best, uint32_t * d_slice_best, uint32_t * d_volume, void * stream)
{
  if (!c || !m || !centres || !search || !d_best) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_matcher(c, m) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!m->field_set) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the grid matcher has no field yet");}
  if (n_scans == 0u || first > m->n || n_scans > m->n - first) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "scans that are not set in the grid matcher");}
  uint32_t dims[3];
  if (lfx_grid_match_search_size(search, dims) != LFX_OK) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "the search config is refused: half_x and half_y in 0 .. 256, step_cells in 1 .. 16, half_theta in 0 .. 180, "
             "with half_theta > 0 a theta_step finite and > 0");
  }
  if (!finite_all(centres, 3u * (size_t)n_scans)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "a centre that is not finite");}
  if (search->half_x > m->cfg.max_half_x || search->half_y > m->cfg.max_half_y || search->half_theta > m->cfg.max_half_theta) {
    return fail(c, LFX_ERR_CAPACITY, "the window is beyond the grid matcher's maxima (" + std::to_string(m->cfg.max_half_x) + ", " +
             std::to_string(m->cfg.max_half_y) + ", " + std::to_string(m->cfg.max_half_theta) + ")");
  }
  const uint32_t Nx = dims[0], Ny = dims[1], T = dims[2];
  Call call(c, stream);
  hipStream_t st = call.st;
  LFX_TRY(call.open());
  // the rotations and the centres through the next slot of the ring: its block is free once the search that used it last has passed
  TableSlot & slot = m->slots[m->next];
  hipError_t mem = hipSuccess;
  LFX_TRY(slot.take(c, slot_doubles(n_scans, T), mem));
  if (mem != hipSuccess) {return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot hold the search's rotations");}
  double * h_rot = reinterpret_cast<double *>(slot.h.p);
  double * h_centres = h_rot + 2u * (size_t)n_scans * T;
  for (uint32_t k = 0; k < n_scans; k++) {
    if (lfx_grid_match_rotations(centres[3u * k + 2u], search->half_theta, search->theta_step, h_rot + 2u * (size_t)k * T) != LFX_OK) {
      return fail(c, LFX_ERR_INVALID_ARGUMENT, "the search's rotations are refused");
    }
    h_centres[2u * k] = centres[3u * k];
    h_centres[2u * k + 1u] = centres[3u * k + 1u];
  }
  LFX_TRY(call.behind(m->tail));
  LFX_TRY(call.take(slot.used));         // (settled by slot.take)
  LFX_HIP(c, hipMemcpyAsync(slot.d.p, slot.h.p, sizeof(double) * slot_doubles(n_scans, T), hipMemcpyHostToDevice, st));
  LFX_HIP(c, hipMemsetAsync(m->keys.p, 0, sizeof(unsigned long long) * (size_t)n_scans * T, st));
  lfx::GmSearchArgs a{};
  a.G = m->geom; a.S = m->S.p;
  a.points = m->points.p; a.n_points = m->n_points.p;
  a.max_beams = m->cfg.max_beams; a.first = first;
  a.rot = slot.d.p; a.centres = slot.d.p + 2u * (size_t)n_scans * T;
  a.Nx = Nx; a.Ny = Ny; a.T = T;
  a.half_x = search->half_x; a.half_y = search->half_y; a.step = search->step_cells;
  a.tiles_x = blocks_for(Nx, lfx::kGmTileX);
  a.slice_key = m->keys.p;
  a.volume = d_volume;
  a.best = d_best; a.slice_best = d_slice_best;
  const dim3 grid(a.tiles_x * blocks_for(Ny, lfx::kGmTileY), T, n_scans);
  hipLaunchKernelGGL(lfx::gridmatch_search_kernel, grid, dim3(lfx::kGmThreads), sizeof(int2) * (size_t)m->cfg.max_beams, st, a);
  hipLaunchKernelGGL(lfx::gridmatch_best_kernel, dim3(n_scans), dim3(lfx::kGmThreads), 0, st, a);
  LFX_HIP(c, hipGetLastError());
  m->next = (m->next + 1u) % lfx_grid_match::kSlots;
  return call.finish();
}

}  // extern "C"
