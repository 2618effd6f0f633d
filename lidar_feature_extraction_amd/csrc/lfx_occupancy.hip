// lfx_occupancy.hip -- occupancy grids (include/lfx.h, the occupancy section; lfx_kernels_occupancy.hpp): every scan's W
// virtual beams and one pose per scan kept on the device, the grid's hit and miss counts rendered from them at the poses of
// the moment, and the counts emitted as nav_msgs/OccupancyGrid bytes.  The tables come from lfx_occupancy_tables and
// lfx_occupancy_emit_table (lfx_pose.cpp) and from nowhere else.  Everything on the device is allocated by lfx_occupancy_create.
#include "lfx_internal.hpp"
#include "lfx_kernels_occupancy.hpp"

#include <algorithm>
#include <cstdint>

using namespace lfx_host;

static_assert(sizeof(lfx_occupancy_counters_t) == sizeof(uint64_t) * lfx::kOccCounters, "the counters block is the caller's record");
static_assert(lfx::kOccHit == LFX_OCCUPANCY_HIT && lfx::kOccClear == LFX_OCCUPANCY_CLEAR && lfx::kOccNone == LFX_OCCUPANCY_NONE, "the kernels' kinds are the header's");

struct lfx_occupancy
{
  int device = 0;
  lfx_occupancy_config cfg{};
  uint32_t n = 0;                        // scans
  double inv_res = 0.0;
  int64_t reach = 0, side = 0;           // the window: side = 2 * reach + 1 cells, the origin cell `reach` from its lower edges
  uint32_t words = 0;                    // 32-bit words of one bitmap, a multiple of 4
  uint64_t device_bytes = 0;
  DevBuf<uint4> beams;                   // [max_scans][W]
  DevBuf<double> poses;                  // [max_scans][12]
  DevBuf<uint32_t> src;                  // an add's scans: the batch scan of each
  DevBuf<double> table;                  // col_cos [W], col_sin [W]
  DevBuf<unsigned long long> keys;       // [2][chunk_scans][W]: the reduce's minima, then its maxima
  DevBuf<uint32_t> bits;                 // [2][chunk_scans][words]: free, then hit; all zero between two chunks
  DevBuf<uint32_t> hits, misses;         // [height][width]
  DevBuf<unsigned long long> counters;   // [kOccCounters]
  DevBuf<int8_t> lut;                    // the emit's table, 4097 bytes
  lfx_occupancy_emit_config lut_cfg{};   // ... of this config (w_hit 0: none yet)
  PinnedBuf upload;                      // what goes up (poses, an add's scan list, the emit's table): rewritten only once
                                         // the object's last queued call has passed
  PinnedBuf readback;                    // the counters
  PinnedBuf image;                       // lfx_occupancy_save: the emitted grid
  Tail tail;                             // behind the last call that touched the object
};

namespace
{
int check_grid(lfx_ctx * c, const lfx_occupancy * g) {return check_device(c, g->device, "the occupancy grid");}

int check_range(lfx_ctx * c, const lfx_occupancy * g, uint32_t first, uint32_t count)
{
  if (first > g->n || count > g->n - first) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "scans outside the occupancy grid's store");}
  return LFX_OK;
}

const char * kConfigRefused = "the occupancy config is refused: n_beams even in 4 .. 4096, max_scans in 1 .. 2^24, width and height in 1 .. 16384, "
  "resolution finite and > 0, a finite origin, 0 < min_range < max_range <= 65536, z_min <= z_max, chunk_scans in 1 .. 1024, "
  "ceil(max_range / resolution) <= 32768";
const char * kEmitRefused = "the emit config is refused: w_hit and w_miss in 1 .. 1000, l_min < l_max, l_max - l_min <= 4096, min_observations >= 1, reserved 0";

// the emit's table on the device: the config of the call before is there already; another one's goes up through the pinned
// block once the object's last call has passed
int put_lut(Call & k, lfx_occupancy * g, const lfx_occupancy_emit_config & cfg)
{
  int8_t lut[4097];
  if (lfx_occupancy_emit_table(&cfg, lut) != LFX_OK) {return fail(k.c, LFX_ERR_INVALID_ARGUMENT, kEmitRefused);}
  if (g->lut_cfg.w_hit != 0 && std::memcmp(&g->lut_cfg, &cfg, sizeof(cfg)) == 0) {return LFX_OK;}
  LFX_TRY(k.after(g->tail));
  g->lut_cfg.w_hit = 0;
  LFX_TRY(send_block(k.c, g->upload, g->lut.p, lut, (size_t)((int64_t)cfg.l_max - (int64_t)cfg.l_min + 1), k.st));
  LFX_TRY(k.record());
  g->lut_cfg = cfg;
  return LFX_OK;
}

int launch_emit(lfx_ctx * c, lfx_occupancy * g, const lfx_occupancy_emit_config & cfg, int8_t * out, hipStream_t st)
{
  lfx::OccEmitArgs a{};
  occupancy_access(g).emit_args(cfg, a);
  a.out = out;
  a.words = (reinterpret_cast<uintptr_t>(out) & 3u) == 0u;
  hipLaunchKernelGGL(lfx::occupancy_emit_kernel, dim3(blocks_for((a.cells + 3u) / 4u, lfx::kOccThreads)), dim3(lfx::kOccThreads), 0, st, a);
  LFX_HIP(c, hipGetLastError());
  return LFX_OK;
}
}  // namespace

namespace lfx_host
{
OccupancyAccess occupancy_access(const lfx_occupancy * g)
{
  OccupancyAccess a;
  a.device = g->device;
  a.width = g->cfg.width; a.height = g->cfg.height;
  a.hits = g->hits.p; a.misses = g->misses.p;
  a.lut = g->lut.p;
  a.tail = &g->tail;
  a.beams = g->beams.p; a.poses = g->poses.p;
  a.n_scans = g->n; a.n_beams = g->cfg.n_beams;
  return a;
}

void OccupancyAccess::emit_args(const lfx_occupancy_emit_config & cfg, lfx::OccEmitArgs & a) const
{
  a.hits = hits; a.misses = misses;
  a.cells = (uint64_t)width * height;
  a.w_hit = cfg.w_hit; a.w_miss = cfg.w_miss; a.l_min = cfg.l_min; a.l_max = cfg.l_max;
  a.min_observations = cfg.min_observations;
  a.lut = lut;
}

int occupancy_put_table(Call & k, lfx_occupancy * g, const lfx_occupancy_emit_config & config) {return put_lut(k, g, config);}
}  // namespace lfx_host

extern "C" {

int lfx_occupancy_create(lfx_ctx * c, const lfx_occupancy_config * config, lfx_occupancy ** out)
{
  if (!c) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!config || !out) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "config and out are required");}
  // (checked here first: the table below is sized by W)
  if (config->n_beams < 4u || config->n_beams > LFX_OCCUPANCY_MAX_BEAMS) {return fail(c, LFX_ERR_INVALID_ARGUMENT, kConfigRefused);}
  const uint32_t W = config->n_beams;
  std::vector<double> table(2u * (size_t)W);
  if (lfx_occupancy_tables(config, table.data(), table.data() + W) != LFX_OK) {return fail(c, LFX_ERR_INVALID_ARGUMENT, kConfigRefused);}
  LFX_HIP(c, hipSetDevice(c->device));
  lfx_occupancy * g = new (std::nothrow) lfx_occupancy();
  if (!g) {return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the occupancy grid");}
  g->device = c->device;
  g->cfg = *config;
  g->inv_res = 1.0 / (double)config->resolution;
  // an end cell lies at most ceil(max_range * inv_res) + 1 cells from its origin cell on either axis (two floors of values
  // less than that many cells apart); one more on either side
  g->reach = (int64_t)std::ceil((double)config->max_range * g->inv_res) + 2;
  g->side = 2 * g->reach + 1;
  g->words = (uint32_t)((((uint64_t)g->side * (uint64_t)g->side + 31u) / 32u + 3u) & ~(uint64_t)3u);
  const size_t K = config->max_scans, C = config->chunk_scans, cells = (size_t)config->width * config->height;
  auto give_up = [&](int code, const std::string & why) {(void)hipGetLastError(); lfx_occupancy_destroy(g); return fail(c, code, why);};
  DevTotal m;
  m.get(g->beams, K * W); m.get(g->poses, 12u * K); m.get(g->src, K); m.get(g->table, 2u * (size_t)W); m.get(g->keys, 2u * C * W);
  m.get(g->bits, 2u * C * g->words); m.get(g->hits, cells); m.get(g->misses, cells); m.get(g->counters, lfx::kOccCounters); m.get(g->lut, 4097u);
  if (!m.ok) {return give_up(LFX_ERR_OUT_OF_MEMORY, m.refusal("the occupancy grid"));}
  g->device_bytes = m.bytes;
  if (hipMemset(g->bits.p, 0, sizeof(uint32_t) * 2u * C * g->words) != hipSuccess || hipMemset(g->hits.p, 0, sizeof(uint32_t) * cells) != hipSuccess ||
    hipMemset(g->misses.p, 0, sizeof(uint32_t) * cells) != hipSuccess || hipMemset(g->counters.p, 0, sizeof(unsigned long long) * lfx::kOccCounters) != hipSuccess ||
    hipMemcpy(g->table.p, table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice) != hipSuccess)
  {
    return give_up(LFX_ERR_HIP, "cannot clear the occupancy grid");
  }
  if (g->upload.reserve(4096u) != hipSuccess || g->readback.reserve(sizeof(lfx_occupancy_counters_t)) != hipSuccess) {
    return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the occupancy grid's pinned blocks");
  }
  *out = g;
  return LFX_OK;
}

void lfx_occupancy_destroy(lfx_occupancy * g) {destroy_on(g);}

int lfx_occupancy_info(const lfx_occupancy * g, lfx_occupancy_info_t * info)
{
  if (!g || !info) {return LFX_ERR_INVALID_ARGUMENT;}
  *info = lfx_occupancy_info_t{};
  info->n_scans = g->n;
  info->max_scans = g->cfg.max_scans;
  info->n_beams = g->cfg.n_beams;
  info->width = g->cfg.width;
  info->height = g->cfg.height;
  info->chunk_scans = g->cfg.chunk_scans;
  info->window = (uint32_t)g->side;
  info->device_bytes = g->device_bytes;
  return LFX_OK;
}

int lfx_occupancy_view(lfx_ctx * c, const lfx_occupancy * g, lfx_occupancy_view_t * view, void * stream)
{
  if (!c || !g || !view) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_grid(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.read(g->tail));
  *view = lfx_occupancy_view_t{};
  view->beams = reinterpret_cast<const float *>(g->beams.p);
  view->poses = g->poses.p;
  view->hits = g->hits.p;
  view->misses = g->misses.p;
  view->n_scans = g->n;
  return LFX_OK;
}

int lfx_occupancy_add_batch(lfx_ctx * c, lfx_occupancy * g, uint32_t n_scans, const double * poses, const uint8_t * select, const uint8_t * d_class,
  uint32_t obstacle_mask, uint32_t clear_mask, uint32_t * first_id, void * stream)
{
  if (!c || !g || !poses) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_grid(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if ((obstacle_mask | clear_mask) > 15u) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "a class mask has bits 0 .. 3 only");}
  const int rb = check_last_batch(c, n_scans);
  if (rb != LFX_OK) {return rb;}
  if (!c->last_points) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the last batch's input points are not known");}
  if (!finite_all(poses, 12u * (size_t)n_scans)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "a pose that is not finite");}
  uint32_t n = 0;
  for (uint32_t s = 0; s < n_scans; s++) {n += (!select || select[s]) ? 1u : 0u;}
  if (n > g->cfg.max_scans - g->n) {
    return fail(c, LFX_ERR_CAPACITY, "the occupancy grid holds " + std::to_string(g->n) + " of " + std::to_string(g->cfg.max_scans) +
             " scans: no room for " + std::to_string(n) + " more");
  }
  if (first_id) {*first_id = g->n;}
  if (n == 0u) {return LFX_OK;}
  Call call(c, stream);
  hipStream_t st = call.st;
  LFX_TRY(call.open());
  LFX_TRY(call.after(g->tail));
  // the pinned block: [the selected scans' poses][their batch scans]
  const size_t pose_bytes = round64(sizeof(double) * 12u * n);
  LFX_HIP(c, g->upload.reserve(pose_bytes + sizeof(uint32_t) * n));
  double * up_pose = reinterpret_cast<double *>(g->upload.p);
  uint32_t * up_src = reinterpret_cast<uint32_t *>(g->upload.p + pose_bytes);
  uint32_t k = 0;
  for (uint32_t s = 0; s < n_scans; s++) {
    if (select && !select[s]) {continue;}
    std::memcpy(up_pose + 12u * (size_t)k, poses + 12u * (size_t)s, sizeof(double) * 12u);
    up_src[k++] = s;
  }
  const uint32_t W = g->cfg.n_beams, C = g->cfg.chunk_scans;
  LFX_HIP(c, hipMemcpyAsync(g->poses.p + 12u * (size_t)g->n, up_pose, sizeof(double) * 12u * n, hipMemcpyHostToDevice, st));
  LFX_HIP(c, hipMemcpyAsync(g->src.p, up_src, sizeof(uint32_t) * n, hipMemcpyHostToDevice, st));
  lfx::OccReduceArgs a{};
  a.pts = static_cast<const uint8_t *>(c->last_points);
  a.L = c->layout;
  a.scan_begin = c->scan_begin.p;
  a.src = g->src.p;
  a.poses = g->poses.p + 12u * (size_t)g->n;
  a.table = g->table.p;
  a.cls = d_class;
  a.obstacle_mask = obstacle_mask; a.clear_mask = clear_mask;
  a.W = W;
  a.min_range = (double)g->cfg.min_range; a.max_range = (double)g->cfg.max_range;
  a.z_min = (double)g->cfg.z_min; a.z_max = (double)g->cfg.z_max;
  a.kmin = g->keys.p; a.kmax = g->keys.p + (size_t)C * W;
  a.beams = g->beams.p + (size_t)g->n * W;
  const bool xyz16 = canonical_xyz16(c->layout, a.pts);
  const dim3 threads(lfx::kOccThreads);
  const size_t lds = 2u * sizeof(unsigned long long) * (size_t)W;        // (the workgroup's two tables: 64 KB at the largest W)
  for (uint32_t first = 0; first < n; first += C) {
    a.first = first;
    a.scans = std::min(C, n - first);
    LFX_HIP(c, hipMemsetAsync(a.kmin, 0xFF, sizeof(unsigned long long) * (size_t)a.scans * W, st));
    LFX_HIP(c, hipMemsetAsync(a.kmax, 0, sizeof(unsigned long long) * (size_t)a.scans * W, st));
    hipLaunchKernelGGL(xyz16 ? lfx::occupancy_reduce_kernel<true> : lfx::occupancy_reduce_kernel<false>, by_scan_grid(a.scans), threads, lds, st, a);
    hipLaunchKernelGGL(lfx::occupancy_resolve_kernel, dim3(blocks_for((uint64_t)a.scans * W, lfx::kOccThreads)), threads, 0, st, a);
    LFX_HIP(c, hipGetLastError());
  }
  g->n += n;
  return call.finish();
}

int lfx_occupancy_set_poses(lfx_ctx * c, lfx_occupancy * g, uint32_t first, uint32_t count, const double * poses, void * stream)
{
  if (!c || !g || (count && !poses)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_grid(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_range(c, g, first, count) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!finite_all(poses, 12u * (size_t)count)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "a pose that is not finite");}
  if (count == 0u) {return LFX_OK;}
  Call k(c, stream);
  return poses_set(k, g->tail, g->poses, g->upload, first, count, poses);
}

int lfx_occupancy_poses(lfx_ctx * c, const lfx_occupancy * g, uint32_t first, uint32_t count, double * poses_out, void * stream)
{
  if (!c || !g || (count && !poses_out)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_grid(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_range(c, g, first, count) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (count == 0u) {return LFX_OK;}
  Call k(c, stream);
  return poses_get(k, g->tail, g->poses, first, count, poses_out);
}

int lfx_occupancy_follow(lfx_ctx * c, lfx_occupancy * g, const double * d_poses, uint32_t first, uint32_t count, void * stream)
{
  if (!c || !g || (count && !d_poses)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_grid(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_range(c, g, first, count) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (count == 0u) {return LFX_OK;}
  Call k(c, stream);
  return poses_follow(k, g->tail, g->poses, d_poses, first, count);
}

int lfx_occupancy_truncate(lfx_ctx * c, lfx_occupancy * g, uint32_t n_scans, void * stream)
{
  if (!c || !g) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_grid(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (n_scans > g->n) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "the occupancy grid holds " + std::to_string(g->n) + " scans: it cannot be truncated to " + std::to_string(n_scans));
  }
  // (nothing is queued: the dropped scans' beams and poses stay where they are until an add writes over them, and every add
  // waits for the object's last call first -- a reader queued before this call still reads what it was promised)
  g->n = n_scans;
  return LFX_OK;
}

int lfx_occupancy_clear(lfx_ctx * c, lfx_occupancy * g, void * stream)
{
  if (!c || !g) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_grid(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  Call k(c, stream);
  hipStream_t st = k.st;
  LFX_TRY(k.open());
  LFX_TRY(k.behind(g->tail));
  const size_t cells = (size_t)g->cfg.width * g->cfg.height;
  LFX_HIP(c, hipMemsetAsync(g->hits.p, 0, sizeof(uint32_t) * cells, st));
  LFX_HIP(c, hipMemsetAsync(g->misses.p, 0, sizeof(uint32_t) * cells, st));
  LFX_HIP(c, hipMemsetAsync(g->counters.p, 0, sizeof(unsigned long long) * lfx::kOccCounters, st));
  return k.finish();
}

int lfx_occupancy_render(lfx_ctx * c, lfx_occupancy * g, uint32_t first, uint32_t count, void * stream)
{
  if (!c || !g) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_grid(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_range(c, g, first, count) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (count == 0u) {return LFX_OK;}
  Call k(c, stream);
  hipStream_t st = k.st;
  LFX_TRY(k.open());
  LFX_TRY(k.behind(g->tail));
  const uint32_t C = g->cfg.chunk_scans;
  lfx::OccRenderArgs a{};
  a.beams = g->beams.p;
  a.poses = g->poses.p;
  a.W = g->cfg.n_beams; a.width = g->cfg.width; a.height = g->cfg.height;
  a.side = g->side; a.reach = g->reach; a.words = g->words;
  a.origin_x = g->cfg.origin_x; a.origin_y = g->cfg.origin_y; a.inv_res = g->inv_res;
  a.free_bits = g->bits.p; a.hit_bits = g->bits.p + (size_t)C * g->words;
  a.hits = g->hits.p; a.misses = g->misses.p;
  a.counters = g->counters.p;
  const dim3 threads(lfx::kOccThreads);
  for (uint32_t at = first; at < first + count; at += C) {
    a.first = at;
    a.scans = std::min(C, first + count - at);
    hipLaunchKernelGGL(lfx::occupancy_cast_kernel, dim3(blocks_for(a.W, lfx::kOccThreads), a.scans), threads, 0, st, a);
    hipLaunchKernelGGL(lfx::occupancy_fold_kernel, dim3(blocks_for(a.words / 4u, lfx::kOccThreads), a.scans), threads, 0, st, a);
    LFX_HIP(c, hipGetLastError());
  }
  return k.finish();
}

int lfx_occupancy_counters(lfx_ctx * c, const lfx_occupancy * g, lfx_occupancy_counters_t * counters, void * stream)
{
  if (!c || !g || !counters) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_grid(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.read(g->tail));
  LFX_TRY(read_block(c, g->readback, g->counters.p, sizeof(*counters), k.st));
  std::memcpy(counters, g->readback.p, sizeof(*counters));
  return LFX_OK;
}

int lfx_occupancy_emit(lfx_ctx * c, lfx_occupancy * g, const lfx_occupancy_emit_config * config, int8_t * out, void * stream)
{
  if (!c || !g || !config || !out) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_grid(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(put_lut(k, g, *config));
  LFX_TRY(k.behind(g->tail));
  LFX_TRY(launch_emit(c, g, *config, out, k.st));
  return k.finish();
}

int lfx_occupancy_save(lfx_ctx * c, lfx_occupancy * g, const lfx_occupancy_emit_config * config, const char * dirname, int occupied_percent,
  int free_percent, void * stream)
{
  if (!c || !g || !config || !dirname) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_grid(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (free_percent < 0 || !(free_percent < occupied_percent) || occupied_percent > 100) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "the thresholds must be 0 <= free_percent < occupied_percent <= 100");
  }
  Call k(c, stream);
  hipStream_t st = k.st;
  LFX_TRY(k.open());
  LFX_TRY(put_lut(k, g, *config));
  LFX_TRY(k.wait(g->tail));              // (the image block may move)
  const size_t cells = (size_t)g->cfg.width * g->cfg.height;
  if (g->image.reserve(cells) != hipSuccess) {(void)hipGetLastError(); return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the pinned block of the grid");}
  LFX_TRY(launch_emit(c, g, *config, reinterpret_cast<int8_t *>(g->image.p), st));
  LFX_HIP(c, hipStreamSynchronize(st));
  const int rc = lfx_occupancy_write_map(dirname, reinterpret_cast<const int8_t *>(g->image.p), g->cfg.width, g->cfg.height, g->cfg.resolution, g->cfg.origin_x,
      g->cfg.origin_y, occupied_percent, free_percent);
  if (rc != LFX_OK) {return fail(c, rc, std::string("cannot write map.pgm and map.yaml in ") + dirname);}
  return k.finish();                     // (the tail once more where a table went up: the call took it there)
}

}  // extern "C"
