// lfx_mapping.hip -- the keyframe mapper: MapBuilder<PointType> (mapping/include/lidar_feature_mapping/map.hpp:95-153) with
// its Map on the device (lfx_kernels_mapping.hpp), and the two savers that write maps with lfx_pcd_write (lfx_pcd.cpp).
// The gate is a sequential chain over the last added pose, so it runs on the host; the clouds never leave the device.
#include "lfx_internal.hpp"
#include "lfx_kernels_mapping.hpp"

#include <algorithm>

using namespace lfx_host;

struct lfx_mapper
{
  int device = 0;
  lfx_mapper_config cfg{};
  DevBuf<float4> map;                        // the map, n records; capacity map.n
  uint64_t n = 0;
  uint64_t added = 0, empty = 0, too_close = 0;
  bool has_pose = false;
  double last[12] = {};                      // prev_transform_
  DevBuf<lfx::MapAppendEntry> table;         // the call's added clouds, uploaded from the pinned block
  DevBuf<float4> staged;                     // lfx_mapper_add_host: the cloud
  // [0, pin_table): the counts and begins a call reads back; [pin_table, ...): the table going up.  The table part is not
  // written again before `uploaded` (recorded behind the previous call's upload and append) has passed.
  PinnedBuf pinned;
  size_t pin_table = 0;
  Tail uploaded;
};

namespace
{
constexpr uint32_t kInitialEntries = 64;

int check(lfx_ctx * c, const lfx_mapper * m) {return check_device(c, m->device, "the mapper");}

// MapBuilder::Callback for n clouds whose begins and counts are known on the host (src: the records they address).
// Decides every outcome, then grows the map if it must and queues one map_append_kernel; all or nothing.
int add_clouds(Call & call, lfx_mapper * m, const float4 * src, const uint32_t * begin, const uint32_t * count, uint32_t n,
  const double * poses, uint8_t * outcomes)
{
  lfx_ctx * c = call.c;
  hipStream_t st = call.st;
  std::vector<uint8_t> out(n);
  std::vector<uint32_t> added;               // indices of the added clouds
  bool has_pose = m->has_pose;
  const double * last = m->last;
  uint64_t n_map = m->n, blocks = 0;
  uint64_t n_empty = 0, n_close = 0;
  for (uint32_t s = 0; s < n; s++) {
    const double * pose = poses + 12 * (size_t)s;
    if (count[s] == 0) {out[s] = LFX_KEYFRAME_EMPTY; n_empty++; continue;}
    if (n_map > 0) {
      double dt = 0., dr = 0.;
      lfx_pose_diff(last, pose, &dt, &dr);
      if (dt < m->cfg.translation_threshold && dr < m->cfg.rotation_threshold) {out[s] = LFX_KEYFRAME_TOO_CLOSE; n_close++; continue;}
    }
    if (count[s] > m->cfg.max_points - n_map) {
      return fail(c, LFX_ERR_CAPACITY, "the map would hold more than max_points (" + std::to_string(m->cfg.max_points) + ") records");
    }
    out[s] = LFX_KEYFRAME_ADDED;
    added.push_back(s);
    n_map += count[s];
    blocks += (count[s] + lfx::kMapAppendThreads - 1u) / lfx::kMapAppendThreads;
    last = pose;
    has_pose = true;
  }
  if (blocks > 0x7FFFFFFFull) {return fail(c, LFX_ERR_CAPACITY, "the call adds too many records for one launch");}
  // grow: max(need, 1.5 x capacity), capped at max_points; the old contents copied on the stream
  if (n_map > m->map.n) {
    const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(n_map, m->map.n + m->map.n / 2), m->cfg.max_points);
    DevBuf<float4> grown;
    if (grown.alloc(want) != hipSuccess) {
      (void)hipGetLastError();
      return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot grow the map to " + std::to_string(want) + " records");
    }
    // (the previous call's append may be queued on another stream: the copy reads the map behind it)
    LFX_TRY(call.read(m->uploaded));
    if (m->n) {LFX_HIP(c, hipMemcpyAsync(grown.p, m->map.p, sizeof(float4) * m->n, hipMemcpyDeviceToDevice, st));}
    // (growth is rare: the copy has read the old map before it goes)
    LFX_HIP(c, hipStreamSynchronize(st));
    m->map = std::move(grown);
  }
  if (!added.empty()) {
    const size_t na = added.size();
    if (m->table.n < na) {
      DevBuf<lfx::MapAppendEntry> t;
      if (t.alloc(na + na / 2) != hipSuccess) {(void)hipGetLastError(); return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the mapper's table");}
      LFX_TRY(call.after(m->uploaded));      // (the previous append may still read the old table)
      m->table = std::move(t);
    }
    const size_t bytes = sizeof(lfx::MapAppendEntry) * na;
    LFX_TRY(call.after(m->uploaded));        // (the previous call's upload has passed: the pinned table may move or be written again)
    LFX_HIP(c, m->pinned.reserve(m->pin_table + bytes));
    lfx::MapAppendEntry * tab = reinterpret_cast<lfx::MapAppendEntry *>(m->pinned.p + m->pin_table);
    uint64_t at = m->n;
    uint32_t first = 0;
    for (size_t k = 0; k < na; k++) {
      const uint32_t s = added[k];
      lfx::MapAppendEntry e{};
      std::memcpy(e.m, poses + 12 * (size_t)s, sizeof(e.m));
      e.dst = at;
      e.src = begin[s];
      e.count = count[s];
      e.first_block = first;
      tab[k] = e;
      at += count[s];
      first += (count[s] + lfx::kMapAppendThreads - 1u) / lfx::kMapAppendThreads;
    }
    LFX_HIP(c, hipMemcpyAsync(m->table.p, tab, bytes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(lfx::map_append_kernel, dim3(first), dim3(lfx::kMapAppendThreads), 0, st, m->table.p, (uint32_t)na, src, m->map.p);
    LFX_HIP(c, hipGetLastError());
    LFX_TRY(call.finish());
  }
  // the call stands: commit
  if (!added.empty()) {std::memcpy(m->last, poses + 12 * (size_t)added.back(), sizeof(m->last));}
  m->has_pose = has_pose;
  m->n = n_map;
  m->added += added.size();
  m->empty += n_empty;
  m->too_close += n_close;
  std::memcpy(outcomes, out.data(), n);
  return LFX_OK;
}

int save_cloud(lfx_ctx * c, const float * d_points, uint64_t n, const std::string & path, hipStream_t st)
{
  std::vector<float> host(4 * (size_t)n);
  LFX_HIP(c, hipMemcpyAsync(host.data(), d_points, sizeof(float) * host.size(), hipMemcpyDeviceToHost, st));
  LFX_HIP(c, hipStreamSynchronize(st));
  return write_pcd(c, path, host.data(), n);
}
}  // namespace

extern "C" {

void lfx_mapper_default_config(lfx_mapper_config * cfg)
{
  if (!cfg) {return;}
  *cfg = lfx_mapper_config{};
  cfg->translation_threshold = 1.0;          // map.hpp:89
  cfg->rotation_threshold = 0.1;             // map.hpp:90
  cfg->initial_capacity_points = (uint64_t)1 << 20;
  cfg->max_points = 0xFFFFFFFFull;
}

int lfx_mapper_create(lfx_ctx * c, const lfx_mapper_config * cfg, lfx_mapper ** out)
{
  if (!c || !cfg || !out) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!(cfg->translation_threshold >= 0.) || !(cfg->rotation_threshold >= 0.)) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "the thresholds must be >= 0");
  }
  if (cfg->max_points == 0 || cfg->max_points > 0xFFFFFFFFull) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "max_points must be in [1, 2^32 - 1]");}
  if (cfg->initial_capacity_points == 0 || cfg->initial_capacity_points > cfg->max_points) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "initial_capacity_points must be in [1, max_points]");
  }
  LFX_HIP(c, hipSetDevice(c->device));
  lfx_mapper * m = new (std::nothrow) lfx_mapper();
  if (!m) {return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the mapper");}
  m->device = c->device;
  m->cfg = *cfg;
  auto give_up = [&](int code, const std::string & why) {lfx_mapper_destroy(m); return fail(c, code, why);};
  if (m->map.alloc(cfg->initial_capacity_points) != hipSuccess) {return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the map");}
  if (m->table.alloc(kInitialEntries) != hipSuccess) {return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the mapper's table");}
  // room for the counts and begins of kInitialEntries clouds at stride 4 (a device batch's scan_info): a batch of up to 64
  // scans allocates nothing in a call that fits the map
  m->pin_table = round64(readback_bytes(kInitialEntries, 4));
  if (m->pinned.reserve(m->pin_table + sizeof(lfx::MapAppendEntry) * kInitialEntries) != hipSuccess) {
    return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the mapper's pinned block");
  }
  *out = m;
  return LFX_OK;
}

void lfx_mapper_destroy(lfx_mapper * m) {destroy_on(m);}

int lfx_mapper_add(lfx_ctx * c, lfx_mapper * m, const float * d_points, const uint32_t * d_begin, const uint32_t * d_count,
  uint32_t count_stride, uint32_t n_clouds, size_t total_points, const double * poses, uint8_t * outcomes, void * stream)
{
  if (!c || !m || !d_points || !d_begin || !d_count || !poses || !outcomes) {return LFX_ERR_INVALID_ARGUMENT;}
  if (n_clouds == 0 || count_stride == 0) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "n_clouds and count_stride must be >= 1");}
  if (!finite_all(poses, 12 * (size_t)n_clouds)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the poses must be finite");}
  if (check(c, m) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  Call k(c, stream);
  LFX_TRY(k.open());
  // the counts and the begins back in one wait: the call's only one
  LFX_TRY(grow_readback(k, m->uploaded, m->pinned, m->pin_table, readback_bytes(n_clouds, count_stride), sizeof(lfx::MapAppendEntry),
    std::max<size_t>(n_clouds, kInitialEntries)));
  const CloudList list{d_begin, d_count, count_stride, total_points, ""};
  std::vector<uint32_t> begin, count;
  LFX_TRY(read_lists(c, &list, 1, n_clouds, m->pinned.p, &begin, &count, k.st));
  return add_clouds(k, m, reinterpret_cast<const float4 *>(d_points), begin.data(), count.data(), n_clouds, poses, outcomes);
}

int lfx_mapper_add_host(lfx_ctx * c, lfx_mapper * m, const float * points, uint32_t n_points, const double pose[12],
  uint8_t * outcome, void * stream)
{
  if (!c || !m || !pose || !outcome || (n_points && !points)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!finite_all(pose, 12)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the pose must be finite");}
  if (check(c, m) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  Call k(c, stream);
  LFX_TRY(k.open());
  const uint32_t zero = 0u;
  if (n_points == 0) {return add_clouds(k, m, nullptr, &zero, &zero, 1, pose, outcome);}
  // staged only where the cloud would be added (nothing is copied for an empty or too-close cloud)
  if (m->n > 0) {
    double dt = 0., dr = 0.;
    lfx_pose_diff(m->last, pose, &dt, &dr);
    if (dt < m->cfg.translation_threshold && dr < m->cfg.rotation_threshold) {
      return add_clouds(k, m, nullptr, &zero, &n_points, 1, pose, outcome);
    }
  }
  LFX_TRY(k.after(m->uploaded));             // (the previous append may still read the staged cloud)
  if (hold(m->staged, n_points) != hipSuccess) {(void)hipGetLastError(); return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot stage the cloud");}
  LFX_HIP(c, hipMemcpyAsync(m->staged.p, points, sizeof(float4) * n_points, hipMemcpyHostToDevice, k.st));
  return add_clouds(k, m, m->staged.p, &zero, &n_points, 1, pose, outcome);
}

int lfx_mapper_view(const lfx_mapper * m, lfx_mapper_store_view * v)
{
  if (!m || !v) {return LFX_ERR_INVALID_ARGUMENT;}
  *v = lfx_mapper_store_view{};
  v->points = reinterpret_cast<const float *>(m->map.p);
  v->n_points = m->n;
  v->capacity_points = m->map.n;
  v->n_added = m->added;
  v->n_empty = m->empty;
  v->n_too_close = m->too_close;
  v->has_pose = m->has_pose ? 1 : 0;
  std::memcpy(v->last_pose, m->last, sizeof(m->last));
  return LFX_OK;
}

int lfx_mapper_save(lfx_ctx * c, const lfx_mapper * m, const char * path, int * written, void * stream)
{
  if (!c || !m || !path || !written) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check(c, m) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  *written = 0;
  if (m->n == 0) {return LFX_OK;}            // "Map is empty! Quit without exporting to a file"
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.read(m->uploaded));              // (the last append may be queued on another stream: the map is read behind it)
  LFX_TRY(save_cloud(c, reinterpret_cast<const float *>(m->map.p), m->n, path, k.st));
  *written = 1;
  return LFX_OK;
}

int lfx_odometry_save(lfx_ctx * c, const lfx_odometry * o, const char * dirname, int written[2], void * stream)
{
  if (!c || !o || !dirname || !written) {return LFX_ERR_INVALID_ARGUMENT;}
  written[0] = written[1] = 0;
  lfx_odometry_store_view v{};
  LFX_TRY(lfx_odometry_view(o, &v));
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.read(odometry_tail(o)));         // (the last append may be queued on another stream: the store is read behind it)
  if (v.n_edge) {
    LFX_TRY(save_cloud(c, v.edge_points, v.n_edge, kind_path(dirname, 0), k.st));
    written[0] = 1;
  }
  if (v.n_surface) {
    LFX_TRY(save_cloud(c, v.surface_points, v.n_surface, kind_path(dirname, 1), k.st));
    written[1] = 1;
  }
  return LFX_OK;
}

}  // extern "C"
