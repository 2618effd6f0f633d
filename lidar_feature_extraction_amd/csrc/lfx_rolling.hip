// lfx_rolling.hip -- the rolling voxel map: one point per voxel in a window of fixed size that follows the vehicle, an
// edge store and a surface store (lfx_kernels_rolling.hpp; the contract is in include/lfx.h).  No reference counterpart:
// the map LOAM's mapping stage keeps.  Moving the window is host arithmetic; inserts and extractions are a few launches.
#include "lfx_internal.hpp"
#include "lfx_kernels_rolling.hpp"

#include <algorithm>

using namespace lfx_host;

namespace
{
struct Store
{
  float leaf = 0.f, inv = 0.f;
  uint32_t n[3] = {0u, 0u, 0u};
  int32_t o[3] = {0, 0, 0};
  uint64_t slots = 0;
  uint32_t epoch = 0;                        // insert calls that launched; the stamps of a call carry it
  DevBuf<uint64_t> keys, stamps;
  DevBuf<float4> points;
  DevBuf<unsigned long long> counters;       // [kRollCounters]
  lfx::RollStore view() const
  {
    lfx::RollStore s{};
    s.keys = keys.p; s.stamps = stamps.p; s.points = points.p; s.inv = inv;
    for (int a = 0; a < 3; a++) {s.o[a] = o[a]; s.n[a] = n[a];}
    return s;
  }
};
}  // namespace

struct lfx_rolling_map
{
  int device = 0;
  lfx_rolling_map_config cfg{};
  double pose[12] = {};                      // the pose of the last scan that was placed
  double correction[12] = {};                // C: map <- odometry frame
  Store store[2];
  // lfx_rolling_map_update_batch: the two boxes cut out around a scan's pose and their indexes (map_rebuild), the
  // downsampled surface clouds of the batch with their counts and statuses, a zero word (begin / row begin of one cloud),
  // the batch's scan_info and lengths on the host
  lfx_map * emap = nullptr, * smap = nullptr;
  DevBuf<float4> box[2];
  DevBuf<float> down;
  DevBuf<uint32_t> zero;
  PinnedBuf h_batch;
  DevBuf<uint32_t> partial;                  // the extraction's counts per workgroup (the larger window's)
  DevBuf<uint64_t> total;                    // ... and their sum
  DevBuf<lfx::RollInsertEntry> table;        // the call's clouds, uploaded from the pinned block
  DevBuf<float4> staged;                     // lfx_rolling_map_insert_host: the cloud
  // [0, pin_table): what a call reads back (counts and begins, a total, the counters); [pin_table, ...): the table going
  // up.  The table part is not written again before `tail` (recorded behind the previous insert) has passed.
  PinnedBuf pinned;
  size_t pin_table = 0;
  Tail tail;
};

namespace
{
constexpr uint32_t kInitialEntries = 64;
constexpr uint64_t kMaxSlots = (uint64_t)1 << 31;

int check(lfx_ctx * c, const lfx_rolling_map * rm, int kind)
{
  if (kind != LFX_ROLLING_EDGE && kind != LFX_ROLLING_SURFACE) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "kind must be LFX_ROLLING_EDGE or LFX_ROLLING_SURFACE");}
  return check_device(c, rm->device, "the rolling map");
}

// The clouds of one insert whose begins and counts are known on the host: the table of the non-empty ones with their
// ranks, then the two launches and the call's record behind them.  All or nothing.
int insert_clouds(Call & k, lfx_rolling_map * rm, int kind, const float4 * src, const uint32_t * begin, const uint32_t * count,
  uint32_t n, const double * poses)
{
  lfx_ctx * const c = k.c;
  hipStream_t const st = k.st;
  Store & s = rm->store[kind];
  uint64_t records = 0, blocks = 0;
  size_t na = 0;
  for (uint32_t i = 0; i < n; i++) {
    records += count[i];
    blocks += (count[i] + lfx::kRollThreads - 1u) / lfx::kRollThreads;
    na += count[i] ? 1u : 0u;
  }
  // (a rank is 32 bits and 0xFFFFFFFF - rank must stay above 0)
  if (records > 0xFFFFFFFEull || blocks > 0x7FFFFFFFull) {return fail(c, LFX_ERR_CAPACITY, "the call inserts too many records for one launch");}
  if (na == 0) {return LFX_OK;}
  if (rm->table.n < na) {
    DevBuf<lfx::RollInsertEntry> t;
    if (t.alloc(na + na / 2) != hipSuccess) {(void)hipGetLastError(); return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the rolling map's table");}
    LFX_TRY(k.after(rm->tail));              // (the previous insert may still read the old table)
    rm->table = std::move(t);
  }
  const size_t bytes = sizeof(lfx::RollInsertEntry) * na;
  LFX_TRY(k.after(rm->tail));                // (the previous insert has passed: the pinned table may be written again)
  LFX_HIP(c, rm->pinned.reserve(rm->pin_table + bytes));
  lfx::RollInsertEntry * tab = reinterpret_cast<lfx::RollInsertEntry *>(rm->pinned.p + rm->pin_table);
  uint32_t first = 0, rank = 0;
  size_t at = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (count[i] == 0) {continue;}
    lfx::RollInsertEntry e{};
    std::memcpy(e.m, poses + 12 * (size_t)i, sizeof(e.m));
    e.src = begin[i];
    e.count = count[i];
    e.first_block = first;
    e.rank = rank;
    tab[at++] = e;
    first += (count[i] + lfx::kRollThreads - 1u) / lfx::kRollThreads;
    rank += count[i];
  }
  if (s.epoch == 0xFFFFFFFFu) {              // the epoch wraps: every stamp back to "older than anything"
    LFX_HIP(c, hipMemsetAsync(s.stamps.p, 0, sizeof(uint64_t) * s.slots, st));
    s.epoch = 0u;
  }
  s.epoch++;
  LFX_HIP(c, hipMemcpyAsync(rm->table.p, tab, bytes, hipMemcpyHostToDevice, st));
  const lfx::RollStore v = s.view();
  hipLaunchKernelGGL(lfx::rolling_claim_kernel, dim3(first), dim3(lfx::kRollThreads), 0, st, v, rm->table.p, (uint32_t)na, src, s.epoch, s.counters.p);
  hipLaunchKernelGGL(lfx::rolling_commit_kernel, dim3(first), dim3(lfx::kRollThreads), 0, st, v, rm->table.p, (uint32_t)na, src, s.epoch, s.counters.p);
  LFX_HIP(c, hipGetLastError());
  return k.finish();
}

// the voxel of a coordinate given in metres as a double, clamped to the voxels a key can name
int32_t clamped_voxel(double x, float inv)
{
  const float f = floorf((float)x * inv);
  return (int32_t)std::min(std::max(f, -lfx::kRollVoxelLimit), lfx::kRollVoxelLimit - 1.f);
}

// voxels lo .. hi inclusive clipped to the window and to the voxels a key can name; false where nothing is left
bool clip_box(const Store & s, const int32_t lo[3], const int32_t hi[3], lfx::RollBox * box)
{
  uint64_t cells = 1;
  for (int a = 0; a < 3; a++) {
    const int64_t first = std::max<int64_t>(std::max<int64_t>(lo[a], s.o[a]), -(int64_t)lfx::kRollVoxelLimit);
    const int64_t last = std::min<int64_t>(std::min<int64_t>(hi[a], (int64_t)s.o[a] + s.n[a] - 1), (int64_t)lfx::kRollVoxelLimit - 1);
    if (last < first) {return false;}
    box->lo[a] = (int32_t)first;
    box->b[a] = (uint32_t)(last - first + 1);
    cells *= box->b[a];
  }
  box->cells = (uint32_t)cells;
  return true;
}

// the live voxels of a box: counted (d_out null) or written up to `capacity`; the count read back, one wait.  A read: the
// stream goes behind the tail and nothing is taken
int extract_box(const Call & k, const lfx_rolling_map * rm, int kind, const lfx::RollBox & box, float4 * d_out, uint64_t capacity,
  uint64_t * n_points)
{
  lfx_ctx * const c = k.c;
  hipStream_t const st = k.st;
  const Store & s = rm->store[kind];
  const uint32_t n_blocks = (uint32_t)(((uint64_t)box.cells + lfx::kRollCells - 1u) / lfx::kRollCells);
  const lfx::RollStore v = s.view();
  LFX_TRY(k.read(rm->tail));                 // (the previous insert may be queued on another stream)
  hipLaunchKernelGGL(lfx::rolling_block_count_kernel, dim3(n_blocks), dim3(lfx::kRollThreads), 0, st, v, box, rm->partial.p);
  hipLaunchKernelGGL(lfx::rolling_partial_scan_kernel, dim3(1), dim3(lfx::kRollThreads), 0, st, rm->partial.p, n_blocks, rm->total.p);
  if (d_out && capacity) {
    hipLaunchKernelGGL(lfx::rolling_write_kernel, dim3(n_blocks), dim3(lfx::kRollThreads), 0, st, v, box, rm->partial.p, d_out, capacity);
  }
  LFX_HIP(c, hipGetLastError());
  uint64_t * h_total = reinterpret_cast<uint64_t *>(rm->pinned.p);
  LFX_HIP(c, hipMemcpyAsync(h_total, rm->total.p, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  LFX_HIP(c, hipStreamSynchronize(st));
  *n_points = *h_total;
  return LFX_OK;
}

bool whole_window(const Store & s, lfx::RollBox * box)
{
  int32_t lo[3], hi[3];
  for (int a = 0; a < 3; a++) {lo[a] = s.o[a]; hi[a] = (int32_t)((int64_t)s.o[a] + s.n[a] - 1);}
  return clip_box(s, lo, hi, box);
}

// Poses [R | t], 3 x 4 row-major, composed in double, every 3-term sum as (a0 b0 + a1 b1) + a2 b2
void pose_compose(const double a[12], const double b[12], double out[12])
{
  double r[12];
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 4; j++) {
      double v = (a[4 * i] * b[j] + a[4 * i + 1] * b[4 + j]) + a[4 * i + 2] * b[8 + j];
      if (j == 3) {v = v + a[4 * i + 3];}
      r[4 * i + j] = v;
    }
  }
  std::memcpy(out, r, sizeof(r));
}

// the inverse of a rigid pose: [R^T | -(R^T t)]
void pose_inverse(const double a[12], double out[12])
{
  double r[12];
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) {r[4 * i + j] = a[4 * j + i];}
    r[4 * i + 3] = -((a[i] * a[3] + a[4 + i] * a[7]) + a[8 + i] * a[11]);
  }
  std::memcpy(out, r, sizeof(r));
}

// whether the windows must follow a scan placed at translation t: for either kind, on any axis, t's voxel lies more than a
// quarter of the window from the window's centre voxel.  false in `ok` where t has no voxel.
bool wants_recentre(const lfx_rolling_map * rm, const double t[3], bool & ok)
{
  bool move = false;
  ok = true;
  for (int k = 0; k < 2; k++) {
    const Store & s = rm->store[k];
    for (int a = 0; a < 3; a++) {
      int32_t v = 0;
      if (!lfx::roll_voxel((float)t[a], s.inv, v)) {ok = false; return false;}
      const int64_t d = (int64_t)v - ((int64_t)s.o[a] + (int64_t)(s.n[a] / 2u));
      if ((d < 0 ? -d : d) > (int64_t)(s.n[a] / 4u)) {move = true;}
    }
  }
  return move;
}

// the box of half extent match_half_extent around t cut out of store `kind` into rm->box[kind] (grown where it must be)
int cut_box(const Call & k, lfx_rolling_map * rm, int kind, const double t[3], uint64_t * n, double lo_m[3], double hi_m[3])
{
  const Store & s = rm->store[kind];
  int32_t vlo[3], vhi[3];
  for (int a = 0; a < 3; a++) {
    vlo[a] = clamped_voxel(t[a] - (double)rm->cfg.match_half_extent[a], s.inv);
    vhi[a] = clamped_voxel(t[a] + (double)rm->cfg.match_half_extent[a], s.inv);
    // the index's bounds: the box's corners padded by one leaf
    lo_m[a] = ((double)vlo[a] - 1.) * (double)s.leaf;
    hi_m[a] = ((double)vhi[a] + 2.) * (double)s.leaf;
  }
  *n = 0;
  lfx::RollBox box{};
  if (!clip_box(s, vlo, vhi, &box)) {return LFX_OK;}
  for (int pass = 0; pass < 2; pass++) {
    LFX_TRY(extract_box(k, rm, kind, box, rm->box[kind].p, rm->box[kind].n, n));
    if (*n <= rm->box[kind].n) {break;}
    // (the buffer is not in use: extract_box has waited)
    if (hold(rm->box[kind], *n) != hipSuccess) {(void)hipGetLastError(); return fail(k.c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the match box");}
  }
  return LFX_OK;
}

int check_store_config(lfx_ctx * c, float leaf, const uint32_t dims[3], const char * name)
{
  if (!(leaf > 0.f) || !std::isfinite(leaf) || !std::isfinite(1.0f / leaf)) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, std::string(name) + "_leaf must be > 0 and finite");
  }
  uint64_t slots = 1;
  for (int a = 0; a < 3; a++) {
    if (dims[a] == 0) {return fail(c, LFX_ERR_INVALID_ARGUMENT, std::string(name) + "_dims must be >= 1");}
    slots *= dims[a];                        // (each factor is below 2^32 and the product is checked after every one)
    if (slots > kMaxSlots) {return fail(c, LFX_ERR_INVALID_ARGUMENT, std::string(name) + "_dims: the window holds more than 2^31 voxels");}
  }
  return LFX_OK;
}
}  // namespace

extern "C" {

void lfx_rolling_map_default_config(lfx_rolling_map_config * cfg)
{
  if (!cfg) {return;}
  *cfg = lfx_rolling_map_config{};
  cfg->edge_leaf = 0.2f;
  cfg->surface_leaf = 0.4f;
  cfg->edge_dims[0] = cfg->edge_dims[1] = 512u; cfg->edge_dims[2] = 128u;
  cfg->surface_dims[0] = cfg->surface_dims[1] = 256u; cfg->surface_dims[2] = 64u;
  cfg->match_half_extent[0] = cfg->match_half_extent[1] = 50.f; cfg->match_half_extent[2] = 12.8f;
  cfg->n_neighbors = 15;
  cfg->max_iter = 20;
  cfg->scan_surface_leaf = 1.0f;
  cfg->edge_cell = cfg->surface_cell = 1.0f;
  std::memcpy(cfg->initial_pose, kIdentityPose, sizeof(kIdentityPose));
}

int lfx_rolling_map_create(lfx_ctx * c, const lfx_rolling_map_config * cfg, lfx_rolling_map ** out)
{
  if (!c || !cfg || !out) {return LFX_ERR_INVALID_ARGUMENT;}
  int rc = check_store_config(c, cfg->edge_leaf, cfg->edge_dims, "edge");
  if (rc == LFX_OK) {rc = check_store_config(c, cfg->surface_leaf, cfg->surface_dims, "surface");}
  if (rc != LFX_OK) {return rc;}
  for (int a = 0; a < 3; a++) {
    if (!(cfg->match_half_extent[a] >= 0.f) || !std::isfinite(cfg->match_half_extent[a])) {
      return fail(c, LFX_ERR_INVALID_ARGUMENT, "match_half_extent must be >= 0 and finite");
    }
  }
  LFX_TRY(check_align_config(c, cfg->n_neighbors, cfg->max_iter, cfg->scan_surface_leaf, "scan_surface_leaf", cfg->edge_cell,
    cfg->surface_cell, cfg->initial_pose));
  LFX_HIP(c, hipSetDevice(c->device));
  lfx_rolling_map * rm = new (std::nothrow) lfx_rolling_map();
  if (!rm) {return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the rolling map");}
  rm->device = c->device;
  rm->cfg = *cfg;
  std::memcpy(rm->pose, cfg->initial_pose, sizeof(rm->pose));
  std::memcpy(rm->correction, kIdentityPose, sizeof(kIdentityPose));
  auto give_up = [&](int code, const std::string & why) {(void)hipGetLastError(); lfx_rolling_map_destroy(rm); return fail(c, code, why);};
  uint64_t most = 0;
  for (int k = 0; k < 2; k++) {
    Store & s = rm->store[k];
    s.leaf = k ? cfg->surface_leaf : cfg->edge_leaf;
    s.inv = 1.0f / s.leaf;
    s.slots = 1;
    for (int a = 0; a < 3; a++) {
      s.n[a] = (k ? cfg->surface_dims : cfg->edge_dims)[a];
      s.o[a] = -(int32_t)(s.n[a] / 2u);
      s.slots *= s.n[a];
    }
    most = std::max(most, s.slots);
    if (s.keys.alloc(s.slots) != hipSuccess || s.stamps.alloc(s.slots) != hipSuccess || s.points.alloc(s.slots) != hipSuccess ||
      s.counters.alloc(lfx::kRollCounters) != hipSuccess)
    {
      return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate a rolling map store of " + std::to_string(s.slots) + " voxels");
    }
  }
  if (rm->partial.alloc((most + lfx::kRollCells - 1u) / lfx::kRollCells) != hipSuccess || rm->total.alloc(1) != hipSuccess ||
    rm->table.alloc(kInitialEntries) != hipSuccess || rm->zero.alloc(4) != hipSuccess)
  {
    return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the rolling map's scratch");
  }
  rm->pin_table = round64(std::max<size_t>(readback_bytes(kInitialEntries, 4), 2 * lfx::kRollCounters * sizeof(uint64_t)));
  if (rm->pinned.reserve(rm->pin_table + sizeof(lfx::RollInsertEntry) * kInitialEntries) != hipSuccess) {
    return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the rolling map's pinned block");
  }
  rm->emap = map_new(c->device);
  rm->smap = map_new(c->device);
  if (!rm->emap || !rm->smap) {return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the match maps");}
  // key 0: never written; stamp 0: older than every bid
  hipError_t e = hipMemset(rm->zero.p, 0, 4 * sizeof(uint32_t));
  for (int k = 0; k < 2 && e == hipSuccess; k++) {
    Store & s = rm->store[k];
    e = hipMemset(s.keys.p, 0, sizeof(uint64_t) * s.slots);
    if (e == hipSuccess) {e = hipMemset(s.stamps.p, 0, sizeof(uint64_t) * s.slots);}
    if (e == hipSuccess) {e = hipMemset(s.counters.p, 0, sizeof(unsigned long long) * lfx::kRollCounters);}
  }
  if (e == hipSuccess) {e = hipDeviceSynchronize();}
  if (e != hipSuccess) {return give_up(LFX_ERR_HIP, hipGetErrorString(e));}
  *out = rm;
  return LFX_OK;
}

void lfx_rolling_map_destroy(lfx_rolling_map * rm) {destroy_with_maps(rm);}

int lfx_rolling_map_recenter(lfx_rolling_map * rm, const double center[3])
{
  if (!rm || !center) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!finite_all(center, 3)) {return LFX_ERR_INVALID_ARGUMENT;}
  int32_t o[2][3];
  for (int k = 0; k < 2; k++) {
    for (int a = 0; a < 3; a++) {
      int32_t v = 0;
      if (!lfx::roll_voxel((float)center[a], rm->store[k].inv, v)) {return LFX_ERR_INVALID_ARGUMENT;}
      o[k][a] = (int32_t)((int64_t)v - (int64_t)(rm->store[k].n[a] / 2u));
    }
  }
  for (int k = 0; k < 2; k++) {
    for (int a = 0; a < 3; a++) {rm->store[k].o[a] = o[k][a];}
  }
  return LFX_OK;
}

int lfx_rolling_map_insert(lfx_ctx * c, lfx_rolling_map * rm, int kind, const float * d_points, const uint32_t * d_begin,
  const uint32_t * d_count, uint32_t count_stride, uint32_t n_clouds, size_t total_points, const double * poses, void * stream)
{
  if (!c || !rm || !d_points || !d_begin || !d_count || !poses) {return LFX_ERR_INVALID_ARGUMENT;}
  if (n_clouds == 0 || count_stride == 0) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "n_clouds and count_stride must be >= 1");}
  if (!finite_all(poses, 12 * (size_t)n_clouds)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the poses must be finite");}
  if (check(c, rm, kind) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.read(rm->tail));
  // the counts and the begins back in one wait: the call's only one
  LFX_TRY(grow_readback(k, rm->tail, rm->pinned, rm->pin_table, readback_bytes(n_clouds, count_stride), sizeof(lfx::RollInsertEntry),
    std::max<size_t>(n_clouds, kInitialEntries)));
  const CloudList list{d_begin, d_count, count_stride, total_points, ""};
  std::vector<uint32_t> begin, count;
  LFX_TRY(read_lists(c, &list, 1, n_clouds, rm->pinned.p, &begin, &count, k.st));
  return insert_clouds(k, rm, kind, reinterpret_cast<const float4 *>(d_points), begin.data(), count.data(), n_clouds, poses);
}

int lfx_rolling_map_insert_host(lfx_ctx * c, lfx_rolling_map * rm, int kind, const float * points, uint32_t n_points,
  const double pose[12], void * stream)
{
  if (!c || !rm || !pose || (n_points && !points)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!finite_all(pose, 12)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the pose must be finite");}
  if (check(c, rm, kind) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (n_points == 0) {return LFX_OK;}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.after(rm->tail));                // (the previous insert may still read the staged cloud)
  if (hold(rm->staged, n_points) != hipSuccess) {(void)hipGetLastError(); return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot stage the cloud");}
  LFX_HIP(c, hipMemcpyAsync(rm->staged.p, points, sizeof(float4) * n_points, hipMemcpyHostToDevice, k.st));
  const uint32_t zero = 0u;
  LFX_TRY(insert_clouds(k, rm, kind, rm->staged.p, &zero, &n_points, 1, pose));
  LFX_HIP(c, hipStreamSynchronize(k.st));      // (the caller's memory is pageable: it has been read when the call returns)
  return LFX_OK;
}

int lfx_rolling_map_extract(lfx_ctx * c, const lfx_rolling_map * rm, int kind, const double lo[3], const double hi[3], float * d_out,
  uint64_t capacity_points, uint64_t * n_points, void * stream)
{
  if (!c || !rm || !lo || !hi || !n_points || (capacity_points && !d_out)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!finite_all(lo, 3) || !finite_all(hi, 3)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the box must be finite");}
  if (check(c, rm, kind) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  const Store & s = rm->store[kind];
  int32_t vlo[3], vhi[3];
  for (int a = 0; a < 3; a++) {vlo[a] = clamped_voxel(lo[a], s.inv); vhi[a] = clamped_voxel(hi[a], s.inv);}
  *n_points = 0;
  lfx::RollBox box{};
  if (!clip_box(s, vlo, vhi, &box)) {return LFX_OK;}
  Call k(c, stream);
  LFX_TRY(k.open());
  return extract_box(k, rm, kind, box, reinterpret_cast<float4 *>(d_out), capacity_points, n_points);
}

int lfx_rolling_map_view(lfx_ctx * c, const lfx_rolling_map * rm, lfx_rolling_map_view_t * v, void * stream)
{
  if (!c || !rm || !v) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check(c, rm, LFX_ROLLING_EDGE) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  Call call(c, stream);
  LFX_TRY(call.open());
  LFX_TRY(call.read(rm->tail));
  hipStream_t const st = call.st;
  lfx_rolling_map_view_t out{};
  uint64_t * h = reinterpret_cast<uint64_t *>(rm->pinned.p);
  for (int k = 0; k < 2; k++) {
    LFX_HIP(c, hipMemcpyAsync(h + lfx::kRollCounters * k, rm->store[k].counters.p, sizeof(uint64_t) * lfx::kRollCounters, hipMemcpyDeviceToHost, st));
  }
  LFX_HIP(c, hipStreamSynchronize(st));
  for (int k = 0; k < 2; k++) {
    const Store & s = rm->store[k];
    const uint64_t * w = h + lfx::kRollCounters * k;
    out.leaf[k] = s.leaf;
    for (int a = 0; a < 3; a++) {out.dims[k][a] = s.n[a]; out.origin[k][a] = s.o[a];}
    out.n_inserted[k] = w[lfx::kRollInserted];
    out.n_merged[k] = w[lfx::kRollInsideCount] - w[lfx::kRollInserted];
    out.n_outside[k] = w[lfx::kRollOutsideCount];
    out.n_nonfinite[k] = w[lfx::kRollNonFiniteCount];
  }
  for (int k = 0; k < 2; k++) {              // (after the counters have been read out of the pinned block)
    lfx::RollBox box{};
    if (whole_window(rm->store[k], &box)) {LFX_TRY(extract_box(call, rm, k, box, nullptr, 0, &out.n_live[k]));}
  }
  std::memcpy(out.pose, rm->pose, sizeof(out.pose));
  std::memcpy(out.correction, rm->correction, sizeof(out.correction));
  *v = out;
  return LFX_OK;
}

int lfx_rolling_map_pose(const lfx_rolling_map * rm, double pose[12])
{
  if (!rm || !pose) {return LFX_ERR_INVALID_ARGUMENT;}
  std::memcpy(pose, rm->pose, sizeof(rm->pose));
  return LFX_OK;
}

int lfx_rolling_map_update_batch(lfx_ctx * c, lfx_rolling_map * rm, uint32_t n_scans, const double * odometry_poses,
  lfx_rolling_map_result * results, void * stream)
{
  if (!c || !rm || !results) {return LFX_ERR_INVALID_ARGUMENT;}
  const int rb = check_last_batch(c, n_scans);
  if (rb != LFX_OK) {return rb;}
  if (odometry_poses && !finite_all(odometry_poses, 12 * (size_t)n_scans)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the odometry poses must be finite");}
  if (check(c, rm, LFX_ROLLING_EDGE) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  Call call(c, stream);
  LFX_TRY(call.open());
  hipStream_t const st = call.st;
  const uint32_t batch = c->last_batch, k = rm->cfg.n_neighbors;
  // the batch's surface clouds downsampled once and every scan's counts, as lfx_odometry_update_batch has them: one wait
  BatchFront f;
  LFX_TRY(batch_front(c, rm->down, 2, false, rm->h_batch, 0, true, rm->cfg.scan_surface_leaf, st, f));
  for (uint32_t s = 0; s < batch; s++) {
    lfx_rolling_map_result r{};
    const double * odom = odometry_poses ? odometry_poses + 12 * (size_t)s : nullptr;
    double initial[12], pose[12];
    if (odom) {pose_compose(rm->correction, odom, initial);} else {std::memcpy(initial, rm->pose, sizeof(initial));}
    if (!finite_all(initial, 12)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the initial pose of scan " + std::to_string(s) + " is not finite");}
    std::memcpy(r.initial_pose, initial, sizeof(initial));
    std::memcpy(pose, initial, sizeof(initial));
    const double t[3] = {initial[3], initial[7], initial[11]};
    bool ok = true;
    if (wants_recentre(rm, t, ok)) {
      ok = lfx_rolling_map_recenter(rm, t) == LFX_OK;
      r.recentered = 1;
    }
    if (!ok) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the initial pose of scan " + std::to_string(s) + " lies outside the voxels a map can name");}
    uint64_t ne = 0, ns = 0;
    double elo[3], ehi[3], slo[3], shi[3];
    // (what the scan queues from here on stands behind the call's record, however the call leaves)
    LFX_TRY(call.behind(rm->tail));
    LFX_TRY(cut_box(call, rm, LFX_ROLLING_EDGE, t, &ne, elo, ehi));
    LFX_TRY(cut_box(call, rm, LFX_ROLLING_SURFACE, t, &ns, slo, shi));
    r.n_edge_map = (uint32_t)ne;
    r.n_surface_map = (uint32_t)ns;
    bool place = true;
    if (ne < k || ns < k) {
      std::memcpy(r.align.pose, initial, sizeof(initial));
      r.align.code = LFX_ALIGN_NOT_RUN;
    } else {
      LFX_TRY(map_rebuild(c, rm->emap, reinterpret_cast<const float *>(rm->box[0].p), (uint32_t)ne, rm->cfg.edge_cell, elo, ehi, st));
      LFX_TRY(map_rebuild(c, rm->smap, reinterpret_cast<const float *>(rm->box[1].p), (uint32_t)ns, rm->cfg.surface_cell, slo, shi, st));
      const uint32_t n_edge = f.info[4 * s + lfx::kInfoEdge];
      const CloudSpan edge{reinterpret_cast<const float *>(c->edge_pts.p), c->scan_begin.p + s, c->scan_info.p + lfx::kInfoEdge + 4 * s, 4,
        n_edge, n_edge, rm->zero.p};
      const CloudSpan surface{f.down, c->scan_begin.p + s, f.down_count + s, 1, f.lengths[2 * s + 1], f.lengths[2 * s + 1], rm->zero.p};
      LFX_TRY(align_clouds(c, rm->emap, rm->smap, k, rm->cfg.max_iter, edge, surface, 1, initial, &r.align, st));
      r.aligned = 1;
      if (LFX_ALIGN_SUCCESS(r.align.code)) {
        std::memcpy(pose, r.align.pose, sizeof(pose));
        if (odom) {
          double inv[12];
          pose_inverse(odom, inv);
          pose_compose(pose, inv, rm->correction);
        }
      } else {
        place = false;                       // the scan stays out of the map; the initial pose is carried on
      }
    }
    if (place) {
      const uint32_t begin = c->h_scan_begin[s];
      LFX_TRY(insert_clouds(call, rm, LFX_ROLLING_EDGE, c->edge_pts.p, &begin, f.info + 4 * s + lfx::kInfoEdge, 1, pose));
      LFX_TRY(insert_clouds(call, rm, LFX_ROLLING_SURFACE, c->surf_pts.p, &begin, f.info + 4 * s + lfx::kInfoSurface, 1, pose));
      r.inserted = 1;
    }
    std::memcpy(rm->pose, pose, sizeof(pose));
    results[s] = r;
  }
  return LFX_OK;
}

int lfx_rolling_map_save(lfx_ctx * c, const lfx_rolling_map * rm, const char * dirname, int written[2], void * stream)
{
  if (!c || !rm || !dirname || !written) {return LFX_ERR_INVALID_ARGUMENT;}
  written[0] = written[1] = 0;
  if (check(c, rm, LFX_ROLLING_EDGE) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  Call call(c, stream);
  LFX_TRY(call.open());
  for (int k = 0; k < 2; k++) {
    lfx::RollBox box{};
    if (!whole_window(rm->store[k], &box)) {continue;}
    uint64_t n = 0, again = 0;
    LFX_TRY(extract_box(call, rm, k, box, nullptr, 0, &n));
    if (n == 0) {continue;}                  // (as lfx_odometry_save: an empty cloud writes no file)
    DevBuf<float4> cloud;
    if (cloud.alloc(n) != hipSuccess) {(void)hipGetLastError(); return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the cloud to save");}
    LFX_TRY(extract_box(call, rm, k, box, cloud.p, n, &again));
    std::vector<float> host(4 * (size_t)n);
    LFX_HIP(c, hipMemcpyAsync(host.data(), cloud.p, sizeof(float) * host.size(), hipMemcpyDeviceToHost, call.st));
    LFX_HIP(c, hipStreamSynchronize(call.st));
    LFX_TRY(write_pcd(c, kind_path(dirname, k), host.data(), n));
    written[k] = 1;
  }
  return LFX_OK;
}

}  // extern "C"
