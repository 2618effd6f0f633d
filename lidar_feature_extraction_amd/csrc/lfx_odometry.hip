// lfx_odometry.hip -- scan-to-local-map odometry: Odometry::Update (odometry.hpp:52-63) over EdgeSurfaceMap
// (edge_surface_map.hpp:38-76) with every cloud on the device (lfx_kernels_odometry.hpp).  The alignment is
// lfx_localize_batch's (align_clouds, lfx_localize.hip); the window maps are lfx_map indexes rebuilt in place.
#include "lfx_internal.hpp"
#include "lfx_kernels_odometry.hpp"

#include <algorithm>
#include <array>

using namespace lfx_host;

namespace
{
struct Box                                   // bounds of one cloud of one scan (the store's coordinates)
{
  double lo[3] = {0., 0., 0.}, hi[3] = {0., 0., 0.};
  bool any = false;
};
}  // namespace

struct lfx_odometry
{
  int device = 0;
  lfx_odometry_config cfg{};
  double pose[12] = {};                      // CurrentPose
  // the store: transformed clouds, scans in insertion order; off_*[j] = first record of retained scan j, [n_scans] = end
  DevBuf<float4> edge, surface;
  std::vector<uint32_t> off_e{0u}, off_s{0u};
  std::vector<std::array<Box, 2>> box;       // per retained scan: edge, surface
  uint64_t added = 0, dropped = 0, compactions = 0;
  lfx_map * emap = nullptr, * smap = nullptr;   // the window maps (map_rebuild)
  DevBuf<uint32_t> bounds;                   // [2][6]: what odometry_append_kernel reduces into
  bool bounds_queued = false;                // the last append's bounds are on their way to the pinned block (settle)
  DevBuf<uint32_t> words;                    // [0] 0 (begin / row begin of a single cloud), [1] n_edge, [2] n_surface, [3] downsampled, [4] status
  DevBuf<float> down;                        // downsampled surface clouds of a batch, then their counts and statuses
  DevBuf<float4> staged;                     // lfx_odometry_update_host: the two clouds, edge first
  PinnedBuf pinned;                          // [12] bounds | [8] words | [batch][4] scan_info | [batch][2] lengths
  bool reports_on = false;                   // lfx_odometry_set_reports
  std::vector<lfx_align_report> reports;     // the scans of the last update* call (a scan that was not aligned: all zero)
  // lfx_odometry_update_batch_deskewed: the poses of the last two scans the update* calls processed ([0] the older one),
  // and the de-skewed clouds of the batch at hand, laid out like the context's
  double recent[2][12] = {};
  uint32_t n_recent = 0;
  DevBuf<float4> dsk_edge, dsk_surface;
  // The work a call leaves queued behind it (the last append, the bounds' copy to the pinned block) is waited for by the
  // next rebuild, or by the next call before it touches the scratch: `tail` is recorded behind it
  Tail tail;
  uint32_t n_scans() const {return (uint32_t)box.size();}
};

namespace
{
constexpr size_t kPinBounds = 0, kPinWords = 12, kPinInfo = 20;

uint32_t * pinned_words(lfx_odometry * o) {return reinterpret_cast<uint32_t *>(o->pinned.p);}

// What lets a scan of (ne, ns) points in: 0 as it is, 1 after the scans older than the window are discarded, -1 not at all
int room(const lfx_odometry * o, uint64_t ne, uint64_t ns)
{
  const uint32_t n = o->n_scans();
  if (o->off_e[n] + ne <= o->cfg.edge_capacity_points && o->off_s[n] + ns <= o->cfg.surface_capacity_points) {return 0;}
  const uint32_t w = std::min(o->cfg.n_local_scans, n);
  const uint64_t ke = o->off_e[n] - o->off_e[n - w], ks = o->off_s[n] - o->off_s[n - w];
  return (ke + ne <= o->cfg.edge_capacity_points && ks + ns <= o->cfg.surface_capacity_points) ? 1 : -1;
}

int no_room(lfx_ctx * c, uint64_t ne, uint64_t ns)
{
  return fail(c, LFX_ERR_INVALID_ARGUMENT, "the scan (" + std::to_string(ne) + " edge, " + std::to_string(ns) +
           " surface points) does not fit the odometry's store beside its window");
}

// the window (the last n_local_scans scans) moved to the front of both stores; the scans before it are discarded.  Moved
// in pieces no longer than the distance moved, so that no copy reads what another one of the same move writes.
int compact(lfx_ctx * c, lfx_odometry * o, hipStream_t st)
{
  const uint32_t n = o->n_scans(), w = std::min(o->cfg.n_local_scans, n), gone = n - w;
  auto move = [&](float4 * p, size_t from, size_t len) -> hipError_t {
      for (size_t at = 0; from && at < len; at += from) {
        const hipError_t e = hipMemcpyAsync(p + at, p + from + at, sizeof(float4) * std::min(from, len - at), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) {return e;}
      }
      return hipSuccess;
    };
  const uint32_t ae = o->off_e[gone], as = o->off_s[gone];
  LFX_HIP(c, move(o->edge.p, ae, o->off_e[n] - ae));
  LFX_HIP(c, move(o->surface.p, as, o->off_s[n] - as));
  o->off_e.erase(o->off_e.begin(), o->off_e.begin() + gone);
  o->off_s.erase(o->off_s.begin(), o->off_s.begin() + gone);
  for (auto & v : o->off_e) {v -= ae;}
  for (auto & v : o->off_s) {v -= as;}
  o->box.erase(o->box.begin(), o->box.begin() + gone);
  o->dropped += gone;
  o->compactions++;
  return LFX_OK;
}

// the tail waited for on the host and taken (a wait only where nothing has waited since; the call records it, however it
// leaves), then the last appended scan's bounds folded into its boxes, once
int settle(Call & call, lfx_odometry * o)
{
  LFX_TRY(call.after(o->tail));
  if (!o->bounds_queued) {return LFX_OK;}
  o->bounds_queued = false;
  const uint32_t * h = pinned_words(o) + kPinBounds;
  std::array<Box, 2> & b = o->box.back();
  for (int k = 0; k < 2; k++) {
    const uint32_t * v = h + 6 * k;
    b[k].any = v[3] != 0u;
    for (int a = 0; a < 3 && b[k].any; a++) {b[k].lo[a] = lfx::float_of_order(~v[a]); b[k].hi[a] = lfx::float_of_order(v[3 + a]);}
  }
  return LFX_OK;
}

// EdgeSurfaceMap::Add: both clouds transformed by `pose` behind the store's last scan (after a compaction where `how` says
// so), and the call's record behind it.  Nothing is waited for: the bounds are read by the next rebuild (settle)
int append(Call & k, lfx_odometry * o, int how, const double pose[12], const float4 * edge, uint32_t ne, const float4 * surface, uint32_t ns)
{
  lfx_ctx * const c = k.c;
  hipStream_t const st = k.st;
  LFX_TRY(settle(k, o));                     // (the bounds table is about to be written again)
  if (how == 1) {LFX_TRY(compact(c, o, st));}
  const uint32_t n = o->n_scans(), at_e = o->off_e[n], at_s = o->off_s[n];
  if (ne + ns) {
    lfx::OdoPose P;
    for (int i = 0; i < 12; i++) {P.m[i] = pose[i];}
    const uint32_t ge = (ne + lfx::kAppendThreads - 1u) / lfx::kAppendThreads, gs = (ns + lfx::kAppendThreads - 1u) / lfx::kAppendThreads;
    LFX_HIP(c, hipMemsetAsync(o->bounds.p, 0, 12 * sizeof(uint32_t), st));
    hipLaunchKernelGGL(lfx::odometry_append_kernel, dim3(ge + gs), dim3(lfx::kAppendThreads), 0, st, P, edge, ne, surface, ns,
      o->edge.p + at_e, o->surface.p + at_s, ge, o->bounds.p);
    LFX_HIP(c, hipGetLastError());
    LFX_HIP(c, hipMemcpyAsync(pinned_words(o) + kPinBounds, o->bounds.p, 12 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  }
  o->off_e.push_back(at_e + ne);
  o->off_s.push_back(at_s + ns);
  o->box.push_back(std::array<Box, 2>{});
  LFX_TRY(k.finish());
  o->bounds_queued = ne + ns > 0;
  o->added++;
  return LFX_OK;
}

// one window map over the last w scans of a store
int rebuild(Call & call, lfx_odometry * o, int k, uint32_t w)
{
  lfx_ctx * const c = call.c;
  LFX_TRY(settle(call, o));
  const uint32_t n = o->n_scans();
  const std::vector<uint32_t> & off = k ? o->off_s : o->off_e;
  double lo[3] = {0., 0., 0.}, hi[3] = {0., 0., 0.};
  bool any = false;
  for (uint32_t j = n - w; j < n; j++) {
    const Box & b = o->box[j][k];
    if (!b.any) {continue;}
    for (int a = 0; a < 3; a++) {
      lo[a] = any ? std::min(lo[a], b.lo[a]) : b.lo[a];
      hi[a] = any ? std::max(hi[a], b.hi[a]) : b.hi[a];
    }
    any = true;
  }
  for (int a = 0; a < 3; a++) {
    if (!std::isfinite(lo[a]) || !std::isfinite(hi[a])) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the window holds a point that is not finite");}
  }
  const float4 * store = k ? o->surface.p : o->edge.p;
  return map_rebuild(c, k ? o->smap : o->emap, reinterpret_cast<const float *>(store + off[n - w]), off[n] - off[n - w],
           k ? o->cfg.surface_cell : o->cfg.edge_cell, lo, hi, call.st);
}

struct ScanIn                                // one scan as the append kernel and the alignment read it
{
  const float4 * edge = nullptr, * surface = nullptr;    // the raw clouds
  uint32_t n_edge = 0, n_surface = 0;
  CloudSpan edge_cloud, down_cloud;                      // the edge cloud and the downsampled surface cloud as align_clouds addresses them
};

// one cloud of n points (or a bound on them) whose rows start at row 0 (the odometry's words hold a 0 first)
CloudSpan single_cloud(const lfx_odometry * o, const float * points, const uint32_t * begin, const uint32_t * count, uint32_t stride, uint32_t n)
{
  return CloudSpan{points, begin, count, stride, n, n, o->words.p};
}

void not_aligned(const double pose[12], lfx_odometry_result * r)
{
  for (int i = 0; i < 12; i++) {r->align.pose[i] = pose[i];}
  r->align.error = 0.; r->align.error_scale = 0.; r->align.iteration = 0; r->align.code = LFX_ALIGN_NOT_RUN;
  r->aligned = 0;
}

// Odometry::Update for one scan
int step(Call & call, lfx_odometry * o, const ScanIn & in, lfx_odometry_result * result, lfx_align_report * report)
{
  lfx_ctx * const c = call.c;
  const int how = room(o, in.n_edge, in.n_surface);
  if (how < 0) {return no_room(c, in.n_edge, in.n_surface);}
  lfx_odometry_result r{};
  double pose[12];
  std::memcpy(pose, o->pose, sizeof(pose));
  const uint32_t n = o->n_scans(), w = std::min(o->cfg.n_local_scans, n), k = o->cfg.n_neighbors;
  if (o->added == 0) {
    not_aligned(pose, &r);                   // IsEmpty: the scan is added at the current pose
  } else {
    r.n_edge_map = o->off_e[n] - o->off_e[n - w];
    r.n_surface_map = o->off_s[n] - o->off_s[n - w];
    if (r.n_edge_map < k || r.n_surface_map < k) {
      not_aligned(pose, &r);                 // (the reference would read nanoflann's uninitialised output)
    } else {
      LFX_TRY(rebuild(call, o, 0, w));
      LFX_TRY(rebuild(call, o, 1, w));
      LFX_TRY(align_clouds(c, o->emap, o->smap, k, o->cfg.max_iter, in.edge_cloud, in.down_cloud, 1, o->pose, &r.align, call.st, report));
      std::memcpy(pose, r.align.pose, sizeof(pose));    // pose_ = update(scan, pose_), whatever the code
      r.aligned = 1;
    }
  }
  LFX_TRY(append(call, o, how, pose, in.edge, in.n_edge, in.surface, in.n_surface));
  std::memcpy(o->pose, pose, sizeof(pose));
  std::memcpy(o->recent[0], o->recent[1], sizeof(pose));
  std::memcpy(o->recent[1], pose, sizeof(pose));
  o->n_recent = std::min(o->n_recent + 1u, 2u);
  *result = r;
  return LFX_OK;
}

int check(lfx_ctx * c, const lfx_odometry * o) {return check_device(c, o->device, "the odometry");}

// the reports of a call over n scans: one per scan, all zero, where reports are on; null where they are off
lfx_align_report * fresh_reports(lfx_odometry * o, uint32_t n)
{
  o->reports.assign(o->reports_on ? n : 0u, lfx_align_report{});
  return o->reports_on ? o->reports.data() : nullptr;
}

// Odometry::Update for one scan whose clouds are on the device: lfx_odometry_update behind its checks, and what every
// other update call runs per scan
int update_scan(Call & k, lfx_odometry * o, const float * d_edge, uint32_t n_edge, const float * d_surface, uint32_t n_surface,
  lfx_odometry_result * result, lfx_align_report * report)
{
  LFX_TRY(settle(k, o));                     // (the pinned words are about to be written again)
  if (hold(o->down, 4 * (size_t)n_surface + 4) != hipSuccess) {return fail(k.c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the downsampled surface cloud");}
  // Nothing is waited for: the downsampled cloud's rows are sized by the cloud's own length, as lfx_localize_batch sizes a
  // few scans' rows.  (align_clouds wants a pointer for an empty edge cloud too.)
  ScanIn in;
  in.edge = reinterpret_cast<const float4 *>(d_edge); in.n_edge = n_edge;
  in.surface = reinterpret_cast<const float4 *>(d_surface); in.n_surface = n_surface;
  LFX_TRY(scan_front(k.c, pinned_words(o) + kPinWords, o->words.p, d_edge ? d_edge : o->down.p, n_edge, d_surface, n_surface,
    o->cfg.surface_leaf, o->down.p, o->words.p, k.st, in.edge_cloud, in.down_cloud));
  return step(k, o, in, result, report);
}

// What the de-skewing batch calls do once their arguments are checked: every scan of the last batch through update_scan,
// its clouds de-skewed just ahead of it by queue(s), which queues scan s's de-skew into dsk_edge / dsk_surface (laid out
// like the context's clouds) on the stream.
template<typename Queue>
int update_deskewed(lfx_ctx * c, lfx_odometry * o, lfx_odometry_result * results, void * stream, Queue queue)
{
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(settle(k, o));
  const uint32_t batch = c->last_batch;
  const size_t total = c->h_scan_begin[batch];
  if (hold(o->dsk_edge, total + 1) != hipSuccess || hold(o->dsk_surface, total + 1) != hipSuccess) {
    return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the de-skewed clouds");
  }
  // (update_scan writes the pinned block's words and bounds, not the batch's scan_info behind them)
  BatchFront f;
  LFX_TRY(f.pin(c, o->pinned, kPinInfo, true));
  LFX_TRY(f.read_info(c, k.st));
  lfx_align_report * const reports = fresh_reports(o, batch);
  for (uint32_t s = 0; s < batch; s++) {
    LFX_TRY(k.take(o->tail));                // (the de-skew reads and writes the odometry's clouds: behind the call's record too)
    LFX_TRY(queue(s));
    const uint32_t b = c->h_scan_begin[s];
    LFX_TRY(update_scan(k, o, reinterpret_cast<const float *>(o->dsk_edge.p + b), f.info[4 * s + lfx::kInfoEdge],
      reinterpret_cast<const float *>(o->dsk_surface.p + b), f.info[4 * s + lfx::kInfoSurface], results + s, reports ? reports + s : nullptr));
  }
  return LFX_OK;
}
}  // namespace

const Tail & lfx_host::odometry_tail(const lfx_odometry * o) {return o->tail;}

extern "C" {

void lfx_odometry_default_config(lfx_odometry_config * cfg)
{
  if (!cfg) {return;}
  *cfg = lfx_odometry_config{};
  cfg->n_local_scans = 7;                    // app/odometry.cpp
  cfg->n_neighbors = 15;                     // N_NEIGHBORS
  cfg->max_iter = 20;                        // Optimizer's default
  cfg->surface_leaf = 1.0f;
  cfg->edge_cell = cfg->surface_cell = 1.0f;
  cfg->edge_capacity_points = cfg->surface_capacity_points = (uint64_t)1 << 22;
  std::memcpy(cfg->initial_pose, kIdentityPose, sizeof(kIdentityPose));
}

int lfx_odometry_create(lfx_ctx * c, const lfx_odometry_config * cfg, lfx_odometry ** out)
{
  if (!c || !cfg || !out) {return LFX_ERR_INVALID_ARGUMENT;}
  if (cfg->n_local_scans == 0) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "n_local_scans must be >= 1");}
  if (cfg->edge_capacity_points == 0 || cfg->surface_capacity_points == 0 || cfg->edge_capacity_points > 0xFFFFFFFFull ||
    cfg->surface_capacity_points > 0xFFFFFFFFull)
  {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "the store's capacities must be in [1, 2^32 - 1] points");
  }
  LFX_TRY(check_align_config(c, cfg->n_neighbors, cfg->max_iter, cfg->surface_leaf, "surface_leaf", cfg->edge_cell, cfg->surface_cell,
    cfg->initial_pose));
  LFX_HIP(c, hipSetDevice(c->device));
  lfx_odometry * o = new (std::nothrow) lfx_odometry();
  if (!o) {return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the odometry");}
  o->device = c->device;
  o->cfg = *cfg;
  std::memcpy(o->pose, cfg->initial_pose, sizeof(o->pose));
  auto give_up = [&](int code, const std::string & why) {lfx_odometry_destroy(o); return fail(c, code, why);};
  o->emap = map_new(c->device);
  o->smap = map_new(c->device);
  if (!o->emap || !o->smap) {return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the window maps");}
  if (o->edge.alloc(cfg->edge_capacity_points) != hipSuccess) {return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the edge store");}
  if (o->surface.alloc(cfg->surface_capacity_points) != hipSuccess) {return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the surface store");}
  if (o->bounds.alloc(12) != hipSuccess) {return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the odometry's bounds");}
  if (o->words.alloc(kScanWords) != hipSuccess) {return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the odometry's words");}
  if (o->pinned.reserve(sizeof(uint32_t) * (kPinInfo + 6 * (size_t)std::max(c->max_batch, 1u))) != hipSuccess) {
    return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the odometry's pinned block");
  }
  hipError_t e = hipMemset(o->words.p, 0, kScanWords * sizeof(uint32_t));
  if (e == hipSuccess) {e = hipDeviceSynchronize();}
  if (e != hipSuccess) {return give_up(LFX_ERR_HIP, hipGetErrorString(e));}
  *out = o;
  return LFX_OK;
}

void lfx_odometry_destroy(lfx_odometry * o) {destroy_with_maps(o);}

int lfx_odometry_update_batch(lfx_ctx * c, lfx_odometry * o, uint32_t n_scans, lfx_odometry_result * results, void * stream)
{
  if (!c || !o || !results) {return LFX_ERR_INVALID_ARGUMENT;}
  const int rb = check_last_batch(c, n_scans);
  if (rb != LFX_OK) {return rb;}
  if (check(c, o) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(settle(k, o));
  const uint32_t batch = c->last_batch;
  lfx_align_report * const reports = fresh_reports(o, batch);
  // the batch's surface clouds downsampled once and every scan's counts: one wait for the whole batch
  BatchFront f;
  LFX_TRY(batch_front(c, o->down, 2, false, o->pinned, kPinInfo, true, o->cfg.surface_leaf, k.st, f));
  for (uint32_t s = 0; s < batch; s++) {
    ScanIn in;
    const uint32_t b = c->h_scan_begin[s];
    in.edge = c->edge_pts.p + b; in.n_edge = f.info[4 * s + lfx::kInfoEdge];
    in.surface = c->surf_pts.p + b; in.n_surface = f.info[4 * s + lfx::kInfoSurface];
    in.edge_cloud = single_cloud(o, reinterpret_cast<const float *>(c->edge_pts.p), c->scan_begin.p + s,
      c->scan_info.p + lfx::kInfoEdge + 4 * s, 4, in.n_edge);
    in.down_cloud = single_cloud(o, f.down, c->scan_begin.p + s, f.down_count + s, 1, f.lengths[2 * s + 1]);
    LFX_TRY(step(k, o, in, results + s, reports ? reports + s : nullptr));
  }
  return LFX_OK;
}

int lfx_odometry_update(lfx_ctx * c, lfx_odometry * o, const float * d_edge, uint32_t n_edge, const float * d_surface,
  uint32_t n_surface, lfx_odometry_result * result, void * stream)
{
  if (!c || !o || !result || (n_edge && !d_edge) || (n_surface && !d_surface)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check(c, o) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  Call k(c, stream);
  LFX_TRY(k.open());
  return update_scan(k, o, d_edge, n_edge, d_surface, n_surface, result, fresh_reports(o, 1));
}

int lfx_odometry_update_batch_deskewed(lfx_ctx * c, lfx_odometry * o, const lfx_time_field * time, const double * sweep_times,
  double sweep_ratio, int to, uint32_t n_scans, lfx_odometry_result * results, void * stream)
{
  if (!c || !o || !results || !time) {return LFX_ERR_INVALID_ARGUMENT;}
  const int rb = check_last_batch(c, n_scans);
  if (rb != LFX_OK) {return rb;}
  if (check(c, o) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (c->deskewed_in_place) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the last batch has already been de-skewed in place");}
  if (!std::isfinite(sweep_ratio)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "sweep_ratio must be finite");}
  if (time->source != LFX_TIME_FROM_INDEX && !sweep_times) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "sweep_times is required with a time field");}
  // (recent[] is read per scan: the scan before has been through its update by then)
  return update_deskewed(c, o, results, stream, [&](uint32_t s) {
             lfx_sweep sw{};
             double D[12];
             if (o->n_recent < 2u) {std::memcpy(D, kIdentityPose, sizeof(D));} else {lfx_motion_between(o->recent[0], o->recent[1], D);}
             lfx_motion_scale(D, sweep_ratio, sw.motion);
             if (sweep_times) {sw.t0 = sweep_times[2 * s]; sw.t1 = sweep_times[2 * s + 1];}
             return deskew_scans(c, time, &sw, s, 1, to, o->dsk_edge.p, o->dsk_surface.p, static_cast<hipStream_t>(stream));
           });
}

// lfx_odometry_update_batch_deskewed with the caller's trajectories in place of the prediction.  Every trajectory is checked
// before the first scan is touched: a refusal leaves the store as it was.
int lfx_odometry_update_batch_trajectory(lfx_ctx * c, lfx_odometry * o, const lfx_time_field * time, const lfx_trajectory * trajectories,
  uint32_t n_scans, lfx_odometry_result * results, void * stream)
{
  if (!c || !o || !results || !time || !trajectories) {return LFX_ERR_INVALID_ARGUMENT;}
  const int rb = check_last_batch(c, n_scans);
  if (rb != LFX_OK) {return rb;}
  if (check(c, o) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (c->deskewed_in_place) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the last batch has already been de-skewed in place");}
  const int rt = check_trajectories(c, trajectories, n_scans);
  if (rt != LFX_OK) {return rt;}
  return update_deskewed(c, o, results, stream, [&](uint32_t s) {
             return deskew_scans_trajectory(c, time, trajectories + s, s, 1, o->dsk_edge.p, o->dsk_surface.p, static_cast<hipStream_t>(stream));
           });
}

int lfx_odometry_update_host(lfx_ctx * c, lfx_odometry * o, const float * edge, uint32_t n_edge, const float * surface,
  uint32_t n_surface, lfx_odometry_result * result, void * stream)
{
  if (!c || !o || !result || (n_edge && !edge) || (n_surface && !surface)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check(c, o) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(settle(k, o));                     // (the previous call may still read the staged clouds)
  if (hold(o->staged, (size_t)n_edge + n_surface + 1) != hipSuccess) {return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot stage the scan's clouds");}
  if (n_edge) {LFX_HIP(c, hipMemcpyAsync(o->staged.p, edge, sizeof(float4) * n_edge, hipMemcpyHostToDevice, k.st));}
  if (n_surface) {LFX_HIP(c, hipMemcpyAsync(o->staged.p + n_edge, surface, sizeof(float4) * n_surface, hipMemcpyHostToDevice, k.st));}
  return update_scan(k, o, reinterpret_cast<const float *>(o->staged.p), n_edge, reinterpret_cast<const float *>(o->staged.p + n_edge),
           n_surface, result, fresh_reports(o, 1));
}

int lfx_odometry_add(lfx_ctx * c, lfx_odometry * o, const double pose[12], const float * d_edge, uint32_t n_edge,
  const float * d_surface, uint32_t n_surface, void * stream)
{
  if (!c || !o || !pose || (n_edge && !d_edge) || (n_surface && !d_surface)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check(c, o) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  const int how = room(o, n_edge, n_surface);
  if (how < 0) {return no_room(c, n_edge, n_surface);}
  Call k(c, stream);
  LFX_TRY(k.open());
  return append(k, o, how, pose, reinterpret_cast<const float4 *>(d_edge), n_edge, reinterpret_cast<const float4 *>(d_surface), n_surface);
}

int lfx_odometry_set_reports(lfx_odometry * o, int on)
{
  if (!o) {return LFX_ERR_INVALID_ARGUMENT;}
  o->reports_on = on != 0;
  if (!o->reports_on) {o->reports.clear();}
  return LFX_OK;
}

int lfx_odometry_reports(const lfx_odometry * o, lfx_align_report * out, uint32_t capacity, uint32_t * n)
{
  if (!o || !n || (capacity && !out)) {return LFX_ERR_INVALID_ARGUMENT;}
  *n = (uint32_t)o->reports.size();
  const uint32_t take = std::min(capacity, *n);
  if (take) {std::memcpy(out, o->reports.data(), sizeof(lfx_align_report) * take);}
  return LFX_OK;
}

int lfx_odometry_pose(const lfx_odometry * o, double pose[12])
{
  if (!o || !pose) {return LFX_ERR_INVALID_ARGUMENT;}
  std::memcpy(pose, o->pose, sizeof(o->pose));
  return LFX_OK;
}

int lfx_odometry_view(const lfx_odometry * o, lfx_odometry_store_view * v)
{
  if (!o || !v) {return LFX_ERR_INVALID_ARGUMENT;}
  const uint32_t n = o->n_scans(), w = std::min(o->cfg.n_local_scans, n);
  *v = lfx_odometry_store_view{};
  v->n_scans = n;
  v->n_window_scans = w;
  v->n_added = o->added;
  v->dropped_scans = o->dropped;
  v->compactions = o->compactions;
  v->edge_points = reinterpret_cast<const float *>(o->edge.p);
  v->surface_points = reinterpret_cast<const float *>(o->surface.p);
  v->n_edge = o->off_e[n];
  v->n_surface = o->off_s[n];
  v->edge_window = reinterpret_cast<const float *>(o->edge.p + o->off_e[n - w]);
  v->surface_window = reinterpret_cast<const float *>(o->surface.p + o->off_s[n - w]);
  v->n_edge_window = o->off_e[n] - o->off_e[n - w];
  v->n_surface_window = o->off_s[n] - o->off_s[n - w];
  v->edge_offsets = o->off_e.data();
  v->surface_offsets = o->off_s.data();
  std::memcpy(v->pose, o->pose, sizeof(o->pose));
  return LFX_OK;
}

}  // extern "C"
