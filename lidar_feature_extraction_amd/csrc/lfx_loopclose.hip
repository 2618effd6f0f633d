// lfx_loopclose.hip -- the loop closer (include/lfx.h, the loop closer section): host orchestration over the public calls of
// the place index, the keyframe store, the alignment and the pose graph.  No kernel of its own: what it returns are those
// calls' bytes, so a caller that composes them by hand gets the same.  What it reads past the public boundary: where the
// index keeps its descriptors (place_db_entries: a detect's queries are the index's own entries), and whether the store has
// reserved flags (keyframes_access: lfx_loop_closer_set_masked has no context to ask through).
#include "lfx_internal.hpp"

#include <algorithm>
#include <cstdint>

using namespace lfx_host;

struct lfx_loop_closer
{
  int device = 0;
  lfx_loop_closer_config cfg{};
  lfx_keyframes * keyframes = nullptr;
  lfx_place_db * db = nullptr;
  lfx_pose_graph * graph = nullptr;
  bool masked = false;                       // lfx_loop_closer_set_masked: the submaps leave the store's flagged records out
  uint64_t ds_capacity = 0;                  // records of `downsampled`
  uint64_t device_bytes = 0;
  DevBuf<float> submap[2];                   // [submap_capacity[kind]][4]
  DevBuf<float> downsampled;                 // [ds_capacity][4]: the query's surface cloud after the voxel grid
  DevBuf<uint32_t> words;                    // kScanWords: what the clouds' begin / count arguments point at
  PinnedBuf h_words;
};

namespace
{
// the smallest of the store's, the index's and the graph's sizes: the ids the contract covers
int common_size(lfx_ctx * c, const lfx_loop_closer * lc, uint32_t & n)
{
  lfx_keyframes_info_t ki{};
  lfx_pose_graph_info_t gi{};
  uint32_t entries = 0;
  if (lfx_keyframes_info(lc->keyframes, &ki) != LFX_OK || lfx_place_db_size(lc->db, &entries) != LFX_OK || lfx_pose_graph_info(lc->graph, &gi) != LFX_OK) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "the loop closer's store, index or graph cannot be read");
  }
  n = std::min(ki.n_keyframes, std::min(entries, gi.n_nodes));
  return LFX_OK;
}

int check_range(lfx_ctx * c, const lfx_loop_closer * lc, uint32_t first, uint32_t count)
{
  uint32_t n = 0;
  int rc = check_device(c, lc->device, "the loop closer");
  if (rc == LFX_OK) {rc = common_size(c, lc, n);}
  if (rc != LFX_OK) {return rc;}
  if (count == 0 || first >= n || count > n - first) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "keyframes " + std::to_string(first) + " .. + " + std::to_string(count) + " are not all below " +
             std::to_string(n) + ", the smallest of the store's, the index's and the graph's sizes");
  }
  return LFX_OK;
}

// the records of keyframes [first, first + count) of `kind`, from the store's host mirror: a build without room queues
// nothing and reports the records needed
int range_points(lfx_ctx * c, const lfx_loop_closer * lc, int kind, uint32_t first, uint32_t count, uint64_t & n)
{
  n = 0;
  const int rc = lfx_keyframes_build(c, lc->keyframes, kind, first, count, nullptr, 0, &n, nullptr);
  return rc == LFX_ERR_CAPACITY ? LFX_OK : rc;
}

int reject(lfx_loop_closure * out, int reason)
{
  out->accepted = 0;
  out->reason = reason;
  return LFX_OK;
}

// the acceptance tests on a closure whose alignment has run, in the header's order
int judge(const lfx_loop_closer_config & cfg, const lfx_loop_closure & cl)
{
  const lfx_align_report & r = cl.report;
  if (!(LFX_ALIGN_SUCCESS(cl.result.code) || cl.result.code == LFX_ALIGN_MAX_ITERATION)) {return LFX_LOOP_ALIGN_FAILED;}
  if (!r.valid) {return LFX_LOOP_NO_REPORT;}
  if (r.rank != 6) {return LFX_LOOP_RANK;}
  if (cfg.reject_degenerate && r.degenerate) {return LFX_LOOP_DEGENERATE;}
  if (!(r.rms_edge <= cfg.max_rms_edge)) {return LFX_LOOP_RMS_EDGE;}
  if (!(r.rms_surface <= cfg.max_rms_surface)) {return LFX_LOOP_RMS_SURFACE;}
  const double residuals = (double)r.n_edge + (double)r.n_surface, inliers = (double)r.n_edge_inliers + (double)r.n_surface_inliers;
  if (!(inliers / residuals >= cfg.min_inlier_share)) {return LFX_LOOP_INLIERS;}
  if (cfg.scale_by_sigma2 && !(std::isfinite(r.sigma2) && r.sigma2 > 0.0)) {return LFX_LOOP_SIGMA2;}
  return LFX_LOOP_ACCEPTED;
}

// steps 2 to 4 of a verification, between the creation of the maps and their destruction
int align_query(lfx_ctx * c, lfx_loop_closer * lc, const lfx_map * edge_map, const lfx_map * surface_map, const float * edge, uint32_t n_edge,
  const float * surface, uint32_t n_surface, const double initial[12], lfx_loop_closure * out, hipStream_t st)
{
  uint32_t * h = reinterpret_cast<uint32_t *>(lc->h_words.p);
  uint32_t * w = lc->words.p;
  h[kScanZero] = 0u; h[kScanEdgeCount] = n_edge; h[kScanSurfaceCount] = n_surface;
  LFX_HIP(c, hipMemcpyAsync(w, h, sizeof(uint32_t) * 3u, hipMemcpyHostToDevice, st));
  const float * scan_surface = surface;
  const uint32_t * scan_count = w + kScanSurfaceCount;
  uint32_t n_scan = n_surface;
  if (lc->cfg.surface_leaf > 0.0f) {
    const int rd = lfx_voxel_downsample(c, surface, w + kScanZero, w + kScanSurfaceCount, 1u, 1u, n_surface, lc->cfg.surface_leaf, lc->downsampled.p,
        w + kScanDownCount, w + kScanDownStatus, st);
    if (rd != LFX_OK) {return rd;}
    LFX_HIP(c, hipMemcpyAsync(h + kScanDownCount, w + kScanDownCount, sizeof(uint32_t) * 2u, hipMemcpyDeviceToHost, st));
    LFX_HIP(c, hipStreamSynchronize(st));
    if (h[kScanDownStatus] == 0u) {                          // (1: the leaf is too small for the cloud, which is used as stored)
      scan_surface = lc->downsampled.p;
      scan_count = w + kScanDownCount;
      n_scan = h[kScanDownCount];
    }
  }
  return lfx_scan_to_map_align_report(c, edge_map, surface_map, lc->cfg.n_neighbors, lc->cfg.max_iter, edge, w + kScanZero, w + kScanEdgeCount, 1u, n_edge,
           n_edge, scan_surface, w + kScanZero, scan_count, 1u, n_scan, n_scan, 1u, initial, &out->result, &out->report, st);
}

// one verification; the ids have been checked
int verify_one(lfx_ctx * c, lfx_loop_closer * lc, uint32_t q, const lfx_place_match & cand, lfx_loop_closure * out, hipStream_t st)
{
  const lfx_loop_closer_config & cfg = lc->cfg;
  const uint32_t cnd = cand.entry;
  std::memset(out, 0, sizeof(*out));
  out->query = q;
  out->candidate = cnd;
  out->match = cand;
  double pose_c[12];
  int rc = lfx_keyframes_poses(c, lc->keyframes, cnd, 1u, pose_c, st);
  if (rc != LFX_OK) {return rc;}
  // 1. the submaps: the candidate's neighbours in id and in space, the query's recent past left out
  const uint32_t w = cfg.submap_half_window;
  const uint32_t lo = cnd > w ? cnd - w : 0u;
  const uint32_t hi = (uint32_t)std::min<uint64_t>((uint64_t)cnd + w, q - cfg.min_gap);
  const double center[3] = {pose_c[3], pose_c[7], pose_c[11]};
  for (int kind = 0; kind < 2; kind++) {
    rc = (lc->masked ? lfx_keyframes_submap_masked : lfx_keyframes_submap)(c, lc->keyframes, kind, center, cfg.submap_radius, lo, hi + 1u - lo,
        lc->submap[kind].p, cfg.submap_capacity[kind], &out->submap[kind], st);
    if (rc != LFX_OK) {return rc;}
  }
  uint64_t begin[2], count[2];
  for (int kind = 0; kind < 2; kind++) {
    rc = range_points(c, lc, kind, 0u, q, begin[kind]);
    if (rc == LFX_OK) {rc = range_points(c, lc, kind, q, 1u, count[kind]);}
    if (rc != LFX_OK) {return rc;}
  }
  if (count[0] == 0u || count[1] == 0u) {return reject(out, LFX_LOOP_EMPTY_QUERY);}
  if (out->submap[0].n_points == 0u || out->submap[1].n_points == 0u) {return reject(out, LFX_LOOP_EMPTY_SUBMAP);}
  if (count[0] > UINT32_MAX || count[1] > UINT32_MAX) {return fail(c, LFX_ERR_CAPACITY, "keyframe " + std::to_string(q) + " has 2^32 records or more");}
  if (cfg.surface_leaf > 0.0f && count[1] > lc->ds_capacity) {
    return fail(c, LFX_ERR_CAPACITY, "keyframe " + std::to_string(q) + " has " + std::to_string(count[1]) + " surface records: the loop closer's "
             "downsample output holds " + std::to_string(lc->ds_capacity) + " (downsample_capacity)");
  }
  lfx_keyframes_store_view view{};
  rc = lfx_keyframes_view(c, lc->keyframes, &view, st);
  if (rc != LFX_OK) {return rc;}
  // 4.'s initial pose: pose_c x Rz(yaw)
  const double cs = std::cos(cand.yaw), sn = std::sin(cand.yaw);
  double initial[12];
  for (int r = 0; r < 3; r++) {
    const double r0 = pose_c[4 * r], r1 = pose_c[4 * r + 1];
    initial[4 * r] = r0 * cs + r1 * sn;
    initial[4 * r + 1] = -r0 * sn + r1 * cs;
    initial[4 * r + 2] = pose_c[4 * r + 2];
    initial[4 * r + 3] = pose_c[4 * r + 3];
  }
  // 2. the maps, gone again before the call returns
  lfx_map * maps[2] = {nullptr, nullptr};
  for (int kind = 0; kind < 2 && rc == LFX_OK; kind++) {
    rc = lfx_map_create(c, lc->submap[kind].p, (uint32_t)out->submap[kind].n_points, cfg.map_cell_size, &maps[kind], st);
  }
  if (rc == LFX_OK) {
    rc = align_query(c, lc, maps[0], maps[1], view.points[0] + 4u * begin[0], (uint32_t)count[0], view.points[1] + 4u * begin[1],
        (uint32_t)count[1], initial, out, st);
  }
  lfx_map_destroy(maps[0]);
  lfx_map_destroy(maps[1]);
  if (rc != LFX_OK) {return rc;}
  out->reason = judge(cfg, *out);
  out->accepted = out->reason == LFX_LOOP_ACCEPTED ? 1 : 0;
  const bool ran = LFX_ALIGN_SUCCESS(out->result.code) || out->result.code == LFX_ALIGN_MAX_ITERATION;
  if (ran && out->report.valid) {
    lfx_pose_graph_edge & e = out->edge;
    e.i = cnd; e.j = q; e.flags = LFX_EDGE_ROBUST;
    (void)lfx_motion_between(pose_c, out->result.pose, e.z);
    (void)lfx_pose_graph_edge_information(out->result.pose, out->report.information, e.information);
    const double s2 = out->report.sigma2;
    if (cfg.scale_by_sigma2 && std::isfinite(s2) && s2 > 0.0) {
      for (double & v : e.information) {v = v / s2;}
    }
  }
  return LFX_OK;
}

int detect(lfx_ctx * c, lfx_loop_closer * lc, uint32_t first, uint32_t count, lfx_place_match * candidates, uint32_t * n_eligible, hipStream_t st)
{
  const lfx_loop_closer_config & cfg = lc->cfg;
  if (count > 65535u) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "at most 65535 keyframes to a call");}
  std::vector<lfx_place_gate> gates(count);
  for (uint32_t s = 0; s < count; s++) {
    const uint32_t q = first + s;
    gates[s].limit = q >= cfg.min_gap ? q - cfg.min_gap + 1u : 0u;
    gates[s].pose = q;
  }
  lfx_keyframes_store_view view{};
  int rc = lfx_keyframes_view(c, lc->keyframes, &view, st);
  if (rc != LFX_OK) {return rc;}
  uint32_t cells = 0;
  const float * entries = place_db_entries(lc->db, &cells);
  rc = lfx_place_db_query_gated(c, lc->db, entries + (size_t)first * cells, count, gates.data(), view.poses, cfg.search_radius, cfg.n_candidates,
      candidates, n_eligible, st);
  if (rc != LFX_OK) {return rc;}
  for (size_t i = 0; i < (size_t)count * cfg.n_candidates; i++) {
    if (candidates[i].distance > cfg.max_distance) {candidates[i] = lfx_place_match{UINT32_MAX, 0u, std::numeric_limits<double>::infinity(), 0.0};}
  }
  return LFX_OK;
}
}  // namespace

extern "C" {

void lfx_loop_closer_default_config(lfx_loop_closer_config * cfg)
{
  if (!cfg) {return;}
  std::memset(cfg, 0, sizeof(*cfg));
  const double inf = std::numeric_limits<double>::infinity();
  cfg->min_gap = 50u;
  cfg->n_candidates = 3u;
  cfg->max_verify = 1u;
  cfg->submap_half_window = 25u;
  cfg->search_radius = 15.0;
  cfg->max_distance = 0.2;
  cfg->submap_radius = 25.0;
  cfg->map_cell_size = 1.0f;
  cfg->surface_leaf = 1.0f;
  cfg->n_neighbors = 15u;
  cfg->max_iter = 20;
  cfg->max_rms_edge = inf;
  cfg->max_rms_surface = inf;
  cfg->min_inlier_share = 0.0;
  cfg->reject_degenerate = 1;
  cfg->scale_by_sigma2 = 1;
}

int lfx_loop_closer_create(lfx_ctx * c, const lfx_loop_closer_config * cfg, lfx_keyframes * keyframes, lfx_place_db * db, lfx_pose_graph * graph,
  lfx_loop_closer ** out)
{
  if (!c) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!cfg || !keyframes || !db || !graph || !out) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "config, keyframes, db, graph and out are required");}
  const bool ok = cfg->min_gap >= 1u && cfg->n_candidates >= 1u && cfg->n_candidates <= LFX_PLACE_MAX_MATCHES && cfg->max_verify >= 1u &&
    cfg->search_radius >= 0.0 && !std::isnan(cfg->max_distance) && cfg->submap_radius >= 0.0 && std::isfinite(cfg->submap_radius) &&
    cfg->submap_capacity[0] >= 1u && cfg->submap_capacity[0] <= UINT32_MAX && cfg->submap_capacity[1] >= 1u && cfg->submap_capacity[1] <= UINT32_MAX &&
    cfg->map_cell_size >= 0.0f && std::isfinite(cfg->map_cell_size) && cfg->surface_leaf >= 0.0f && std::isfinite(cfg->surface_leaf) &&
    cfg->n_neighbors >= 1u && cfg->n_neighbors <= 16u && cfg->max_iter >= 1 && !std::isnan(cfg->max_rms_edge) && !std::isnan(cfg->max_rms_surface) &&
    !std::isnan(cfg->min_inlier_share) && cfg->downsample_capacity <= UINT32_MAX;
  if (!ok) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "the loop closer's config is refused: min_gap, max_verify >= 1, n_candidates 1 .. 16, radii >= 0, "
             "submap_capacity 1 .. 2^32 - 1 each, downsample_capacity below 2^32, cell and leaf >= 0, n_neighbors 1 .. 16, max_iter >= 1, no NaN threshold");
  }
  lfx_keyframes_info_t ki{};
  if (lfx_keyframes_info(keyframes, &ki) != LFX_OK) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the keyframe store cannot be read");}
  // all three on the context's device: an empty read of each checks it (and says which is not) and queues nothing
  uint64_t none = 0;
  int rd = lfx_keyframes_build(c, keyframes, LFX_KEYFRAMES_EDGE, 0u, 0u, nullptr, 0u, &none, nullptr);
  if (rd == LFX_OK) {rd = lfx_place_db_download(c, db, 0u, 0u, nullptr, nullptr);}
  if (rd == LFX_OK) {rd = lfx_pose_graph_poses(c, graph, 0u, 0u, nullptr, nullptr);}
  if (rd != LFX_OK) {return rd;}
  LFX_HIP(c, hipSetDevice(c->device));
  lfx_loop_closer * lc = new (std::nothrow) lfx_loop_closer();
  if (!lc) {return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the loop closer");}
  lc->device = c->device;
  lc->cfg = *cfg;
  lc->keyframes = keyframes;
  lc->db = db;
  lc->graph = graph;
  lc->ds_capacity = cfg->surface_leaf > 0.0f ? (cfg->downsample_capacity ? cfg->downsample_capacity : std::min<uint64_t>(ki.max_points[1], 1u << 20)) : 0u;
  if (lc->submap[0].alloc(4u * (size_t)cfg->submap_capacity[0]) != hipSuccess || lc->submap[1].alloc(4u * (size_t)cfg->submap_capacity[1]) != hipSuccess ||
    (lc->ds_capacity && lc->downsampled.alloc(4u * (size_t)lc->ds_capacity) != hipSuccess) || lc->words.alloc(kScanWords) != hipSuccess ||
    lc->h_words.reserve(sizeof(uint32_t) * kScanWords) != hipSuccess)
  {
    (void)hipGetLastError();
    delete lc;
    return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the loop closer's buffers");
  }
  // (every device buffer carries 16 spare bytes behind its elements: DevBuf::alloc)
  const uint64_t buffers = lc->ds_capacity ? 4u : 3u;
  lc->device_bytes = sizeof(float) * 4u * (cfg->submap_capacity[0] + cfg->submap_capacity[1] + lc->ds_capacity) + sizeof(uint32_t) * kScanWords + 16u * buffers;
  *out = lc;
  return LFX_OK;
}

void lfx_loop_closer_destroy(lfx_loop_closer * lc) {destroy_on(lc);}

int lfx_loop_closer_info(const lfx_loop_closer * lc, lfx_loop_closer_info_t * info)
{
  if (!lc || !info) {return LFX_ERR_INVALID_ARGUMENT;}
  info->device_bytes = lc->device_bytes;
  return LFX_OK;
}

int lfx_loop_closer_set_masked(lfx_loop_closer * lc, int masked)
{
  if (!lc) {return LFX_ERR_INVALID_ARGUMENT;}
  if (masked && !keyframes_access(lc->keyframes).has_flags) {return LFX_ERR_INVALID_ARGUMENT;}
  lc->masked = masked != 0;
  return LFX_OK;
}

int lfx_loop_closer_get_masked(const lfx_loop_closer * lc, int * masked)
{
  if (!lc || !masked) {return LFX_ERR_INVALID_ARGUMENT;}
  *masked = lc->masked ? 1 : 0;
  return LFX_OK;
}

int lfx_loop_closer_detect(lfx_ctx * c, lfx_loop_closer * lc, uint32_t first, uint32_t count, lfx_place_match * candidates, uint32_t * n_eligible,
  void * stream)
{
  if (!c || !lc || !candidates) {return LFX_ERR_INVALID_ARGUMENT;}
  const int rc = check_range(c, lc, first, count);
  if (rc != LFX_OK) {return rc;}
  LFX_HIP(c, hipSetDevice(c->device));
  return detect(c, lc, first, count, candidates, n_eligible, static_cast<hipStream_t>(stream));
}

int lfx_loop_closer_verify(lfx_ctx * c, lfx_loop_closer * lc, uint32_t query_id, const lfx_place_match * candidate, lfx_loop_closure * out, void * stream)
{
  if (!c || !lc || !candidate || !out) {return LFX_ERR_INVALID_ARGUMENT;}
  const int rc = check_range(c, lc, query_id, 1u);
  if (rc != LFX_OK) {return rc;}
  if (candidate->entry == UINT32_MAX || (uint64_t)candidate->entry + lc->cfg.min_gap > query_id || !std::isfinite(candidate->yaw)) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "the candidate must be an entry with entry + min_gap <= query_id and a finite yaw");
  }
  LFX_HIP(c, hipSetDevice(c->device));
  return verify_one(c, lc, query_id, *candidate, out, static_cast<hipStream_t>(stream));
}

int lfx_loop_closer_update(lfx_ctx * c, lfx_loop_closer * lc, uint32_t first, uint32_t count, lfx_loop_closure * closures,
  lfx_loop_closer_result * result, void * stream)
{
  if (!c || !lc || !closures) {return LFX_ERR_INVALID_ARGUMENT;}
  int rc = check_range(c, lc, first, count);
  if (rc != LFX_OK) {return rc;}
  LFX_HIP(c, hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uint32_t k = lc->cfg.n_candidates;
  lfx_loop_closer_result res{};
  if (result) {*result = res;}
  std::vector<lfx_place_match> candidates((size_t)count * k);
  rc = detect(c, lc, first, count, candidates.data(), nullptr, st);
  if (rc != LFX_OK) {return rc;}
  std::vector<lfx_pose_graph_edge> edges;
  for (uint32_t s = 0; s < count; s++) {
    lfx_loop_closure & cl = closures[s];
    std::memset(&cl, 0, sizeof(cl));
    cl.query = first + s;
    cl.candidate = UINT32_MAX;
    cl.reason = LFX_LOOP_NO_CANDIDATE;
    const lfx_place_match * mine = candidates.data() + (size_t)s * k;
    res.n_detected += mine[0].entry != UINT32_MAX ? 1u : 0u;
    // (ascending distance: the matches detect emptied are the last ones)
    for (uint32_t t = 0; t < k && t < lc->cfg.max_verify && mine[t].entry != UINT32_MAX; t++) {
      rc = verify_one(c, lc, first + s, mine[t], &cl, st);
      if (rc != LFX_OK) {return rc;}
      res.n_verified++;
      if (cl.accepted) {edges.push_back(cl.edge); break;}
    }
  }
  res.n_accepted = (uint32_t)edges.size();
  if (result) {*result = res;}
  if (edges.empty()) {return LFX_OK;}
  rc = lfx_pose_graph_add_edges(c, lc->graph, edges.data(), (uint32_t)edges.size(), st);
  if (rc != LFX_OK) {
    res.n_accepted = 0u;                                 // (no edge went in)
    if (result) {*result = res;}
    return rc;
  }
  rc = lfx_pose_graph_optimize(c, lc->graph, &res.graph, st);
  if (result) {*result = res;}
  if (rc != LFX_OK) {return rc;}
  if (res.graph.code == LFX_POSE_GRAPH_CONVERGED || res.graph.code == LFX_POSE_GRAPH_MAX_ITERATIONS) {
    const double * d_poses = nullptr;
    uint32_t n_nodes = 0;
    lfx_keyframes_info_t ki{};
    rc = lfx_pose_graph_view(c, lc->graph, &d_poses, &n_nodes, st);
    if (rc == LFX_OK) {rc = lfx_keyframes_info(lc->keyframes, &ki);}
    if (rc == LFX_OK) {rc = lfx_keyframes_follow(c, lc->keyframes, d_poses, 0u, std::min(n_nodes, ki.n_keyframes), st);}
    if (rc != LFX_OK) {return rc;}
    LFX_HIP(c, hipStreamSynchronize(st));
    res.followed = 1;
    if (result) {*result = res;}
  }
  return LFX_OK;
}

}  // extern "C"
