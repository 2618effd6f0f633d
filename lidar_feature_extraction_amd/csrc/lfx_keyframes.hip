// lfx_keyframes.hip -- the keyframe store (include/lfx.h, the keyframe store section; lfx_kernels_keyframes.hpp): every
// keyframe's edge and surface records kept on the device in the SENSOR frame, one pose per keyframe beside them, and world
// clouds written from the two at the poses of the moment -- so that a map follows a pose graph's corrections.  The host
// mirrors the begin tables (the exclusive prefix of the counts): what a call needs to size a launch or refuse a request it
// knows without a wait.  Everything on the device is allocated by lfx_keyframes_create.
#include "lfx_internal.hpp"
#include "lfx_kernels_keyframes.hpp"

#include <algorithm>
#include <cstdint>

using namespace lfx_host;

static_assert(sizeof(lfx::KfPlanRecord) == sizeof(lfx_keyframes_submap_result), "the plan writes the caller's record");
static_assert(lfx::kKfNoId == LFX_KEYFRAMES_NO_ID, "the kernels' missing id is the header's");

struct lfx_keyframes
{
  int device = 0;
  lfx_keyframes_config cfg{};
  uint32_t n = 0;                        // keyframes
  std::vector<uint64_t> begin[2];        // the host's mirror of the begin tables: [n + 1]
  uint64_t device_bytes = 0;
  uint64_t chunk = 0;                    // records of `scratch`
  DevBuf<float4> records[2];
  DevBuf<uint64_t> d_begin[2];
  DevBuf<double> poses;
  DevBuf<lfx::KfCopyEntry> table[2];     // an add's clouds, uploaded from the pinned block
  DevBuf<uint8_t> flag;                  // the submap's selection, its plan and its record
  DevBuf<uint64_t> out_begin;
  DevBuf<lfx::KfPlanRecord> record;
  DevBuf<float4> scratch;                // lfx_keyframes_save: one chunk of a world cloud
  DevBuf<uint64_t> mask_runs;            // lfx_keyframes_build_masked: the kept records per run of kKfRun, then their prefix
  bool has_flags = false;                // lfx_keyframes_reserve_flags: the next four, allocated there and nowhere else
  uint64_t flag_bytes = 0;
  DevBuf<uint8_t> flags[2];              // one byte per record of the kind, addressed as the records are; non-zero: left out
  DevBuf<uint64_t> kept_begin, kept;     // lfx_keyframes_submap_masked: per keyframe of the window, G(begin[k]) and the kept records
  PinnedBuf readback;                    // the counts and begins an add reads back; the submap's record
  PinnedBuf upload;                      // what goes up (tables, begins, poses, a host keyframe's records): rewritten only
                                         // once the store's last queued call has passed
  Tail tail;                             // behind the last call that touched the store: order_behind before a call's own
                                         // work, done after it; settle before the pinned upload block is rewritten
};

namespace
{
constexpr uint32_t kInitialClouds = 64;
constexpr uint64_t kSaveChunk = (uint64_t)1 << 20;

int check_store(lfx_ctx * c, const lfx_keyframes * s) {return check_device(c, s->device, "the keyframe store");}

int check_range(lfx_ctx * c, const lfx_keyframes * s, uint32_t first, uint32_t count)
{
  if (first > s->n || count > s->n - first) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "keyframes outside the store");}
  return LFX_OK;
}

int check_kind(lfx_ctx * c, int kind)
{
  if (kind != LFX_KEYFRAMES_EDGE && kind != LFX_KEYFRAMES_SURFACE) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "kind must be LFX_KEYFRAMES_EDGE or LFX_KEYFRAMES_SURFACE");}
  return LFX_OK;
}

// the world records of source records [lo, hi), which lie in keyframes [k_lo, k_hi), to d_out (plain form) or to where
// out_begin says (selected form, indexed from `first`)
int launch_transform(lfx_ctx * c, const lfx_keyframes * s, int kind, uint64_t lo, uint64_t hi, uint32_t k_lo, uint32_t k_hi, bool selected,
  uint32_t first, float * d_out, hipStream_t st)
{
  const uint64_t blocks = (hi - lo + lfx::kKfRun - 1u) / lfx::kKfRun;
  if (blocks > 0x7FFFFFFFull) {return fail(c, LFX_ERR_CAPACITY, "too many records for one launch");}
  lfx::KfRange a{};
  a.rec_lo = lo; a.rec_hi = hi; a.k_lo = k_lo; a.k_hi = k_hi; a.first = first;
  if (selected) {
    hipLaunchKernelGGL(lfx::keyframes_transform_kernel<true>, dim3((uint32_t)blocks), dim3(lfx::kKfThreads), 0, st, s->records[kind].p,
      s->d_begin[kind].p, s->poses.p, s->out_begin.p, reinterpret_cast<float4 *>(d_out), a);
  } else {
    hipLaunchKernelGGL(lfx::keyframes_transform_kernel<false>, dim3((uint32_t)blocks), dim3(lfx::kKfThreads), 0, st, s->records[kind].p,
      s->d_begin[kind].p, s->poses.p, s->out_begin.p, reinterpret_cast<float4 *>(d_out), a);
  }
  LFX_HIP(c, hipGetLastError());
  return LFX_OK;
}

// n keyframes whose records lie on the device (src[kind], addressed by begin / count) and whose poses lie in the pinned
// block at `pose_at`: tables, begins and poses go up, one copy launch per kind; then the mirror is extended.  The caller has
// checked the capacities and settled the store.
struct KindPlan
{
  const uint4 * src = nullptr;
  const uint32_t * begin = nullptr, * count = nullptr;   // host, [n]
};

int append(Call & call, lfx_keyframes * s, const KindPlan plan[2], uint32_t n, size_t pose_at, size_t table_at)
{
  lfx_ctx * c = call.c;
  hipStream_t st = call.st;
  uint8_t * up = s->upload.p;
  size_t at = table_at;
  LFX_TRY(call.behind(s->tail));
  for (int kind = 0; kind < 2; kind++) {
    lfx::KfCopyEntry * tab = reinterpret_cast<lfx::KfCopyEntry *>(up + at);
    at += round64(sizeof(lfx::KfCopyEntry) * n);
    uint64_t * nb = reinterpret_cast<uint64_t *>(up + at);
    at += round64(sizeof(uint64_t) * n);
    uint64_t dst = s->begin[kind][s->n];
    uint32_t entries = 0, blocks = 0;
    for (uint32_t k = 0; k < n; k++) {
      const uint32_t cnt = plan[kind].count[k];
      if (cnt) {
        lfx::KfCopyEntry e{};
        e.dst = dst; e.src = plan[kind].begin[k]; e.count = cnt; e.first_block = blocks;
        tab[entries++] = e;
        blocks += (cnt + lfx::kKfThreads - 1u) / lfx::kKfThreads;
      }
      dst += cnt;
      nb[k] = dst;
    }
    LFX_HIP(c, hipMemcpyAsync(s->d_begin[kind].p + s->n + 1u, nb, sizeof(uint64_t) * n, hipMemcpyHostToDevice, st));
    if (entries) {
      LFX_HIP(c, hipMemcpyAsync(s->table[kind].p, tab, sizeof(lfx::KfCopyEntry) * entries, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(lfx::keyframes_copy_kernel, dim3(blocks), dim3(lfx::kKfThreads), 0, st, s->table[kind].p, entries, plan[kind].src,
        reinterpret_cast<uint4 *>(s->records[kind].p));
      LFX_HIP(c, hipGetLastError());
    }
  }
  LFX_HIP(c, hipMemcpyAsync(s->poses.p + 12u * (size_t)s->n, up + pose_at, sizeof(double) * 12u * n, hipMemcpyHostToDevice, st));
  // the call stands: commit
  for (int kind = 0; kind < 2; kind++) {
    uint64_t dst = s->begin[kind][s->n];
    for (uint32_t k = 0; k < n; k++) {dst += plan[kind].count[k]; s->begin[kind].push_back(dst);}
  }
  s->n += n;
  return call.finish();
}

// what an add of n keyframes needs of the pinned upload block: [poses][per kind: table, begins]
size_t upload_bytes(uint32_t n) {return round64(sizeof(double) * 12u * n) + 2u * (round64(sizeof(lfx::KfCopyEntry) * n) + round64(sizeof(uint64_t) * n));}

// the keyframes and records an add would bring fit
int check_room(lfx_ctx * c, const lfx_keyframes * s, uint32_t n, const uint64_t add[2])
{
  if (n > s->cfg.max_keyframes - s->n) {
    return fail(c, LFX_ERR_CAPACITY, "the store holds " + std::to_string(s->n) + " of " + std::to_string(s->cfg.max_keyframes) +
             " keyframes: no room for " + std::to_string(n) + " more");
  }
  for (int kind = 0; kind < 2; kind++) {
    if (add[kind] > s->cfg.max_points[kind] - s->begin[kind][s->n]) {
      return fail(c, LFX_ERR_CAPACITY, std::string("the store holds ") + std::to_string(s->begin[kind][s->n]) + " of " +
               std::to_string(s->cfg.max_points[kind]) + (kind ? " surface" : " edge") + " records: no room for " + std::to_string(add[kind]) + " more");
    }
  }
  return LFX_OK;
}

int save_kind(lfx_ctx * c, const lfx_keyframes * s, int kind, const std::string & path, hipStream_t st)
{
  const uint64_t total = s->begin[kind][s->n];
  std::vector<float> host(4u * (size_t)total);
  for (uint64_t lo = 0; lo < total; lo += s->chunk) {
    const uint64_t hi = std::min(total, lo + s->chunk);
    // (the scratch is reused: the copy down and the next chunk's kernel follow each other on the stream)
    const int rc = launch_transform(c, s, kind, lo, hi, 0u, s->n, false, 0u, reinterpret_cast<float *>(s->scratch.p), st);
    if (rc != LFX_OK) {return rc;}
    LFX_HIP(c, hipMemcpyAsync(host.data() + 4u * (size_t)lo, s->scratch.p, sizeof(float4) * (size_t)(hi - lo), hipMemcpyDeviceToHost, st));
  }
  LFX_HIP(c, hipStreamSynchronize(st));
  return write_pcd(c, path, host.data(), total);
}

int check_flags(lfx_ctx * c, const lfx_keyframes * s)
{
  if (!s->has_flags) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the store has no flags: lfx_keyframes_reserve_flags comes first");}
  return LFX_OK;
}

// the kept records of the source records [lo, hi) under `flags`, counted per run into mask_runs and scanned there (what
// keyframes_mask_scatter_kernel places from); the total is copied to *h_total, pinned, behind them.  No wait.
int launch_mask_count(lfx_ctx * c, const lfx_keyframes * s, const uint8_t * flags, uint64_t lo, uint64_t hi, uint64_t * h_total, hipStream_t st)
{
  const uint64_t runs = (hi - lo + lfx::kKfRun - 1u) / lfx::kKfRun;
  if (runs + 1u > s->mask_runs.n) {return fail(c, LFX_ERR_CAPACITY, "too many records for the masked build's table");}
  hipLaunchKernelGGL(lfx::keyframes_mask_count_kernel, dim3((uint32_t)runs), dim3(lfx::kKfThreads), 0, st, flags, lo, hi, s->mask_runs.p);
  LFX_HIP(c, hipGetLastError());
  hipLaunchKernelGGL(lfx::keyframes_mask_scan_kernel, dim3(1), dim3(lfx::kKfThreads), 0, st, s->mask_runs.p, (uint32_t)runs);
  LFX_HIP(c, hipGetLastError());
  LFX_HIP(c, hipMemcpyAsync(h_total, s->mask_runs.p + runs, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  return LFX_OK;
}

// save_kind without the store's flagged records: per chunk of source records the kept ones counted (one wait: where the
// chunk's records go on the host), placed in the scratch by the masked build's scatter and copied down.  *kept: the file's
// records; none kept, no file.
int save_kind_masked(lfx_ctx * c, const lfx_keyframes * s, int kind, const std::string & path, uint64_t * kept, hipStream_t st)
{
  const uint64_t total = s->begin[kind][s->n];
  std::vector<float> host(4u * (size_t)total);
  uint64_t * h_kept = reinterpret_cast<uint64_t *>(s->readback.p);
  uint64_t at = 0u;
  for (uint64_t lo = 0; lo < total; lo += s->chunk) {
    const uint64_t hi = std::min(total, lo + s->chunk);
    const int rc = launch_mask_count(c, s, s->flags[kind].p, lo, hi, h_kept, st);
    if (rc != LFX_OK) {return rc;}
    LFX_HIP(c, hipStreamSynchronize(st));
    const uint64_t n = *h_kept;
    if (n == 0u) {continue;}
    lfx::KfRange a{};
    a.rec_lo = lo; a.rec_hi = hi; a.k_lo = 0u; a.k_hi = s->n;
    hipLaunchKernelGGL(lfx::keyframes_mask_scatter_kernel, dim3((uint32_t)((hi - lo + lfx::kKfRun - 1u) / lfx::kKfRun)), dim3(lfx::kKfThreads), 0, st,
      s->records[kind].p, s->d_begin[kind].p, s->poses.p, s->flags[kind].p, s->mask_runs.p, s->scratch.p, a);
    LFX_HIP(c, hipGetLastError());
    LFX_HIP(c, hipMemcpyAsync(host.data() + 4u * (size_t)at, s->scratch.p, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, st));
    at += n;
  }
  LFX_HIP(c, hipStreamSynchronize(st));
  *kept = at;
  return at == 0u ? LFX_OK : write_pcd(c, path, host.data(), at);
}

}  // namespace

lfx_host::KeyframesAccess lfx_host::keyframes_access(const lfx_keyframes * s)
{
  KeyframesAccess a;
  a.device = s->device;
  a.n = s->n;
  a.has_flags = s->has_flags;
  for (int kind = 0; kind < 2; kind++) {
    a.records[kind] = s->records[kind].p;
    a.d_begin[kind] = s->d_begin[kind].p;
    a.begin[kind] = s->begin[kind].data();
    a.flags[kind] = s->flags[kind].p;
  }
  a.poses = s->poses.p;
  a.scratch = s->scratch.p;
  a.chunk = s->chunk;
  a.tail = &s->tail;
  return a;
}

extern "C" {

void lfx_keyframes_default_config(lfx_keyframes_config * config)
{
  if (!config) {return;}
  *config = lfx_keyframes_config{};
}

int lfx_keyframes_create(lfx_ctx * c, const lfx_keyframes_config * config, lfx_keyframes ** out)
{
  if (!c) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!config || !out) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "config and out are required");}
  if (config->max_keyframes < 1u || config->max_keyframes > (1u << 30)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "max_keyframes must be in 1 .. 2^30");}
  for (int kind = 0; kind < 2; kind++) {
    if (config->max_points[kind] < 1u || config->max_points[kind] > ((uint64_t)1 << 40)) {
      return fail(c, LFX_ERR_INVALID_ARGUMENT, "max_points must be in 1 .. 2^40 for both kinds");
    }
  }
  LFX_HIP(c, hipSetDevice(c->device));
  lfx_keyframes * s = new (std::nothrow) lfx_keyframes();
  if (!s) {return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the keyframe store");}
  s->device = c->device;
  s->cfg = *config;
  const size_t K = config->max_keyframes;
  s->chunk = std::min<uint64_t>(kSaveChunk, std::max(config->max_points[0], config->max_points[1]));
  auto give_up = [&](int code, const std::string & why) {(void)hipGetLastError(); lfx_keyframes_destroy(s); return fail(c, code, why);};
  DevTotal m;
  for (int kind = 0; kind < 2; kind++) {m.get(s->records[kind], config->max_points[kind]); m.get(s->d_begin[kind], K + 1u); m.get(s->table[kind], K);}
  m.get(s->poses, 12u * K); m.get(s->flag, K); m.get(s->out_begin, K); m.get(s->record, 1u); m.get(s->scratch, s->chunk);
  m.get(s->mask_runs, (size_t)(std::max(config->max_points[0], config->max_points[1]) / lfx::kKfRun) + 2u);
  if (!m.ok) {return give_up(LFX_ERR_OUT_OF_MEMORY, m.refusal("the keyframe store"));}
  s->device_bytes = m.bytes;
  for (int kind = 0; kind < 2; kind++) {
    // begin[0] = 0; every entry behind the last keyframe's reads as "no record lies here" (all ones) until an add writes it
    if (hipMemset(s->d_begin[kind].p, 0xFF, sizeof(uint64_t) * (K + 1u)) != hipSuccess || hipMemset(s->d_begin[kind].p, 0, sizeof(uint64_t)) != hipSuccess) {
      return give_up(LFX_ERR_HIP, "cannot clear the begin tables");
    }
    s->begin[kind].reserve(K + 1u);
    s->begin[kind].push_back(0u);
  }
  if (s->readback.reserve(2u * sizeof(uint32_t) * (5u * kInitialClouds) + sizeof(lfx::KfPlanRecord)) != hipSuccess ||
    s->upload.reserve(upload_bytes(kInitialClouds)) != hipSuccess)
  {
    return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the keyframe store's pinned blocks");
  }
  *out = s;
  return LFX_OK;
}

void lfx_keyframes_destroy(lfx_keyframes * s) {destroy_on(s);}

int lfx_keyframes_info(const lfx_keyframes * s, lfx_keyframes_info_t * info)
{
  if (!s || !info) {return LFX_ERR_INVALID_ARGUMENT;}
  *info = lfx_keyframes_info_t{};
  info->n_keyframes = s->n;
  info->max_keyframes = s->cfg.max_keyframes;
  for (int kind = 0; kind < 2; kind++) {info->n_points[kind] = s->begin[kind][s->n]; info->max_points[kind] = s->cfg.max_points[kind];}
  info->device_bytes = s->device_bytes;
  return LFX_OK;
}

int lfx_keyframes_view(lfx_ctx * c, const lfx_keyframes * s, lfx_keyframes_store_view * view, void * stream)
{
  if (!c || !s || !view) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_store(c, s) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.read(s->tail));
  *view = lfx_keyframes_store_view{};
  for (int kind = 0; kind < 2; kind++) {
    view->points[kind] = reinterpret_cast<const float *>(s->records[kind].p);
    view->begin[kind] = s->d_begin[kind].p;
    view->n_points[kind] = s->begin[kind][s->n];
  }
  view->poses = s->poses.p;
  view->n_keyframes = s->n;
  return LFX_OK;
}

int lfx_keyframes_add(lfx_ctx * c, lfx_keyframes * s, const lfx_keyframes_clouds * edge, const lfx_keyframes_clouds * surface, uint32_t n,
  const double * poses, uint32_t * first_id, void * stream)
{
  if (!c || !s || !edge || !surface || !poses) {return LFX_ERR_INVALID_ARGUMENT;}
  const lfx_keyframes_clouds * in[2] = {edge, surface};
  for (int kind = 0; kind < 2; kind++) {
    if (!in[kind]->d_points || !in[kind]->d_begin || !in[kind]->d_count) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "d_points, d_begin and d_count are required");}
    if (in[kind]->count_stride == 0u) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "count_stride must be >= 1");}
  }
  if (n == 0u) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "n must be >= 1");}
  if (!finite_all(poses, 12u * (size_t)n)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "a pose that is not finite");}
  if (check_store(c, s) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  const uint64_t none[2] = {0u, 0u};
  LFX_TRY(check_room(c, s, n, none));
  Call call(c, stream);
  LFX_TRY(call.open());
  // both kinds' counts and begins back in one wait: the call's only one
  const CloudList lists[2] = {{edge->d_begin, edge->d_count, edge->count_stride, edge->total_points, "edge "},
    {surface->d_begin, surface->d_count, surface->count_stride, surface->total_points, "surface "}};
  LFX_HIP(c, s->readback.reserve(readback_bytes(n, edge->count_stride) + readback_bytes(n, surface->count_stride)));
  std::vector<uint32_t> begin[2], count[2];
  LFX_TRY(read_lists(c, lists, 2, n, s->readback.p, begin, count, call.st));
  uint64_t add[2] = {0u, 0u};
  for (int kind = 0; kind < 2; kind++) {
    uint64_t blocks = 0u;
    for (uint32_t k = 0; k < n; k++) {
      add[kind] += count[kind][k];
      blocks += (count[kind][k] + lfx::kKfThreads - 1u) / lfx::kKfThreads;
    }
    if (blocks > 0x7FFFFFFFull) {return fail(c, LFX_ERR_CAPACITY, "the call adds too many records for one launch");}
  }
  LFX_TRY(check_room(c, s, n, add));
  LFX_TRY(call.after(s->tail));
  LFX_HIP(c, s->upload.reserve(upload_bytes(n)));
  std::memcpy(s->upload.p, poses, sizeof(double) * 12u * n);
  KindPlan plan[2];
  for (int kind = 0; kind < 2; kind++) {
    plan[kind].src = reinterpret_cast<const uint4 *>(in[kind]->d_points);
    plan[kind].begin = begin[kind].data();
    plan[kind].count = count[kind].data();
  }
  const uint32_t first = s->n;
  LFX_TRY(append(call, s, plan, n, 0u, round64(sizeof(double) * 12u * n)));
  if (first_id) {*first_id = first;}
  return LFX_OK;
}

int lfx_keyframes_add_host(lfx_ctx * c, lfx_keyframes * s, const float * edge, uint32_t n_edge, const float * surface, uint32_t n_surface,
  const double pose[12], uint32_t * id, void * stream)
{
  if (!c || !s || !pose || (n_edge && !edge) || (n_surface && !surface)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!finite_all(pose, 12u)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "a pose that is not finite");}
  if (check_store(c, s) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  const uint64_t add[2] = {n_edge, n_surface};
  LFX_TRY(check_room(c, s, 1u, add));
  Call k(c, stream);
  hipStream_t st = k.st;
  LFX_TRY(k.open());
  LFX_TRY(k.after(s->tail));
  // the pinned block: [pose][the two new begins][edge records][surface records]; copied up from there, straight into place
  const size_t head = 128u, e_bytes = sizeof(float4) * (size_t)n_edge, s_bytes = sizeof(float4) * (size_t)n_surface;
  LFX_HIP(c, s->upload.reserve(head + e_bytes + s_bytes));
  uint8_t * up = s->upload.p;
  std::memcpy(up, pose, sizeof(double) * 12u);
  uint64_t * nb = reinterpret_cast<uint64_t *>(up + 96u);
  const float * src[2] = {edge, surface};
  const size_t bytes[2] = {e_bytes, s_bytes}, where[2] = {head, head + e_bytes};
  LFX_TRY(k.behind(s->tail));
  for (int kind = 0; kind < 2; kind++) {
    const uint64_t at = s->begin[kind][s->n];
    nb[kind] = at + add[kind];
    if (bytes[kind]) {
      std::memcpy(up + where[kind], src[kind], bytes[kind]);
      LFX_HIP(c, hipMemcpyAsync(s->records[kind].p + at, up + where[kind], bytes[kind], hipMemcpyHostToDevice, st));
    }
    LFX_HIP(c, hipMemcpyAsync(s->d_begin[kind].p + s->n + 1u, nb + kind, sizeof(uint64_t), hipMemcpyHostToDevice, st));
  }
  LFX_HIP(c, hipMemcpyAsync(s->poses.p + 12u * (size_t)s->n, up, sizeof(double) * 12u, hipMemcpyHostToDevice, st));
  for (int kind = 0; kind < 2; kind++) {s->begin[kind].push_back(nb[kind]);}
  if (id) {*id = s->n;}
  s->n += 1u;
  return k.finish();
}

int lfx_keyframes_set_poses(lfx_ctx * c, lfx_keyframes * s, uint32_t first, uint32_t count, const double * poses, void * stream)
{
  if (!c || !s || (count && !poses)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_store(c, s) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_range(c, s, first, count) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!finite_all(poses, 12u * (size_t)count)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "a pose that is not finite");}
  if (count == 0u) {return LFX_OK;}
  Call k(c, stream);
  return poses_set(k, s->tail, s->poses, s->upload, first, count, poses);
}

int lfx_keyframes_poses(lfx_ctx * c, const lfx_keyframes * s, uint32_t first, uint32_t count, double * poses_out, void * stream)
{
  if (!c || !s || (count && !poses_out)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_store(c, s) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_range(c, s, first, count) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (count == 0u) {return LFX_OK;}
  Call k(c, stream);
  return poses_get(k, s->tail, s->poses, first, count, poses_out);
}

int lfx_keyframes_follow(lfx_ctx * c, lfx_keyframes * s, const double * d_poses, uint32_t first, uint32_t count, void * stream)
{
  if (!c || !s || (count && !d_poses)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_store(c, s) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_range(c, s, first, count) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (count == 0u) {return LFX_OK;}
  Call k(c, stream);
  return poses_follow(k, s->tail, s->poses, d_poses, first, count);
}

int lfx_keyframes_build(lfx_ctx * c, const lfx_keyframes * s, int kind, uint32_t first, uint32_t count, float * d_out, uint64_t capacity_points,
  uint64_t * n_out, void * stream)
{
  if (!c || !s || !n_out) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_store(c, s) != LFX_OK || check_kind(c, kind) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_range(c, s, first, count) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  const uint64_t lo = s->begin[kind][first], hi = s->begin[kind][first + count];
  if (hi - lo > capacity_points) {
    *n_out = hi - lo;
    return fail(c, LFX_ERR_CAPACITY, "the keyframes hold " + std::to_string(hi - lo) + " records: more than capacity_points (" + std::to_string(capacity_points) + ")");
  }
  *n_out = hi - lo;
  if (hi == lo) {return LFX_OK;}
  if (!d_out) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "d_out is required");}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.behind(s->tail));
  LFX_TRY(launch_transform(c, s, kind, lo, hi, first, first + count, false, first, d_out, k.st));
  return k.finish();
}

int lfx_keyframes_build_masked(lfx_ctx * c, const lfx_keyframes * s, int kind, uint32_t first, uint32_t count, const uint8_t * d_flags, float * d_out,
  uint64_t capacity_points, uint64_t * d_begin_out, uint64_t * n_out, void * stream)
{
  if (!c || !s || !n_out) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_store(c, s) != LFX_OK || check_kind(c, kind) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_range(c, s, first, count) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  const uint64_t lo = s->begin[kind][first], hi = s->begin[kind][first + count];
  *n_out = 0u;
  Call k(c, stream);
  hipStream_t st = k.st;
  LFX_TRY(k.open());
  if (hi == lo) {
    if (d_begin_out) {LFX_HIP(c, hipMemsetAsync(d_begin_out, 0, sizeof(uint64_t) * ((size_t)count + 1u), st));}
    return LFX_OK;
  }
  if (!d_flags) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "d_flags is required");}
  const uint64_t runs = (hi - lo + lfx::kKfRun - 1u) / lfx::kKfRun;
  if (runs + 1u > s->mask_runs.n) {return fail(c, LFX_ERR_CAPACITY, "too many records for the masked build's table");}
  LFX_TRY(k.behind(s->tail));
  hipLaunchKernelGGL(lfx::keyframes_mask_count_kernel, dim3((uint32_t)runs), dim3(lfx::kKfThreads), 0, st, d_flags, lo, hi, s->mask_runs.p);
  LFX_HIP(c, hipGetLastError());
  hipLaunchKernelGGL(lfx::keyframes_mask_scan_kernel, dim3(1), dim3(lfx::kKfThreads), 0, st, s->mask_runs.p, (uint32_t)runs);
  LFX_HIP(c, hipGetLastError());
  // the call's only wait: the kept records (the caller needs them to hand the cloud on; the capacity is checked against them)
  LFX_TRY(read_block(c, s->readback, s->mask_runs.p + runs, sizeof(uint64_t), st));
  *n_out = *reinterpret_cast<const uint64_t *>(s->readback.p);
  if (*n_out > capacity_points) {
    return fail(c, LFX_ERR_CAPACITY, "the keyframes keep " + std::to_string(*n_out) + " records: more than capacity_points (" + std::to_string(capacity_points) + ")");
  }
  if (*n_out > 0u) {
    if (!d_out) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "d_out is required");}
    lfx::KfRange a{};
    a.rec_lo = lo; a.rec_hi = hi; a.k_lo = first; a.k_hi = first + count; a.first = first;
    hipLaunchKernelGGL(lfx::keyframes_mask_scatter_kernel, dim3((uint32_t)runs), dim3(lfx::kKfThreads), 0, st, s->records[kind].p, s->d_begin[kind].p,
      s->poses.p, d_flags, s->mask_runs.p, reinterpret_cast<float4 *>(d_out), a);
    LFX_HIP(c, hipGetLastError());
  }
  if (d_begin_out) {
    hipLaunchKernelGGL(lfx::keyframes_mask_begin_kernel, dim3(count / lfx::kKfThreads + 1u), dim3(lfx::kKfThreads), 0, st, d_flags, s->d_begin[kind].p,
      s->mask_runs.p, first, count, lo, d_begin_out);
    LFX_HIP(c, hipGetLastError());
  }
  return k.finish();
}

int lfx_keyframes_submap(lfx_ctx * c, const lfx_keyframes * s, int kind, const double center[3], double radius, uint32_t first, uint32_t count,
  float * d_out, uint64_t capacity_points, lfx_keyframes_submap_result * result, void * stream)
{
  if (!c || !s || !center || !result) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_store(c, s) != LFX_OK || check_kind(c, kind) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_range(c, s, first, count) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!finite_all(center, 3u) || !std::isfinite(radius) || radius < 0.0) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the centre must be finite, the radius finite and >= 0");}
  *result = lfx_keyframes_submap_result{};
  result->first_id = result->last_id = LFX_KEYFRAMES_NO_ID;
  if (count == 0u) {return LFX_OK;}
  Call k(c, stream);
  hipStream_t st = k.st;
  LFX_TRY(k.open());
  LFX_TRY(k.behind(s->tail));
  hipLaunchKernelGGL(lfx::keyframes_flag_kernel, dim3((count + lfx::kKfThreads - 1u) / lfx::kKfThreads), dim3(lfx::kKfThreads), 0, st, s->poses.p, first,
    count, center[0], center[1], center[2], radius * radius, s->flag.p);
  LFX_HIP(c, hipGetLastError());
  hipLaunchKernelGGL(lfx::keyframes_plan_kernel<false>, dim3(1), dim3(lfx::kKfThreads), 0, st, s->flag.p, s->d_begin[kind].p, first, count, capacity_points,
    s->out_begin.p, s->record.p);
  LFX_HIP(c, hipGetLastError());
  // the call's only wait: the plan's record (the caller needs n_points to hand the cloud on; the launch below its range)
  LFX_TRY(read_block(c, s->readback, s->record.p, sizeof(lfx::KfPlanRecord), st));
  std::memcpy(result, s->readback.p, sizeof(*result));
  result->reserved = 0u;
  if (result->n_points > 0u) {
    if (!d_out) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "d_out is required");}
    const uint32_t k_lo = result->first_id, k_hi = result->last_id + 1u;
    LFX_TRY(launch_transform(c, s, kind, s->begin[kind][k_lo], s->begin[kind][k_hi], k_lo, k_hi, true, first, d_out, st));
  }
  return k.finish();
}

int lfx_keyframes_save(lfx_ctx * c, const lfx_keyframes * s, const char * dirname, int written[2], void * stream)
{
  if (!c || !s || !dirname || !written) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_store(c, s) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  written[0] = written[1] = 0;
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.read(s->tail));
  for (int kind = 0; kind < 2; kind++) {
    if (s->begin[kind][s->n] == 0u) {continue;}
    LFX_TRY(save_kind(c, s, kind, kind_path(dirname, kind), k.st));
    written[kind] = 1;
  }
  return LFX_OK;
}

// --- flags that belong to the store ----------------------------------------------------------------------------------------------

int lfx_keyframes_reserve_flags(lfx_ctx * c, lfx_keyframes * s, void * stream)
{
  if (!c || !s) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_store(c, s) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (s->has_flags) {return LFX_OK;}
  Call k(c, stream);
  LFX_TRY(k.open());
  DevBuf<uint8_t> flags[2];
  DevBuf<uint64_t> kept_begin, kept;
  const size_t K = s->cfg.max_keyframes;
  const uint64_t bytes = s->cfg.max_points[0] + s->cfg.max_points[1] + 2u * sizeof(uint64_t) * K;
  if (flags[0].alloc(s->cfg.max_points[0]) != hipSuccess || flags[1].alloc(s->cfg.max_points[1]) != hipSuccess || kept_begin.alloc(K) != hipSuccess ||
    kept.alloc(K) != hipSuccess)
  {
    (void)hipGetLastError();
    return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the keyframe store's " + std::to_string(bytes) + " bytes of flags");
  }
  LFX_TRY(k.behind(s->tail));
  for (int kind = 0; kind < 2; kind++) {LFX_HIP(c, hipMemsetAsync(flags[kind].p, 0, s->cfg.max_points[kind], k.st));}
  LFX_TRY(k.finish());
  for (int kind = 0; kind < 2; kind++) {s->flags[kind] = std::move(flags[kind]);}
  s->kept_begin = std::move(kept_begin);
  s->kept = std::move(kept);
  s->flag_bytes = bytes;
  s->has_flags = true;
  return LFX_OK;
}

int lfx_keyframes_flags(lfx_ctx * c, lfx_keyframes * s, uint8_t * d_flags[2], void * stream)
{
  if (!c || !s || !d_flags) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_store(c, s) != LFX_OK || check_flags(c, s) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.read(s->tail));
  for (int kind = 0; kind < 2; kind++) {d_flags[kind] = s->flags[kind].p;}
  return LFX_OK;
}

int lfx_keyframes_set_flags(lfx_ctx * c, lfx_keyframes * s, int kind, uint32_t first, uint32_t count, const uint8_t * d_src, void * stream)
{
  if (!c || !s) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_store(c, s) != LFX_OK || check_kind(c, kind) != LFX_OK || check_flags(c, s) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_range(c, s, first, count) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  const uint64_t lo = s->begin[kind][first], hi = s->begin[kind][first + count];
  if (hi == lo) {return LFX_OK;}
  if (!d_src) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "d_src is required");}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.behind(s->tail));
  LFX_HIP(c, hipMemcpyAsync(s->flags[kind].p + lo, d_src + lo, (size_t)(hi - lo), hipMemcpyDeviceToDevice, k.st));
  return k.finish();
}

int lfx_keyframes_clear_flags(lfx_ctx * c, lfx_keyframes * s, int kind, uint32_t first, uint32_t count, void * stream)
{
  if (!c || !s) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_store(c, s) != LFX_OK || check_kind(c, kind) != LFX_OK || check_flags(c, s) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_range(c, s, first, count) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  const uint64_t lo = s->begin[kind][first], hi = s->begin[kind][first + count];
  if (hi == lo) {return LFX_OK;}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.behind(s->tail));
  LFX_HIP(c, hipMemsetAsync(s->flags[kind].p + lo, 0, (size_t)(hi - lo), k.st));
  return k.finish();
}

int lfx_keyframes_flags_info(lfx_ctx * c, const lfx_keyframes * s, lfx_keyframes_flags_info_t * info, void * stream)
{
  if (!c || !s || !info) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_store(c, s) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  *info = lfx_keyframes_flags_info_t{};
  if (!s->has_flags) {return LFX_OK;}
  info->reserved = 1;
  info->device_bytes = s->flag_bytes;
  const uint64_t total[2] = {s->begin[0][s->n], s->begin[1][s->n]};
  if (total[0] == 0u && total[1] == 0u) {return LFX_OK;}
  Call k(c, stream);
  hipStream_t st = k.st;
  LFX_TRY(k.open());
  LFX_TRY(k.behind(s->tail));
  // both kinds' kept records through the masked build's table, one behind the other; the call's only wait
  uint64_t * h_kept = reinterpret_cast<uint64_t *>(s->readback.p);
  for (int kind = 0; kind < 2; kind++) {
    h_kept[kind] = 0u;
    if (total[kind] == 0u) {continue;}
    LFX_TRY(launch_mask_count(c, s, s->flags[kind].p, 0u, total[kind], h_kept + kind, st));
  }
  LFX_HIP(c, hipStreamSynchronize(st));
  for (int kind = 0; kind < 2; kind++) {info->n_flagged[kind] = total[kind] - h_kept[kind];}
  return k.finish();
}

int lfx_keyframes_submap_masked(lfx_ctx * c, const lfx_keyframes * s, int kind, const double center[3], double radius, uint32_t first,
  uint32_t count, float * d_out, uint64_t capacity_points, lfx_keyframes_submap_result * result, void * stream)
{
  if (!c || !s || !center || !result) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_store(c, s) != LFX_OK || check_kind(c, kind) != LFX_OK || check_flags(c, s) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_range(c, s, first, count) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!finite_all(center, 3u) || !std::isfinite(radius) || radius < 0.0) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the centre must be finite, the radius finite and >= 0");}
  *result = lfx_keyframes_submap_result{};
  result->first_id = result->last_id = LFX_KEYFRAMES_NO_ID;
  if (count == 0u) {return LFX_OK;}
  const uint64_t lo = s->begin[kind][first], hi = s->begin[kind][first + count];
  const uint64_t runs = (hi - lo + lfx::kKfRun - 1u) / lfx::kKfRun;
  if (runs + 1u > s->mask_runs.n) {return fail(c, LFX_ERR_CAPACITY, "too many records for the masked build's table");}
  Call k(c, stream);
  hipStream_t st = k.st;
  LFX_TRY(k.open());
  LFX_TRY(k.behind(s->tail));
  const dim3 per_keyframe((count + lfx::kKfThreads - 1u) / lfx::kKfThreads), threads(lfx::kKfThreads);
  const uint8_t * flags = s->flags[kind].p;
  lfx::KfRange a{};
  a.rec_lo = lo; a.rec_hi = hi; a.k_lo = first; a.k_hi = first + count; a.first = first;
  hipLaunchKernelGGL(lfx::keyframes_flag_kernel, per_keyframe, threads, 0, st, s->poses.p, first, count, center[0], center[1], center[2], radius * radius,
    s->flag.p);
  LFX_HIP(c, hipGetLastError());
  if (runs > 0u) {
    hipLaunchKernelGGL(lfx::keyframes_submask_count_kernel, dim3((uint32_t)runs), threads, 0, st, flags, s->d_begin[kind].p, s->flag.p, s->mask_runs.p, a);
    LFX_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(lfx::keyframes_mask_scan_kernel, dim3(1), threads, 0, st, s->mask_runs.p, (uint32_t)runs);
    LFX_HIP(c, hipGetLastError());
  }
  // (a window without records has only empty keyframes: the next kernel reads no prefix)
  const uint32_t waves = lfx::kKfThreads / lfx::kKfWave;                  // (one wave per keyframe)
  hipLaunchKernelGGL(lfx::keyframes_submask_kept_kernel, dim3((count + waves - 1u) / waves), threads, 0, st, flags, s->d_begin[kind].p, s->flag.p, s->mask_runs.p, first, count, lo,
    s->kept_begin.p, s->kept.p);
  LFX_HIP(c, hipGetLastError());
  hipLaunchKernelGGL(lfx::keyframes_plan_kernel<true>, dim3(1), threads, 0, st, s->flag.p, s->kept.p, first, count, capacity_points, s->out_begin.p,
    s->record.p);
  LFX_HIP(c, hipGetLastError());
  // the call's only wait: the plan's record, as lfx_keyframes_submap's
  LFX_TRY(read_block(c, s->readback, s->record.p, sizeof(lfx::KfPlanRecord), st));
  std::memcpy(result, s->readback.p, sizeof(*result));
  result->reserved = 0u;
  if (result->n_points > 0u) {
    if (!d_out) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "d_out is required");}
    // the runs of the count pass that hold the written keyframes' records
    const uint64_t run0 = (s->begin[kind][result->first_id] - lo) / lfx::kKfRun;
    const uint64_t run1 = (s->begin[kind][result->last_id + 1u] - lo + lfx::kKfRun - 1u) / lfx::kKfRun;
    hipLaunchKernelGGL(lfx::keyframes_submask_scatter_kernel, dim3((uint32_t)(run1 - run0)), threads, 0, st, s->records[kind].p, s->d_begin[kind].p,
      s->poses.p, flags, s->mask_runs.p, s->out_begin.p, s->kept_begin.p, reinterpret_cast<float4 *>(d_out), (uint32_t)run0, a);
    LFX_HIP(c, hipGetLastError());
  }
  return k.finish();
}

int lfx_keyframes_save_masked(lfx_ctx * c, const lfx_keyframes * s, const char * dirname, int written[2], void * stream)
{
  if (!c || !s || !dirname || !written) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_store(c, s) != LFX_OK || check_flags(c, s) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  written[0] = written[1] = 0;
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.read(s->tail));
  for (int kind = 0; kind < 2; kind++) {
    if (s->begin[kind][s->n] == 0u) {continue;}
    uint64_t kept = 0u;
    LFX_TRY(save_kind_masked(c, s, kind, kind_path(dirname, kind), &kept, k.st));
    written[kind] = kept > 0u ? 1 : 0;
  }
  return LFX_OK;
}

}  // extern "C"
