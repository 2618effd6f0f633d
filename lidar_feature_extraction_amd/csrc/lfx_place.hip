// lfx_place.hip -- place recognition (include/lfx.h, the place recognition section; lfx_kernels_place.hpp):
// lfx_scan_context_batch, the descriptors of the last device batch's scans from its input records, and lfx_place_db, the
// index that compares query descriptors with every entry of a range -- or, gated, with the entries below a limit whose pose
// lies near the query's -- under every column shift.  The descriptor's tables come from
// lfx_scan_context_tables (lfx_pose.cpp) and from nowhere else.
#include "lfx_internal.hpp"
#include "lfx_kernels_place.hpp"

#include <algorithm>
#include <cstdint>

using namespace lfx_host;

struct lfx_place_db
{
  int device = 0;
  lfx_scan_context_config cfg{};
  uint32_t capacity = 0, n = 0;
  DevBuf<float> desc;                        // [capacity][R][S]
  DevBuf<double> norms;                      // [capacity][S]
  DevBuf<float> staged;                      // lfx_place_db_add_host: the descriptors on their way up
  // a query's workspace: the queries' norms, the least distance and its shift per (query, entry), the matches
  mutable DevBuf<double> query_norms, best_distance;
  mutable DevBuf<uint32_t> best_shift;
  mutable DevBuf<lfx::PlaceMatchDevice> matches;
  mutable PinnedBuf h_matches;
  // the gated query's: the gates, the lists of eligible entries ([queries][largest limit]) and their lengths
  mutable DevBuf<lfx::PlaceGate> gates;
  mutable DevBuf<uint32_t> list, n_eligible;
  mutable PinnedBuf h_gates, h_eligible;
  Tail added;                                // behind the last add's copy and norms
};

namespace
{
uint32_t cells_of(const lfx_scan_context_config & cfg) {return cfg.n_rings * cfg.n_sectors;}

int check_db(lfx_ctx * c, const lfx_place_db * db) {return check_device(c, db->device, "the place index");}

// the config's tables as the kernel takes them (sc_table_doubles), or what lfx_scan_context_tables refuses
int write_tables(lfx_ctx * c, const lfx_scan_context_config * cfg, double * out)
{
  // (checked here first: the arrays below are sized by R and S)
  if (cfg->n_rings < 1u || cfg->n_rings > LFX_SCAN_CONTEXT_MAX_RINGS || cfg->n_sectors < 4u || cfg->n_sectors > LFX_SCAN_CONTEXT_MAX_SECTORS) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "n_rings must be in 1 .. 40 and n_sectors even, in 4 .. 120");
  }
  const uint32_t R = cfg->n_rings, S = cfg->n_sectors;
  if (lfx_scan_context_tables(cfg, out, out + S, out + 2u * S) != LFX_OK) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "the scan-context config is refused: n_sectors even, radii finite with 0 <= min_radius < max_radius, "
             "sensor_height finite");
  }
  out[2u * S + R + 1u] = (double)cfg->min_radius * (double)cfg->min_radius;
  return LFX_OK;
}

// the ring's next slot with room for the call's table and keys, the kernels that used it last waited for; a failure leaves
// the ring where it was
int take_slot(lfx_ctx * c, size_t doubles, size_t keys, lfx_ctx::PlaceSlot *& slot)
{
  LFX_HIP(c, hipSetDevice(c->device));
  slot = &c->place_slots[c->place_next];
  hipError_t e;
  const int rs = slot->table.take(c, doubles, e);
  if (rs != LFX_OK) {return rs;}
  if (e == hipSuccess) {e = hold(slot->keys, keys);}
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, LFX_ERR_OUT_OF_MEMORY, std::string("cannot set up the scan-context tables: ") + hipGetErrorString(e));
  }
  c->place_next = (c->place_next + 1u) % lfx_ctx::kPlaceSlots;
  return LFX_OK;
}

// the comparison kernels may ask for more dynamic LDS than a kernel gets unasked (82 KB at R = 40, S = 120)
int allow_compare_lds(lfx_ctx * c)
{
  const int most = (int)lfx::place_compare_lds(LFX_SCAN_CONTEXT_MAX_RINGS, LFX_SCAN_CONTEXT_MAX_SECTORS);
  LFX_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(lfx::place_compare_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, most));
  LFX_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(lfx::place_compare_gated_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, most));
  return LFX_OK;
}

// the device's matches as the caller's: the yaw of each shift
void write_matches(const lfx::PlaceMatchDevice * got, size_t n_matches, uint32_t S, lfx_place_match * matches)
{
  const double step = (2.0 * M_PI) / (double)S;
  for (size_t i = 0; i < n_matches; i++) {
    lfx_place_match & m = matches[i];
    m.entry = got[i].entry;
    m.shift = got[i].shift;
    m.distance = got[i].distance;
    m.yaw = got[i].entry == UINT32_MAX ? 0.0 : (2u * got[i].shift <= S ? (double)got[i].shift * step : ((double)got[i].shift - (double)S) * step);
  }
}

int launch_norms(lfx_ctx * c, const float * d_desc, double * d_norms, uint32_t n, const lfx_scan_context_config & cfg, hipStream_t st)
{
  const size_t threads = (size_t)n * cfg.n_sectors;
  hipLaunchKernelGGL(lfx::place_norms_kernel, dim3(blocks_for(threads, lfx::kPlaceThreads)), dim3(lfx::kPlaceThreads), 0, st,
    d_desc, d_norms, n, cfg.n_rings, cfg.n_sectors);
  LFX_HIP(c, hipGetLastError());
  return LFX_OK;
}

// n descriptors on the device appended: all or nothing
int add_device(Call & k, lfx_place_db * db, const float * d_desc, uint32_t n)
{
  const size_t cells = cells_of(db->cfg);
  float * dst = db->desc.p + (size_t)db->n * cells;
  // (the add before may be queued on another stream: the event recorded at the end then stands for both)
  LFX_TRY(k.behind(db->added));
  // (hipMemcpyDefault: d_desc may be pinned host memory, lfx_host_alloc, which a kernel writes as it writes device memory)
  LFX_HIP(k.c, hipMemcpyAsync(dst, d_desc, sizeof(float) * cells * n, hipMemcpyDefault, k.st));
  LFX_TRY(launch_norms(k.c, dst, db->norms.p + (size_t)db->n * db->cfg.n_sectors, n, db->cfg, k.st));
  LFX_TRY(k.finish());
  db->n += n;
  return LFX_OK;
}

int check_add(lfx_ctx * c, const lfx_place_db * db, uint32_t n)
{
  if (check_db(c, db) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (n > db->capacity - db->n) {
    return fail(c, LFX_ERR_CAPACITY, "the place index holds " + std::to_string(db->n) + " of " + std::to_string(db->capacity) + " entries: no room for " +
             std::to_string(n) + " more");
  }
  return LFX_OK;
}
}  // namespace

const float * lfx_host::place_db_entries(const lfx_place_db * db, uint32_t * cells)
{
  *cells = cells_of(db->cfg);
  return db->desc.p;
}

extern "C" {

int lfx_scan_context_batch(lfx_ctx * c, const lfx_scan_context_config * cfg, uint32_t n_scans, float * d_desc_out, void * stream)
{
  if (!c) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!cfg || !d_desc_out) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "config and d_desc_out are required");}
  double table[2 * LFX_SCAN_CONTEXT_MAX_SECTORS + LFX_SCAN_CONTEXT_MAX_RINGS + 2];
  const int rt = write_tables(c, cfg, table);
  if (rt != LFX_OK) {return rt;}
  const int rb = check_last_batch(c, n_scans);
  if (rb != LFX_OK) {return rb;}
  if (!c->last_points) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the last batch's input points are not known");}
  const uint32_t R = cfg->n_rings, S = cfg->n_sectors;
  const size_t doubles = lfx::sc_table_doubles(R, S), total = (size_t)n_scans * R * S;
  Call k(c, stream);
  hipStream_t st = k.st;
  lfx_ctx::PlaceSlot * slot;
  LFX_TRY(take_slot(c, doubles, total, slot));
  LFX_TRY(k.take(slot->table.used));     // (settled by take_slot)
  std::memcpy(slot->table.h.p, table, sizeof(double) * doubles);
  LFX_HIP(c, hipMemcpyAsync(slot->table.d.p, slot->table.h.p, sizeof(double) * doubles, hipMemcpyHostToDevice, st));
  LFX_HIP(c, hipMemsetAsync(slot->keys.p, 0, sizeof(uint32_t) * total, st));
  lfx::ScanContextArgs a{};
  a.pts = static_cast<const uint8_t *>(c->last_points);
  a.L = c->layout;
  a.scan_begin = c->scan_begin.p;
  a.table = slot->table.d.p;
  a.keys = slot->keys.p;
  a.R = R; a.S = S;
  const bool xyz16 = canonical_xyz16(c->layout, a.pts);
  hipLaunchKernelGGL(xyz16 ? lfx::scan_context_kernel<true> : lfx::scan_context_kernel<false>, by_scan_grid(n_scans), dim3(lfx::kPlaceThreads), 0, st, a);
  LFX_HIP(c, hipGetLastError());
  hipLaunchKernelGGL(lfx::scan_context_finish_kernel, dim3(blocks_for(total, lfx::kPlaceThreads)), dim3(lfx::kPlaceThreads), 0, st,
    slot->keys.p, d_desc_out, total, cfg->sensor_height);
  LFX_HIP(c, hipGetLastError());
  return k.finish();
}

int lfx_place_db_create(lfx_ctx * c, const lfx_scan_context_config * cfg, uint32_t capacity, lfx_place_db ** out)
{
  if (!c) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!cfg || !out) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "config and out are required");}
  double table[2 * LFX_SCAN_CONTEXT_MAX_SECTORS + LFX_SCAN_CONTEXT_MAX_RINGS + 2];
  const int rt = write_tables(c, cfg, table);
  if (rt != LFX_OK) {return rt;}
  if (capacity == 0) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "capacity must be >= 1");}
  LFX_HIP(c, hipSetDevice(c->device));
  const int ra = allow_compare_lds(c);
  if (ra != LFX_OK) {return ra;}
  lfx_place_db * db = new (std::nothrow) lfx_place_db();
  if (!db) {return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the place index");}
  db->device = c->device;
  db->cfg = *cfg;
  db->capacity = capacity;
  auto give_up = [&](int code, const std::string & why) {(void)hipGetLastError(); lfx_place_db_destroy(db); return fail(c, code, why);};
  if (db->desc.alloc((size_t)capacity * cells_of(*cfg)) != hipSuccess || db->norms.alloc((size_t)capacity * cfg->n_sectors) != hipSuccess) {
    return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the place index's descriptors");
  }
  *out = db;
  return LFX_OK;
}

void lfx_place_db_destroy(lfx_place_db * db) {destroy_on(db);}

int lfx_place_db_add(lfx_ctx * c, lfx_place_db * db, const float * d_desc, uint32_t n, void * stream)
{
  if (!c || !db || (n && !d_desc)) {return LFX_ERR_INVALID_ARGUMENT;}
  const int rc = check_add(c, db, n);
  if (rc != LFX_OK || n == 0) {return rc;}
  Call k(c, stream);
  LFX_TRY(k.open());
  return add_device(k, db, d_desc, n);
}

int lfx_place_db_add_host(lfx_ctx * c, lfx_place_db * db, const float * desc, uint32_t n, void * stream)
{
  if (!c || !db || (n && !desc)) {return LFX_ERR_INVALID_ARGUMENT;}
  const int rc = check_add(c, db, n);
  if (rc != LFX_OK || n == 0) {return rc;}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.after(db->added));           // (the add before may still read the staged descriptors, on whichever stream)
  const size_t floats = (size_t)n * cells_of(db->cfg);
  if (hold(db->staged, floats) != hipSuccess) {(void)hipGetLastError(); return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot stage the descriptors");}
  LFX_HIP(c, hipMemcpyAsync(db->staged.p, desc, sizeof(float) * floats, hipMemcpyHostToDevice, k.st));
  // (pageable memory has been read when the copy returns; a pinned block must not be rewritten before `stream` passes it)
  return add_device(k, db, db->staged.p, n);
}

int lfx_place_db_size(const lfx_place_db * db, uint32_t * n)
{
  if (!db || !n) {return LFX_ERR_INVALID_ARGUMENT;}
  *n = db->n;
  return LFX_OK;
}

int lfx_place_db_download(lfx_ctx * c, const lfx_place_db * db, uint32_t first, uint32_t count, float * desc_out, void * stream)
{
  if (!c || !db || (count && !desc_out)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_db(c, db) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (first > db->n || count > db->n - first) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "entries outside the place index");}
  if (count == 0) {return LFX_OK;}
  Call k(c, stream);
  hipStream_t st = k.st;
  LFX_TRY(k.open());
  LFX_TRY(k.read(db->added));
  const size_t cells = cells_of(db->cfg);
  LFX_HIP(c, hipMemcpyAsync(desc_out, db->desc.p + (size_t)first * cells, sizeof(float) * cells * count, hipMemcpyDeviceToHost, st));
  LFX_HIP(c, hipStreamSynchronize(st));
  return LFX_OK;
}

int lfx_place_db_query(lfx_ctx * c, const lfx_place_db * db, const float * d_desc, uint32_t n_queries, uint32_t first, uint32_t count,
  uint32_t k, lfx_place_match * matches, void * stream)
{
  if (!c || !db || !d_desc || !matches) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_db(c, db) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (n_queries == 0 || n_queries > 65535u) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "n_queries must be in 1 .. 65535");}
  if (k < 1u || k > LFX_PLACE_MAX_MATCHES) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "k must be in 1 .. 16");}
  if (first > db->n || count > db->n - first) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "entries outside the place index");}
  Call call(c, stream);
  hipStream_t st = call.st;
  LFX_TRY(call.open());
  const uint32_t R = db->cfg.n_rings, S = db->cfg.n_sectors;
  const size_t cells = (size_t)R * S, pairs = (size_t)n_queries * count, n_matches = (size_t)n_queries * k;
  if (hold(db->query_norms, (size_t)n_queries * S) != hipSuccess || hold(db->best_distance, pairs) != hipSuccess ||
    hold(db->best_shift, pairs) != hipSuccess || hold(db->matches, n_matches) != hipSuccess ||
    db->h_matches.reserve(sizeof(lfx::PlaceMatchDevice) * n_matches) != hipSuccess)
  {
    (void)hipGetLastError();
    return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the query's workspace");
  }
  LFX_TRY(call.read(db->added));
  lfx_scan_context_config cfg = db->cfg;
  LFX_TRY(launch_norms(c, d_desc, db->query_norms.p, n_queries, cfg, st));
  if (count) {
    lfx::PlaceCompareArgs a{};
    a.query = d_desc; a.query_norms = db->query_norms.p;
    a.entries = db->desc.p + (size_t)first * cells; a.entry_norms = db->norms.p + (size_t)first * S;
    a.best_distance = db->best_distance.p; a.best_shift = db->best_shift.p;
    a.count = count; a.R = R; a.S = S;
    a.tile = lfx::place_tile(S, pairs);
    const dim3 grid(blocks_for(count, a.tile), n_queries);
    hipLaunchKernelGGL(lfx::place_compare_kernel, grid, dim3(lfx::kPlaceThreads), (uint32_t)lfx::place_compare_lds(R, S), st, a);
    LFX_HIP(c, hipGetLastError());
  }
  hipLaunchKernelGGL(lfx::place_select_kernel, dim3(n_queries), dim3(lfx::kPlaceThreads), 0, st, db->best_distance.p, db->best_shift.p, count, first, k,
    db->matches.p, static_cast<const uint32_t *>(nullptr), static_cast<const uint32_t *>(nullptr));
  LFX_HIP(c, hipGetLastError());
  LFX_HIP(c, hipMemcpyAsync(db->h_matches.p, db->matches.p, sizeof(lfx::PlaceMatchDevice) * n_matches, hipMemcpyDeviceToHost, st));
  LFX_HIP(c, hipStreamSynchronize(st));
  write_matches(reinterpret_cast<const lfx::PlaceMatchDevice *>(db->h_matches.p), n_matches, S, matches);
  return LFX_OK;
}

int lfx_place_db_query_gated(lfx_ctx * c, const lfx_place_db * db, const float * d_desc, uint32_t n_queries, const lfx_place_gate * gates,
  const double * d_poses, double radius, uint32_t k, lfx_place_match * matches, uint32_t * n_eligible, void * stream)
{
  if (!c || !db || !d_desc || !gates || !matches) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_db(c, db) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (n_queries == 0 || n_queries > 65535u) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "n_queries must be in 1 .. 65535");}
  if (k < 1u || k > LFX_PLACE_MAX_MATCHES) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "k must be in 1 .. 16");}
  if (!(radius >= 0.0)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "radius must be >= 0 (+inf: no position test)");}
  uint32_t stride = 0;                                   // the largest limit: what the lists and the launches are sized by
  for (uint32_t q = 0; q < n_queries; q++) {
    if (gates[q].limit > db->n) {
      return fail(c, LFX_ERR_INVALID_ARGUMENT, "gate " + std::to_string(q) + ": limit " + std::to_string(gates[q].limit) + " is above the index's " +
               std::to_string(db->n) + " entries");
    }
    stride = std::max(stride, gates[q].limit);
  }
  Call call(c, stream);
  hipStream_t st = call.st;
  LFX_TRY(call.open());
  const uint32_t R = db->cfg.n_rings, S = db->cfg.n_sectors;
  const size_t pairs = (size_t)n_queries * stride, n_matches = (size_t)n_queries * k;
  if (hold(db->query_norms, (size_t)n_queries * S) != hipSuccess || hold(db->best_distance, pairs) != hipSuccess ||
    hold(db->best_shift, pairs) != hipSuccess || hold(db->list, pairs) != hipSuccess || hold(db->matches, n_matches) != hipSuccess ||
    hold(db->gates, n_queries) != hipSuccess || hold(db->n_eligible, n_queries) != hipSuccess ||
    db->h_matches.reserve(sizeof(lfx::PlaceMatchDevice) * n_matches) != hipSuccess ||
    db->h_gates.reserve(sizeof(lfx::PlaceGate) * n_queries) != hipSuccess || db->h_eligible.reserve(sizeof(uint32_t) * n_queries) != hipSuccess)
  {
    (void)hipGetLastError();
    return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the query's workspace");
  }
  LFX_TRY(call.read(db->added));
  // (the call is synchronous: the pinned blocks are free again when it returns)
  static_assert(sizeof(lfx::PlaceGate) == sizeof(lfx_place_gate), "the kernel's gate is the header's");
  std::memcpy(db->h_gates.p, gates, sizeof(lfx::PlaceGate) * n_queries);
  LFX_HIP(c, hipMemcpyAsync(db->gates.p, db->h_gates.p, sizeof(lfx::PlaceGate) * n_queries, hipMemcpyHostToDevice, st));
  lfx_scan_context_config cfg = db->cfg;
  LFX_TRY(launch_norms(c, d_desc, db->query_norms.p, n_queries, cfg, st));
  hipLaunchKernelGGL(lfx::place_gate_kernel, dim3(n_queries), dim3(lfx::kPlaceThreads), 0, st, db->gates.p, d_poses, radius * radius, stride, db->list.p,
    db->n_eligible.p);
  LFX_HIP(c, hipGetLastError());
  if (stride) {
    lfx::PlaceCompareArgs a{};
    a.query = d_desc; a.query_norms = db->query_norms.p;
    a.entries = db->desc.p; a.entry_norms = db->norms.p;
    a.best_distance = db->best_distance.p; a.best_shift = db->best_shift.p;
    a.count = stride; a.R = R; a.S = S;
    // The lists' lengths stay on the device, so the launch is sized by the bound.  Where every entry below the limit is
    // eligible: lfx_place_db_query's tiles, a workgroup to each.  With the position test, which leaves short lists: tiles of
    // one pass, so that a short list spreads over workgroups, and at most about 8 192 workgroups in all, each taking every
    // gridDim.x-th tile up to its list's end (64 queries against 65 536 entries would start a million workgroups otherwise,
    // nearly all of them with nothing to do).
    a.tile = lfx::place_tile(S, pairs);
    uint32_t per_query = blocks_for(stride, a.tile);
    if (d_poses) {
      a.tile = lfx::place_pass_entries(S);
      per_query = std::min(blocks_for(stride, a.tile), std::max(8192u / n_queries, 1u));
    }
    const dim3 grid(per_query, n_queries);
    hipLaunchKernelGGL(lfx::place_compare_gated_kernel, grid, dim3(lfx::kPlaceThreads), (uint32_t)lfx::place_compare_lds(R, S), st, a,
      static_cast<const uint32_t *>(db->list.p), static_cast<const uint32_t *>(db->n_eligible.p), stride);
    LFX_HIP(c, hipGetLastError());
  }
  hipLaunchKernelGGL(lfx::place_select_kernel, dim3(n_queries), dim3(lfx::kPlaceThreads), 0, st, db->best_distance.p, db->best_shift.p, stride, 0u, k,
    db->matches.p, static_cast<const uint32_t *>(db->list.p), static_cast<const uint32_t *>(db->n_eligible.p));
  LFX_HIP(c, hipGetLastError());
  LFX_HIP(c, hipMemcpyAsync(db->h_eligible.p, db->n_eligible.p, sizeof(uint32_t) * n_queries, hipMemcpyDeviceToHost, st));
  LFX_HIP(c, hipMemcpyAsync(db->h_matches.p, db->matches.p, sizeof(lfx::PlaceMatchDevice) * n_matches, hipMemcpyDeviceToHost, st));
  LFX_HIP(c, hipStreamSynchronize(st));
  write_matches(reinterpret_cast<const lfx::PlaceMatchDevice *>(db->h_matches.p), n_matches, S, matches);
  if (n_eligible) {std::memcpy(n_eligible, db->h_eligible.p, sizeof(uint32_t) * n_queries);}
  return LFX_OK;
}

}  // extern "C"
