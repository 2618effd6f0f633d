// lfx_internal.hpp -- what the translation units of liblfx.so share: the context behind lfx_ctx, device / pinned
// buffers, error plumbing.  Not part of the C ABI (include/lfx.h is).
#pragma once

#include "../../include/lfx.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "lfx_kernels_common.hpp"

namespace lfx_host
{

// The unit kernels live in four translation units of their own, one per variant of the parameters (lfx_unit_v0.hip ...
// lfx_unit_v3.hip over lfx_unit_variant.inl; UnitVariant in lfx_kernels_unit.hpp); run_batch launches them through these.
// the padding the unit kernels of variant V are compiled for (lfx::UnitVariant<V>::kPT: lfx_unit_variant.inl checks; 0 = at run time)
constexpr int kUnitVariantPadding[4] = {5, 5, 2, 0};

struct UnitOrgArgs
{
  lfx::Params prm;
  uint32_t cap, flags, max_rings, drop_zero;
  const uint8_t * pts;
  const uint32_t * scan_begin;
  uint32_t * ring_count;
  const lfx::UnitTables * tab;
  const uint32_t * xform, * geom;
};
struct UnitArgs
{
  lfx::Params prm;
  uint32_t cap, flags, max_rings;
  const uint32_t * ring_count;
  const float2 * sxy;
  const float * sz;
  const uint32_t * sidx;
  const lfx::UnitTables * tab;
  uint32_t * defer_count, * defer_list;
  const uint32_t * list_count, * list;
  uint32_t redo_cap;
};
#define LFX_DECLARE_UNIT_LAUNCHERS(V) \
  void launch_unit_org_v##V(int chunks, bool xf, bool holes, dim3 grid, uint32_t lds_pad, hipStream_t st, const UnitOrgArgs & a); \
  void launch_unit_v##V(bool second, int chunks, bool loop, dim3 grid, uint32_t lds_pad, hipStream_t st, const UnitArgs & a);
LFX_DECLARE_UNIT_LAUNCHERS(0) LFX_DECLARE_UNIT_LAUNCHERS(1) LFX_DECLARE_UNIT_LAUNCHERS(2) LFX_DECLARE_UNIT_LAUNCHERS(3)
#undef LFX_DECLARE_UNIT_LAUNCHERS
inline void launch_unit_org(int variant, int chunks, bool xf, bool holes, dim3 grid, uint32_t lds_pad, hipStream_t st, const UnitOrgArgs & a)
{
  switch (variant) {
    case 0: launch_unit_org_v0(chunks, xf, holes, grid, lds_pad, st, a); break;
    case 1: launch_unit_org_v1(chunks, xf, holes, grid, lds_pad, st, a); break;
    case 2: launch_unit_org_v2(chunks, xf, holes, grid, lds_pad, st, a); break;
    default: launch_unit_org_v3(chunks, xf, holes, grid, lds_pad, st, a); break;
  }
}
inline void launch_unit(int variant, bool second, int chunks, bool loop, dim3 grid, uint32_t lds_pad, hipStream_t st, const UnitArgs & a)
{
  switch (variant) {
    case 0: launch_unit_v0(second, chunks, loop, grid, lds_pad, st, a); break;
    case 1: launch_unit_v1(second, chunks, loop, grid, lds_pad, st, a); break;
    case 2: launch_unit_v2(second, chunks, loop, grid, lds_pad, st, a); break;
    default: launch_unit_v3(second, chunks, loop, grid, lds_pad, st, a); break;
  }
}

// Device memory with one owner: freed when the owner goes, moved but never copied.  alloc gives back what the buffer held
// before it asks for more, and a buffer whose alloc failed is empty ({nullptr, 0}).
template<typename T>
struct DevBuf
{
  T * p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf & operator=(const DevBuf &) = delete;
  DevBuf(DevBuf && o) noexcept : p(o.p), n(o.n) {o.p = nullptr; o.n = 0;}
  DevBuf & operator=(DevBuf && o) noexcept
  {
    if (this != &o) {release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0;}
    return *this;
  }
  ~DevBuf() {release();}
  hipError_t alloc(size_t count)       // (16 spare bytes behind the elements)
  {
    release();
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), count * sizeof(T) + 16);
    if (e == hipSuccess) {n = count;} else {p = nullptr;}
    return e;
  }
  void release()
  {
    if (p) {(void)hipFree(p);}
    p = nullptr;
    n = 0;
  }
};
static_assert(!std::is_copy_constructible_v<DevBuf<float>> && !std::is_copy_assignable_v<DevBuf<float>>, "a device buffer has one owner");

// a device buffer that holds at least `need` elements, grown by half again when it must grow -- or, `exact`, to `need` and
// no further: the buffers that are the library's largest at 1 024 scans -- (its contents are not kept)
template<typename T>
hipError_t hold(DevBuf<T> & b, size_t need, bool exact = false)
{
  if (b.n >= need && (b.p || need == 0)) {return hipSuccess;}
  return b.alloc(exact ? need : need + need / 2);
}

// What a _create allocates: `ok` while every buffer was given -- after one that was not, no more are asked for, its error is
// cleared from the runtime, and the sum goes on, so that the refusal names the whole.  device_bytes is `bytes`.
struct DevTotal
{
  bool ok = true;
  uint64_t bytes = 0;
  template<typename T>
  void get(DevBuf<T> & buf, size_t count)
  {
    if (ok && buf.alloc(count) != hipSuccess) {ok = false; (void)hipGetLastError();}
    bytes += (uint64_t)count * sizeof(T);
  }
  std::string refusal(const char * whose) const {return std::string("cannot allocate ") + whose + "'s " + std::to_string(bytes) + " bytes";}
};

// what every _destroy does: the object's device current while its buffers and events go
template<typename T>
void destroy_on(T * o)
{
  if (!o) {return;}
  (void)hipSetDevice(o->device);
  delete o;
}

struct HostScan          // the per-ring lists of one scan (the large arrays live in the pinned result block)
{
  std::vector<uint8_t> ring_status;
  std::vector<uint32_t> ring_count, ring_offset;
  std::vector<uint16_t> ring_id;
};

// Pinned host memory that only ever grows (the results handed to the caller stay valid until the next call); owned as a
// DevBuf is.
struct PinnedBuf
{
  uint8_t * p = nullptr;
  size_t bytes = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf &) = delete;
  PinnedBuf & operator=(const PinnedBuf &) = delete;
  PinnedBuf(PinnedBuf && o) noexcept : p(o.p), bytes(o.bytes) {o.p = nullptr; o.bytes = 0;}
  PinnedBuf & operator=(PinnedBuf && o) noexcept
  {
    if (this != &o) {release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0;}
    return *this;
  }
  ~PinnedBuf() {release();}
  hipError_t reserve(size_t need)
  {
    if (need <= bytes) {return hipSuccess;}
    // (growing is rare; a copy queued on the old block by a call that returned early with an error must not outlive it)
    if (p) {(void)hipDeviceSynchronize();}
    release();
    const size_t want = need + need / 4 + 4096;
    const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), want, hipHostMallocDefault);
    if (e == hipSuccess) {bytes = want;} else {p = nullptr;}
    return e;
  }
  void release()
  {
    if (p) {(void)hipHostFree(p);}
    p = nullptr;
    bytes = 0;
  }
};
static_assert(!std::is_copy_constructible_v<PinnedBuf> && !std::is_copy_assignable_v<PinnedBuf>, "a pinned block has one owner");

// The event behind the last call queued on an object, on whichever stream that went to, and whether anything has waited
// for it since; owned as a DevBuf is.  Another stream is put behind it (order_behind), a call records it behind its own
// work (done, which creates it on first use), and the host waits for it before it rewrites a pinned block or a staging
// buffer that the call reads (settle).  An owner declares its Tail AFTER the buffers it guards: members go in reverse
// order, so the event is waited for before they are freed.  The state is mutable: calls that only read an object take it
// const and still order themselves.  (Defined behind lfx_ctx, whose error text they write.)
struct Tail
{
  mutable hipEvent_t event = nullptr;
  mutable bool pending = false;
  Tail() = default;
  Tail(const Tail &) = delete;
  Tail & operator=(const Tail &) = delete;
  Tail(Tail && o) noexcept : event(o.event), pending(o.pending) {o.event = nullptr; o.pending = false;}
  Tail & operator=(Tail && o) noexcept
  {
    if (this != &o) {release(); event = o.event; pending = o.pending; o.event = nullptr; o.pending = false;}
    return *this;
  }
  ~Tail() {release();}
  int order_behind(lfx_ctx * c, hipStream_t st) const;
  int done(lfx_ctx * c, hipStream_t st) const;
  int settle(lfx_ctx * c) const;
  void release()
  {
    if (event) {(void)hipEventSynchronize(event); (void)hipEventDestroy(event);}
    event = nullptr;
    pending = false;
  }
};
static_assert(!std::is_copy_constructible_v<Tail> && !std::is_copy_assignable_v<Tail>, "a tail event has one owner");

// One slot of a ring that a call's table of constants goes out through: the pinned block it is written to, the device table
// it is copied to, and the event behind the kernels that read either -- so that a call never rewrites a block or a table
// still in use, whichever streams the calls are on.  A slot is sized by the calls that took it and grows on demand.
struct TableSlot
{
  PinnedBuf h;
  DevBuf<double> d;
  Tail used;
  // The kernels that used the slot last (a ring's length of calls ago: long done) waited for, then room for `doubles` on
  // both sides.  LFX_ERR_HIP where the wait fails; what an allocation answered comes back in `mem`, for the caller to word.
  // A failure leaves the slot valid, with what memory it had or none; the caller advances its ring after success.
  int take(lfx_ctx * c, size_t doubles, hipError_t & mem);
};

// The kernel slots of lfx_kernel_times, in the order of the comment on LFX_N_KERNELS (lfx.h); kKernelNames (lfx_api.hip) is
// written in this order
enum KernelSlot : int
{
  kSlotScatter, kSlotUnit, kSlotOrder, kSlotUnitSecond, kSlotExtract, kSlotTotals, kSlotCompact, kSlotUnitOrg, kSlotCut, kSlotTail,
  kSlotGridCount, kSlotReset, kSlotLong,
  kSlotPgLinearize, kSlotPgNode, kSlotPgReduce, kSlotPgChainFactor, kSlotPgChainSolve, kSlotPgAssemble, kSlotPgDiag, kSlotPgPanel, kSlotPgUpdate,
  kSlotPgSolve, kSlotPgStep, kSlotCount
};
static_assert(kSlotCount == LFX_N_KERNELS, "a slot per kernel of lfx_kernel_times");

}  // namespace lfx_host

// The route selection of run_batch (lfx_api.hip, choose_route): what it remembers between batches, the switches that pin
// its choices (tests), what it decides for one batch.
struct RouteState
{
  uint32_t report[lfx::kCounters] = {};  // the counters block of the last batch whose report has landed (lfx_kernels_common.hpp)
  uint32_t report_rings = 0;             // rings of that batch (0 = no report yet)
  bool use_xform = false;                // rings arrive rotated / reversed: ring_cut_kernel ahead of the organised-scan kernel
  bool use_holes = false;                // the grid holds (0, 0, 0) records the zero filter drops: grid_count_kernel + the holes form
  bool bucket_all = false;               // the stream is not organised: bucketing route for every scan
  uint32_t retry_in = 0;                 // ... and the organised-scan kernel is tried again in so many batches
  bool pre_order = false;                // order repair BEFORE the first unit pass (a stream that keeps arriving out of order)
};
struct RoutePins                         // LFX_DEBUG_FUSED / _XFORM / _SHORT_TAIL / _PRE_ORDER (0 / 1; -1 = not pinned), _REDO_CAP (0 = not)
{
  int fused = -1, xform = -1, short_tail = -1, pre_order = -1, holes = -1;
  uint32_t redo_cap = 0;
};
struct RouteChoice
{
  bool fused = false, xform = false, short_tail = false, pre_order = false, holes = false;
  uint32_t fb_grid = 0, redo_cap = 0;
};

struct lfx_ctx
{
  int device = 0;
  lfx_params params{};
  lfx::Params dev{};
  lfx::Layout layout{};
  uint32_t max_points = 0, max_batch = 0, cap = 0, max_chunks = 0, max_rings = 0, ring_threads = 0, slow_grid = 0;
  size_t total_cap = 0, ring_lds = 0, order_lds = 0;
  uint32_t stage_flags = LFX_STAGE_ALL;  // LFX_DEBUG_RING_FLAGS overrides it for slow-kernel ablations (wrong results)
  uint32_t unit_lds_pad = 0;             // LFX_DEBUG_UNIT_LDS_PAD: extra LDS per workgroup (occupancy experiments)
  int unit_variant = 3;                  // which compilation of the unit kernels serves the parameters (UnitVariant, lfx_kernels_unit.hpp)
  uint32_t unit_chunks = 6;              // chunks of 64 positions per unit wave (3..6), from the configured ring length
  uint32_t unit_flags = 65u;             // LFX_DEBUG_UNIT_FLAGS: 1 edge pass, 64 surface pass (ablations only)
  uint32_t drop_zero = 0;                // lfx_config::drop_zero_points
  // What a batch reports about its stream (the counters block behind ring_flags) is copied to pinned memory at the end of
  // the batch, nobody waiting; the next batches' route is chosen from the last report that has LANDED.
  // No event stands behind it: a host that runs ahead of the device (a loop of lfx_extract_batch_device calls, the pipelined
  // pair) would ask about the batch it has just queued and never find that event passed.  The block carries the batch's
  // serial number before and after the counters (feature_compact_kernel writes begin, fence, counters, fence, end; the
  // host reads end, counters, begin): a block whose two serials agree is one batch's report, whichever batch has got that
  // far -- the route follows the stream a few batches behind instead of not at all.
  uint32_t * h_counters = nullptr;       // pinned [1 + lfx::kCounters + 1]
  uint32_t batch_serial = 0;             // serial of the batch queued last (never 0 in the block)
  uint32_t report_taken = 0;             // serial of the report the route state was last fed with
  RouteState route;
  RoutePins route_pins;
  bool pre_order = false;                // this batch's choice (run_batch)
  // The organised-scan kernel (lfx_kernels_extract.hpp, unit_body<ORG>) reads a driver's column-major scan directly; scans
  // that are not of that form fall back to the bucketing route inside the same call (choose_route decides per batch).
  bool fused_possible = false;
  bool last_used_xform = false;          // the last batch's organised-scan kernel ran with the ring transforms
  int totals_env = -1;                   // LFX_DEBUG_TOTALS_KERNEL=1: ring_totals_kernel also for small batches (A/B)
  bool fast_path = true;                 // wave-per-unit kernel first, workgroup-per-ring kernel for what it defers
  std::string err;
  lfx_log_fn log_cb = nullptr;           // lfx_set_log_callback
  void * log_user = nullptr;

  // device scratch
  lfx_host::DevBuf<uint32_t> scan_begin, scan_geom, scan_info, chunk_base, chunk_flags, ring_count, ring_nedge,
    ring_nsurf, ring_ebase, ring_sbase, ring_flags, unit_ne, unit_ns, unit_span, slow_list, defer_list, redo_list, fb_list, xform,
    sidx, rec_idx, edge_idx,
    surf_idx, d_sidx, counters, scan_flags, tail_ticket;
  // Ring ids that are not 0 .. max_rings-1 (lfx_config.ring_ids, lfx_set_ring_ids, or found by the host entry points in a
  // scan that carried another id): slot_id[k] = the id of slot k (ascending), ring_slot the device table id -> slot the
  // bucketing kernel reads; empty = the id is the slot.  ids_given: the caller said so (no looking up by the library).
  lfx_host::DevBuf<uint16_t> ring_slot;
  std::vector<uint16_t> slot_id;
  bool ids_given = false, organised_by_config = false;
  lfx_host::DevBuf<uint16_t> cum16;      // grid_count_kernel's prefix table (the holes form; contexts with the zero filter on)
  lfx_host::DevBuf<uint4> hole_desc;     // ... and its unit descriptors
  // Contexts whose ring capacity is above LFX_MAX_RING_POINTS (long rings, ring_long_kernel): the long list ({entry, how}
  // pairs, one per ring id and scan), its length (zeroed ahead of every batch) and the kernel's workspace, long_slices
  // slices of long_slice_bytes in HBM.  Empty in every other context.
  lfx_host::DevBuf<uint32_t> long_list, long_count;
  lfx_host::DevBuf<uint8_t> long_work;
  uint32_t long_slices = 0;
  size_t long_slice_bytes = 0;
  // The batch's accumulators (counters, scan_flags, ring_nedge / ring_nsurf) exist twice: batch k uses set `parity`, its
  // compaction zeroes the other one over the scans the batch before last left dirty there (par_dirty).  aux_dirty: scans whose
  // bucketing-route tables (look-back flags, ring flags, ring transforms) a batch since the last reset may have touched.
  uint32_t parity = 0, par_dirty[2] = {0u, 0u}, aux_dirty = 0;
  uint32_t scan_count_from = 256;        // batches of so many scans take scan_count_kernel for the holes form's count pass (LFX_DEBUG_SCAN_COUNT_FROM)
  lfx_host::DevBuf<uint8_t> ring_status, label_s, staging, d_label;
  lfx_host::DevBuf<double> d_curv;
  lfx_host::DevBuf<float2> sxy;
  lfx_host::DevBuf<float> sz;
  lfx_host::DevBuf<double> curv_s;
  lfx_host::DevBuf<float4> edge_pts, surf_pts, rec_pts;
  lfx_host::DevBuf<float4> rec32;         // the record slots of the unit kernels (lfx_kernels_common.hpp rec_slot_places)
  uint32_t slot_places = 64;              // places per slot: what the context's unit kernels are compiled for
  lfx_host::DevBuf<lfx::UnitTables> unit_tab;      // the unit kernel's output pointers (one element)
  lfx_host::DevBuf<uint32_t> vox_scratch;          // lfx_voxel_downsample: sort keys / values, allocated on first use
  lfx_host::DevBuf<double> align_scratch;          // lfx_scan_to_map_align: states, rows, errors; allocated on first use
  lfx_host::DevBuf<float> align_surface;           // lfx_localize_batch: the downsampled surface clouds (+ counts, status)
  lfx_host::PinnedBuf h_align;                     // the alignment's small copies to and from the host (poses, counts, states)
  lfx_host::PinnedBuf h_loc;                       // lfx_localize_batch: the clouds' lengths as the device saw them, [batch][2]
  bool vox_lds_asked = false;                      // the voxel-grid kernel has been granted its 144 KB of dynamic LDS on this device
  int align_guess = 4;                             // iterations the previous alignment needed: so many are queued before the host looks
  uint32_t loc_guess[2] = {0u, 0u};                // longest edge / downsampled surface cloud of the previous lfx_localize_batch

  // lfx_deskew_batch, lfx_deskew_batch_trajectory (lfx_deskew.hip): a call's table of constants goes out through the next of
  // a ring of kDeskewSlots table slots (TableSlot; `used` is recorded behind the kernel that read d).  deskewed_in_place: the
  // last batch's clouds have been de-skewed in place (a second de-skew would correct them twice); run_batch lifts it
  static constexpr uint32_t kDeskewSlots = 8;
  using DeskewSlot = lfx_host::TableSlot;
  DeskewSlot deskew_slots[kDeskewSlots];
  uint32_t deskew_next = 0;
  bool deskewed_in_place = false;

  // lfx_scan_context_batch (lfx_place.hip): a call's tables go out as the de-skew's do, through the next of a ring of slots,
  // each with the call's cell keys ([scans][R * S] u32) beside the table (`used` is recorded behind the kernel that turned
  // the keys into the caller's floats; declared first, the keys go after it has been waited for).
  static constexpr uint32_t kPlaceSlots = 4;
  struct PlaceSlot
  {
    lfx_host::DevBuf<uint32_t> keys;
    lfx_host::TableSlot table;
  };
  PlaceSlot place_slots[kPlaceSlots];
  uint32_t place_next = 0;

  // lfx_segment_batch, lfx_pack_features_segmented (lfx_segment.hip): the range images of one chunk of scans (at most
  // LFX_SEGMENT_BUDGET_CELLS cells, grown on demand), the filtered pack's counts, and an event behind the last call that used
  // any of it: the next call's stream waits for it, so that calls on different streams take the workspace one behind the other.
  // The tables of the kSegTables configs seen last stay on the device, each with the pinned block it went up from; a slot
  // is refilled (its block rewritten) only after the event has passed, so no call waits for its stream.
  struct SegmentWork
  {
    static constexpr uint32_t kSegTables = 4;
    struct Table
    {
      lfx_host::DevBuf<double> d;
      lfx_host::PinnedBuf h;
      uint32_t columns = 0;              // 0: empty
      float row_step = 0.0f;
    };
    lfx_host::DevBuf<uint64_t> image;
    lfx_host::DevBuf<float4> cell;
    lfx_host::DevBuf<uint32_t> parent, csize, crowmax, pack_counts;
    Table tables[kSegTables];
    uint32_t table_next = 0;             // the slot the next unseen config takes
    lfx_host::Tail used;
  };
  SegmentWork seg;

  hipStream_t stream = nullptr;          // used by the synchronous host entry points
  std::vector<uint32_t> h_scan_begin;    // of the last batch
  std::vector<uint32_t> h_scan_geom;     // [batch][kGeomStride]: columns per ring and block boundaries of every scan (organised-scan kernel)
  std::vector<uint32_t> uploaded_begin;  // what scan_begin on the device currently holds
  uint32_t last_batch = 0;
  const void * last_points = nullptr;
  std::vector<lfx_host::HostScan> host;
  uint32_t outputs = LFX_OUT_ALL;        // lfx_config::outputs
  lfx_host::PinnedBuf h_in, h_out;                 // staging of the synchronous host API (allocated on first use)
  // lfx_extract_submit / lfx_extract_wait: two scans in flight, each with its own device input, pinned staging and result
  // block; the uploads run on copy_stream beside the kernels of the scan before
  struct Slot
  {
    lfx_host::DevBuf<uint8_t> in;
    lfx_host::PinnedBuf hin, hout;
    hipEvent_t uploaded = nullptr, done = nullptr;
    uint64_t ticket = 0;
    bool busy = false;
    void * plan = nullptr;               // FetchPlan (lfx_api.hip)
    lfx_host::HostScan host;
  };
  Slot slots[2];
  hipStream_t copy_stream = nullptr;
  uint64_t next_ticket = 1, next_wait = 1;
  uint32_t * h_status = nullptr;         // pinned, lfx_batch_status

  bool profiling = false;
  uint32_t profile_every = 1, batch_no = 0;   // lfx_set_profiling_interval: events around every n-th batch only
  bool profile_now = false;
  struct Span { hipEvent_t a, b; int k; };
  std::vector<Span> spans;
  std::vector<hipEvent_t> free_events;
  double ms[LFX_N_KERNELS] = {};
  uint64_t launches[LFX_N_KERNELS] = {};
};

namespace lfx {struct OccEmitArgs;}     // lfx_kernels_occvalue.hpp

namespace lfx_host
{

std::string & create_error();          // what lfx_last_error(NULL) reports (lfx_api.hip)

// lfx_kernel_times: a pair of events around one launch (or a few) on `s`, kept in the context's spans until they are drained,
// where `on`; events are reused.  The extraction's batches pass profile_now (lfx_set_profiling_interval samples batches); the
// pose graph has no batches and passes profiling.
inline hipEvent_t take_event(lfx_ctx * c)
{
  if (!c->free_events.empty()) {
    hipEvent_t e = c->free_events.back();
    c->free_events.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}
struct TimedSpan
{
  TimedSpan(lfx_ctx * c, bool on, int k, hipStream_t s)
  : c_(c), on_(on), k_(k), s_(s)
  {
    if (on_) {
      a_ = take_event(c_);
      b_ = take_event(c_);
      (void)hipEventRecord(a_, s_);
    }
  }
  ~TimedSpan()
  {
    if (on_) {
      (void)hipEventRecord(b_, s_);
      c_->spans.push_back({a_, b_, k_});
    }
  }
  TimedSpan(const TimedSpan &) = delete;
  TimedSpan & operator=(const TimedSpan &) = delete;
  lfx_ctx * c_;
  bool on_;
  int k_;
  hipStream_t s_;
  hipEvent_t a_ = nullptr, b_ = nullptr;
};

#define LFX_HIP(ctx, call) \
  do { \
    const hipError_t e_ = (call); \
    if (e_ != hipSuccess) { \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_); \
      return LFX_ERR_HIP; \
    } \
  } while (0)

inline int fail(lfx_ctx * ctx, int code, const std::string & msg)
{
  if (ctx) {ctx->err = msg;}
  return code;
}

inline int Tail::order_behind(lfx_ctx * c, hipStream_t st) const
{
  if (pending) {LFX_HIP(c, hipStreamWaitEvent(st, event, 0));}
  return LFX_OK;
}
inline int Tail::done(lfx_ctx * c, hipStream_t st) const
{
  if (!event) {LFX_HIP(c, hipEventCreateWithFlags(&event, hipEventDisableTiming));}
  LFX_HIP(c, hipEventRecord(event, st));
  pending = true;
  return LFX_OK;
}
inline int Tail::settle(lfx_ctx * c) const
{
  if (pending) {LFX_HIP(c, hipEventSynchronize(event)); pending = false;}
  return LFX_OK;
}

inline int TableSlot::take(lfx_ctx * c, size_t doubles, hipError_t & mem)
{
  const int rs = used.settle(c);
  if (rs != LFX_OK) {return rs;}
  mem = h.reserve(sizeof(double) * doubles);
  if (mem == hipSuccess) {mem = hold(d, doubles);}
  if (mem != hipSuccess) {(void)hipGetLastError();}     // (the caller words `mem`; the runtime's last error is cleared here)
  return LFX_OK;
}

// an object made on one device handed to a context of another: `what` names it ("the mapper", ...)
inline int check_device(lfx_ctx * c, int device, const char * what)
{
  if (device != c->device) {return fail(c, LFX_ERR_INVALID_ARGUMENT, std::string(what) + " lives on another device");}
  return LFX_OK;
}

#define LFX_TRY(call) \
  do { \
    const int rc_ = (call); \
    if (rc_ != LFX_OK) {return rc_;} \
  } while (0)

// One call's scope on one stream over the tails of the objects it touches (up to kTails; nothing allocated).  A call opens
// (the device), puts itself behind each tail -- `behind` on the stream, `after` on the host, where the host is about to
// rewrite a block the tail guards -- queues its work on `st` and finishes: every tail taken is recorded, in the order taken.
// A call that leaves early, by whichever return, records them as it goes out of scope, so that the next call on another
// stream waits for what this one did queue; the call's own error text stays.  `read` orders the stream and `wait` waits on
// the host, and neither takes anything: the views, and the reads that end in a wait of their own.  `record` records the
// taken tails in the middle of a call and keeps them: behind a table that went up, before the call orders itself again.
struct Call
{
  static constexpr int kTails = 4;
  lfx_ctx * c;
  hipStream_t st;
  Call(lfx_ctx * ctx, void * stream) : c(ctx), st(static_cast<hipStream_t>(stream)) {}
  Call(const Call &) = delete;
  Call & operator=(const Call &) = delete;
  ~Call()
  {
    if (n == 0) {return;}
    std::string said;                    // (a record that fails here does not reword the failure the call returned with)
    said.swap(c->err);
    (void)record();
    c->err.swap(said);
  }
  int open() {LFX_HIP(c, hipSetDevice(c->device)); return LFX_OK;}
  int behind(const Tail & t) {LFX_TRY(t.order_behind(c, st)); return take(t);}
  int after(const Tail & t) {LFX_TRY(t.settle(c)); return take(t);}
  int read(const Tail & t) const {return t.order_behind(c, st);}
  int wait(const Tail & t) const {return t.settle(c);}
  int take(const Tail & t)               // (a tail taken twice is recorded once)
  {
    for (int i = 0; i < n; i++) {
      if (taken[i] == &t) {return LFX_OK;}
    }
    if (n == kTails) {return fail(c, LFX_ERR_CAPACITY, "a call over more tails than lfx_host::Call holds");}
    taken[n++] = &t;
    return LFX_OK;
  }
  int record() const
  {
    int rc = LFX_OK;
    for (int i = 0; i < n; i++) {
      const int r = taken[i]->done(c, st);
      rc = rc != LFX_OK ? rc : r;
    }
    return rc;
  }
  int finish()
  {
    const int rc = record();
    n = 0;
    return rc;
  }
  const Tail * taken[kTails] = {};
  int n = 0;
};

// a small block of the device down through a pinned block, waited for: counters, stats, a plan's record
inline int read_block(lfx_ctx * c, const PinnedBuf & pinned, const void * d_src, size_t bytes, hipStream_t st)
{
  LFX_HIP(c, hipMemcpyAsync(pinned.p, d_src, bytes, hipMemcpyDeviceToHost, st));
  LFX_HIP(c, hipStreamSynchronize(st));
  return LFX_OK;
}
// a small table up through a pinned block, which the caller has settled (Call::after); src null: the caller wrote the block
inline int send_block(lfx_ctx * c, PinnedBuf & up, void * d_dst, const void * src, size_t bytes, hipStream_t st)
{
  LFX_HIP(c, up.reserve(bytes));
  if (src) {std::memcpy(up.p, src, bytes);}
  LFX_HIP(c, hipMemcpyAsync(d_dst, up.p, bytes, hipMemcpyHostToDevice, st));
  return LFX_OK;
}

// An object's pose table, [n][12] doubles on the device behind its tail: entries [first, first + count) set from the host
// through the object's upload block, read back, or copied from the same entries of another table on the device.  The
// caller has checked the range and that count is not 0.
inline int poses_set(Call & k, const Tail & tail, DevBuf<double> & d, PinnedBuf & upload, uint32_t first, uint32_t count, const double * poses)
{
  LFX_TRY(k.open());
  LFX_TRY(k.after(tail));
  LFX_TRY(send_block(k.c, upload, d.p + 12u * (size_t)first, poses, sizeof(double) * 12u * count, k.st));
  return k.finish();
}
inline int poses_get(Call & k, const Tail & tail, const DevBuf<double> & d, uint32_t first, uint32_t count, double * poses_out)
{
  LFX_TRY(k.open());
  LFX_TRY(k.read(tail));
  LFX_HIP(k.c, hipMemcpyAsync(poses_out, d.p + 12u * (size_t)first, sizeof(double) * 12u * count, hipMemcpyDeviceToHost, k.st));
  LFX_HIP(k.c, hipStreamSynchronize(k.st));
  return LFX_OK;
}
inline int poses_follow(Call & k, const Tail & tail, DevBuf<double> & d, const double * d_poses, uint32_t first, uint32_t count)
{
  LFX_TRY(k.open());
  LFX_TRY(k.behind(tail));
  LFX_HIP(k.c, hipMemcpyAsync(d.p + 12u * (size_t)first, d_poses + 12u * (size_t)first, sizeof(double) * 12u * count, hipMemcpyDeviceToDevice, k.st));
  return k.finish();
}

// the 2-D grids' sides (occupancy grids, distance fields, the grid matcher's field), and two of them that must agree
inline bool grid_sides_ok(uint32_t width, uint32_t height)
{
  return width >= 1u && width <= LFX_OCCUPANCY_MAX_SIDE && height >= 1u && height <= LFX_OCCUPANCY_MAX_SIDE;
}
inline int check_same_cells(lfx_ctx * c, const char * a, uint32_t aw, uint32_t ah, const char * b, uint32_t bw, uint32_t bh)
{
  if (aw == bw && ah == bh) {return LFX_OK;}
  return fail(c, LFX_ERR_INVALID_ARGUMENT, std::string(a) + " is " + std::to_string(aw) + " x " + std::to_string(ah) + " cells, " + b + " " +
           std::to_string(bw) + " x " + std::to_string(bh));
}

inline bool finite_all(const double * v, size_t n)
{
  for (size_t i = 0; i < n; i++) {
    if (!std::isfinite(v[i])) {return false;}
  }
  return true;
}

// the parts of a pinned block start on 64-byte boundaries (tables of doubles; a copy up starts aligned)
inline size_t round64(size_t bytes) {return (bytes + 63u) & ~(size_t)63u;}

// workgroups of `threads` (or tiles of that many items) that cover n items
inline uint32_t blocks_for(uint64_t n, uint32_t threads) {return (uint32_t)((n + threads - 1u) / threads);}

// The grid of a kernel that walks every scan's records with a grid stride, (chunks, scans): a scan of 64 x 1800 has 115 k
// input records, which 32 workgroups of 256 walk in 15 steps; large batches fill the device with fewer (the de-skews walk
// feature records with it, an eighth as many).
inline dim3 by_scan_grid(uint32_t n_scans) {return dim3(n_scans >= 32u ? 8u : 32u, n_scans);}

// whether the batch's input records are the canonical ones load_xyz<true> reads (lfx_kernels_image.hpp): x, y, z
// little-endian in the first 12 bytes of 32-byte records that start 16-byte aligned
inline bool canonical_xyz16(const lfx::Layout & L, const void * pts)
{
  return L.step == 32u && L.ox == 0u && L.oy == 4u && L.oz == 8u && !L.be && (reinterpret_cast<uintptr_t>(pts) & 15u) == 0u;
}

// One list of n clouds on the device, as the stores' add and insert calls are handed it: cloud s is d_count[s *
// count_stride] records from record d_begin[s] of total_points.  name: what a refusal calls the list ("", "edge ", "surface ")
struct CloudList
{
  const uint32_t * d_begin = nullptr, * d_count = nullptr;
  uint32_t count_stride = 1;
  uint64_t total_points = 0;
  const char * name = "";
};
// the counts (a strided span, read whole) and begins of n clouds as read_lists reads one list back
inline size_t readback_bytes(uint32_t n, uint32_t stride) {return sizeof(uint32_t) * ((size_t)(n - 1) * stride + 1 + n);}

// The begins and counts of the n clouds of each of n_lists lists (1 or 2) into begin[l] / count[l], through `pinned`
// (readback_bytes of each list, one behind the other): every copy queued on st, then one wait, the calling call's only
// one.  A cloud that runs past its list's total_points is refused.
inline int read_lists(lfx_ctx * c, const CloudList * lists, int n_lists, uint32_t n, uint8_t * pinned, std::vector<uint32_t> * begin,
  std::vector<uint32_t> * count, hipStream_t st)
{
  const uint32_t * h_count[2];
  uint32_t * at = reinterpret_cast<uint32_t *>(pinned);
  for (int l = 0; l < n_lists; l++) {
    const size_t span = (size_t)(n - 1) * lists[l].count_stride + 1;
    h_count[l] = at;
    LFX_HIP(c, hipMemcpyAsync(at, lists[l].d_count, sizeof(uint32_t) * span, hipMemcpyDeviceToHost, st));
    LFX_HIP(c, hipMemcpyAsync(at + span, lists[l].d_begin, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, st));
    at += span + n;
  }
  LFX_HIP(c, hipStreamSynchronize(st));
  for (int l = 0; l < n_lists; l++) {
    const uint32_t * h_begin = h_count[l] + (size_t)(n - 1) * lists[l].count_stride + 1;
    begin[l].assign(h_begin, h_begin + n);
    count[l].resize(n);
    for (uint32_t s = 0; s < n; s++) {
      count[l][s] = h_count[l][(size_t)s * lists[l].count_stride];
      if ((uint64_t)begin[l][s] + count[l][s] > lists[l].total_points) {
        return fail(c, LFX_ERR_INVALID_ARGUMENT, std::string(lists[l].name) + "cloud " + std::to_string(s) + " (records " + std::to_string(begin[l][s]) +
                 " + " + std::to_string(count[l][s]) + ") runs past total_points (" + std::to_string(lists[l].total_points) + ")");
      }
    }
  }
  return LFX_OK;
}

// The pinned block of a store whose calls read lists back into [0, pin_table) and send their table of entries up from
// pin_table on: room for a read-back of `need` bytes and `entries` entries of `entry_bytes` behind it.  The block may move,
// so what was queued behind `tail` is waited for first: nothing may still read the table in it.
inline int grow_readback(const Call & k, const Tail & tail, PinnedBuf & pinned, size_t & pin_table, size_t need, size_t entry_bytes, size_t entries)
{
  if (need <= pin_table) {return LFX_OK;}
  LFX_TRY(k.wait(tail));
  const size_t at = round64(need);
  LFX_HIP(k.c, pinned.reserve(at + entry_bytes * entries));
  pin_table = at;
  return LFX_OK;
}

// the calls that work on the last batch: the caller's arrays are sized by ITS count (one pose after a batch of 16 would be
// read and written 15 entries too far)
inline int check_last_batch(lfx_ctx * c, uint32_t n_scans)
{
  if (c->last_batch == 0) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "no batch has been extracted yet");}
  if (n_scans != c->last_batch) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "n_scans (" + std::to_string(n_scans) + ") is not the number of scans of the last batch (" +
             std::to_string(c->last_batch) + ")");
  }
  return LFX_OK;
}

// lfx_downsample.hip: lfx_voxel_downsample with the extras of lfx_localize_batch
int voxel_downsample(
  lfx_ctx * c, const float * d_points, const uint32_t * d_begin, const uint32_t * d_count, uint32_t count_stride,
  uint32_t n_clouds, size_t total_points, float leaf, float * d_out, uint32_t * d_out_count, uint32_t * d_status, void * stream,
  bool unfiltered, const uint32_t * d_other_count, uint32_t * lengths);

// lfx_deskew.hip: scans first .. first + n - 1 of the last batch de-skewed by sweeps[0 .. n - 1] into buffers laid out like
// the context's clouds (lfx_deskew_batch's checks; lfx_odometry_update_batch_deskewed takes one scan at a time)
int deskew_scans(lfx_ctx * c, const lfx_time_field * time, const lfx_sweep * sweeps, uint32_t first, uint32_t n, int to,
  float4 * edge_out, float4 * surf_out, hipStream_t st);
// what is refused about trajectories[0 .. n - 1], nothing touched (lfx_odometry_update_batch_trajectory asks before its first scan)
int check_trajectories(lfx_ctx * c, const lfx_trajectory * trajectories, uint32_t n);
// deskew_scans along trajectories[0 .. n - 1] (lfx_deskew_batch_trajectory's checks; lfx_odometry_update_batch_trajectory)
int deskew_scans_trajectory(lfx_ctx * c, const lfx_time_field * time, const lfx_trajectory * trajectories, uint32_t first, uint32_t n,
  float4 * edge_out, float4 * surf_out, hipStream_t st);

// lfx_localize.hip: a map rebuilt in place (lfx_odometry.hip's window maps) and the optimizer over clouds
lfx_map * map_new(int device);
int map_rebuild(lfx_ctx * c, lfx_map * m, const float * d_points, uint32_t n_points, float cell_size, const double lo[3],
  const double hi[3], hipStream_t st);
// one kind of cloud of a set of scans, as the alignment is handed it (device pointers; lfx_scan_to_map_align's arguments)
struct CloudSpan
{
  const float * points = nullptr;          // records of 4 floats
  const uint32_t * begin = nullptr, * count = nullptr;   // cloud s: count[s * count_stride] records from record begin[s]
  uint32_t count_stride = 1, longest = 0;  // (longest: what the launches are sized by)
  // where each cloud's ROWS start in the residuals and Jacobians ([n_clouds]); null: where its points start.  total counts
  // rows: with compact row starts the scratch is sized by the clouds' real lengths, not by the layout the points happen to
  // lie in (lfx_localize_batch: scan s's clouds start at its first input point)
  size_t total = 0;
  const uint32_t * row_begin = nullptr;
};
// lfx_wire.hip: the [2][batch + 1] offsets table of lfx_pack_features from two arrays of per-scan counts `stride` words apart
// (feature_offsets_kernel; lfx_pack_features_segmented hands it its own counts)
void launch_feature_offsets(const uint32_t * edge_counts, const uint32_t * surface_counts, uint32_t stride, uint32_t batch,
  uint32_t * d_offsets, hipStream_t st);

// lfx_place.hip: where an index keeps its descriptors on the device ([entries][*cells] floats, cells = R * S) -- a loop
// closer's detect queries the index with its own entries (lfx_loopclose.hip)
const float * place_db_entries(const lfx_place_db * db, uint32_t * cells);

// lfx_keyframes.hip: a store as the visibility votes (lfx_visibility.hip) and the voxel filter (lfx_voxelfilter.hip) read it
// -- the device arrays, the host's mirror of the begin tables ([n + 1] per kind) and the store's tail event, which a reader
// orders itself behind and records
struct KeyframesAccess
{
  int device = 0;
  uint32_t n = 0;
  bool has_flags = false;               // lfx_keyframes_reserve_flags has run
  const float4 * records[2] = {nullptr, nullptr};
  const uint64_t * d_begin[2] = {nullptr, nullptr};
  const uint64_t * begin[2] = {nullptr, nullptr};
  const double * poses = nullptr;
  const uint8_t * flags[2] = {nullptr, nullptr};   // the store's own flags (has_flags)
  float4 * scratch = nullptr;           // lfx_keyframes_save's chunk of a world cloud: `chunk` records
  uint64_t chunk = 0;
  const Tail * tail = nullptr;
};
KeyframesAccess keyframes_access(const lfx_keyframes * s);

// lfx_odometry.hip: the event behind the store's last append, for lfx_odometry_save (lfx_mapping.hip) to read behind
const Tail & odometry_tail(const lfx_odometry * o);

// What a reader of an occupancy grid's counts needs (lfx_occupancy.hip; the distance field reads them in place): the two
// count arrays, the emit's table on the device and the tail event the reader orders itself behind and moves.
struct OccupancyAccess
{
  int device = 0;
  uint32_t width = 0, height = 0;
  const uint32_t * hits = nullptr, * misses = nullptr;
  const int8_t * lut = nullptr;
  const Tail * tail = nullptr;
  // ... and a reader of its scans (lfx_gridmatch.hip): the beams [n_scans][n_beams] and the poses [n_scans][12]
  const uint4 * beams = nullptr;
  const double * poses = nullptr;
  uint32_t n_scans = 0, n_beams = 0;
  // the emit of `cfg` over the counts: everything of `a` but where the bytes go (lfx_occupancy.hip)
  void emit_args(const lfx_occupancy_emit_config & cfg, lfx::OccEmitArgs & a) const;
};
OccupancyAccess occupancy_access(const lfx_occupancy * g);
// What a reader of a distance field's d2 needs (lfx_distance.hip; the grid matcher's score field is a look-up of it): the
// array, the last transform's cap and the tail event the reader orders itself behind and moves.
struct DistanceAccess
{
  int device = 0;
  uint32_t width = 0, height = 0;
  bool transformed = false;
  uint32_t cap = 0;
  const uint32_t * d2 = nullptr;
  const Tail * tail = nullptr;
};
DistanceAccess distance_access(const lfx_distance * f);
// the emit's table of `config` put on the device as lfx_occupancy_emit puts it (nothing is sent for the config of the call
// before); LFX_ERR_INVALID_ARGUMENT, before anything is queued: what lfx_occupancy_emit_table refuses
int occupancy_put_table(Call & k, lfx_occupancy * g, const lfx_occupancy_emit_config & config);

int align_clouds(
  lfx_ctx * c, const lfx_map * edge_map, const lfx_map * surface_map, uint32_t n_neighbors, int max_iter, const CloudSpan & edge,
  const CloudSpan & surface, uint32_t n_clouds, const double * initial_poses, lfx_align_result * results, void * stream,
  lfx_align_report * reports = nullptr);

// The front of lfx_localize_batch, lfx_odometry_update_batch and lfx_rolling_map_update_batch: the last batch's surface clouds
// downsampled once into the caller's buffer (the clouds, a count and a status per scan, then what else the caller keeps
// there), the scans' lengths left in the caller's pinned block on the way ([batch][2]: edge count, downsampled length),
// behind the batch's scan_info ([batch][4]) where the caller reads it.
struct BatchFront
{
  float * down = nullptr;
  uint32_t * down_count = nullptr, * down_status = nullptr;
  uint32_t * info = nullptr, * lengths = nullptr;
  // room in `pinned` from word `at` on: [batch][4] info where with_info, then [batch][2] lengths
  int pin(lfx_ctx * c, PinnedBuf & pinned, size_t at, bool with_info)
  {
    const size_t batch = c->last_batch, info_words = with_info ? 4 * batch : 0;
    LFX_HIP(c, pinned.reserve(sizeof(uint32_t) * (at + info_words + 2 * batch)));
    uint32_t * const w = reinterpret_cast<uint32_t *>(pinned.p) + at;
    info = with_info ? w : nullptr;
    lengths = w + info_words;
    return LFX_OK;
  }
  // every scan's counts on the host: one wait
  int read_info(lfx_ctx * c, hipStream_t st) const
  {
    LFX_HIP(c, hipMemcpyAsync(info, c->scan_info.p, sizeof(uint32_t) * 4 * c->last_batch, hipMemcpyDeviceToHost, st));
    LFX_HIP(c, hipStreamSynchronize(st));
    return LFX_OK;
  }
};
// (words_per_scan: count and status included; `exact`: hold's.  A cloud PCL hands back unfiltered -- a leaf too small for its
// extent -- is copied.  Waits, in read_info, where with_info, else for nothing.)
inline int batch_front(lfx_ctx * c, DevBuf<float> & buf, uint32_t words_per_scan, bool exact, PinnedBuf & pinned, size_t at, bool with_info,
  float leaf, hipStream_t st, BatchFront & f)
{
  const uint32_t batch = c->last_batch;
  const size_t total = c->h_scan_begin[batch];
  if (hold(buf, 4 * total + words_per_scan * (size_t)batch, exact) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the downsampled surface clouds");
  }
  LFX_TRY(f.pin(c, pinned, at, with_info));
  f.down = buf.p;
  f.down_count = reinterpret_cast<uint32_t *>(f.down + 4 * total);
  f.down_status = f.down_count + batch;
  void * d_lengths = nullptr;
  LFX_HIP(c, hipHostGetDevicePointer(&d_lengths, f.lengths, 0));
  LFX_TRY(voxel_downsample(c, reinterpret_cast<const float *>(c->surf_pts.p), c->scan_begin.p, c->scan_info.p + lfx::kInfoSurface, 4, batch,
    total, leaf, f.down, f.down_count, f.down_status, st, true, c->scan_info.p + lfx::kInfoEdge, static_cast<uint32_t *>(d_lengths)));
  return with_info ? f.read_info(c, st) : LFX_OK;
}

// One scan's clouds as five device words that the clouds' begin and count arguments point at (lfx_localize_host,
// lfx_odometry_update, the loop closer's query); an owner keeps kScanWords of them
enum : uint32_t {kScanZero, kScanEdgeCount, kScanSurfaceCount, kScanDownCount, kScanDownStatus, kScanSent, kScanWords = 8};
// The words written into h_words (pinned; the caller has waited for what read it last) and queued for d_words, the surface
// cloud downsampled into d_down where there is one, and both clouds as align_clouds addresses them: sized by their own
// lengths (a bound on the downsampled one, whose count the kernels read on the device), rows from row_begin.  No wait.
inline int scan_front(lfx_ctx * c, uint32_t * h_words, uint32_t * d_words, const float * d_edge, uint32_t n_edge, const float * d_surface,
  uint32_t n_surface, float leaf, float * d_down, const uint32_t * row_begin, hipStream_t st, CloudSpan & edge, CloudSpan & down)
{
  h_words[kScanZero] = 0u; h_words[kScanEdgeCount] = n_edge; h_words[kScanSurfaceCount] = n_surface; h_words[kScanDownCount] = 0u; h_words[kScanDownStatus] = 0u;
  LFX_HIP(c, hipMemcpyAsync(d_words, h_words, sizeof(uint32_t) * kScanSent, hipMemcpyHostToDevice, st));
  if (n_surface) {
    LFX_TRY(voxel_downsample(c, d_surface, d_words + kScanZero, d_words + kScanSurfaceCount, 1, 1, n_surface, leaf, d_down,
      d_words + kScanDownCount, d_words + kScanDownStatus, st, true, d_words + kScanEdgeCount, nullptr));
  }
  edge = CloudSpan{d_edge, d_words + kScanZero, d_words + kScanEdgeCount, 1, n_edge, n_edge, row_begin};
  down = CloudSpan{d_down, d_words + kScanZero, d_words + kScanDownCount, 1, n_surface, n_surface, row_begin};
  return LFX_OK;
}

// the identity pose, [R | t] 3 x 4 row-major
constexpr double kIdentityPose[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

// the alignment settings the odometry's and the rolling map's configs share (leaf_name: what the config calls the scans' leaf)
inline int check_align_config(lfx_ctx * c, uint32_t n_neighbors, int max_iter, float leaf, const char * leaf_name, float edge_cell,
  float surface_cell, const double initial_pose[12])
{
  if (n_neighbors < 3 || n_neighbors > 16) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "n_neighbors must be in [3, 16]");}
  if (max_iter < 1) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "max_iter must be >= 1");}
  if (!(leaf > 0.f) || !std::isfinite(leaf)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, std::string(leaf_name) + " must be > 0");}
  if (!(edge_cell >= 0.f) || !std::isfinite(edge_cell) || !(surface_cell >= 0.f) || !std::isfinite(surface_cell)) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "edge_cell / surface_cell must be >= 0 (0: no grid)");
  }
  if (!finite_all(initial_pose, 12)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "initial_pose must be finite");}
  return LFX_OK;
}

// destroy_on for an owner of maps (emap, smap): they go after the object, whose destructor waits for its tail
template<typename T>
void destroy_with_maps(T * o)
{
  if (!o) {return;}
  lfx_map * const emap = o->emap, * const smap = o->smap;
  destroy_on(o);
  lfx_map_destroy(emap);
  lfx_map_destroy(smap);
}

// the savers' file of a kind (dirname/edge.pcd, dirname/surface.pcd); a host cloud written as PCD, or the writer's message
inline std::string kind_path(const char * dirname, int kind)
{
  const std::string dir(dirname);
  return dir + ((!dir.empty() && dir.back() == '/') ? "" : "/") + (kind ? "surface.pcd" : "edge.pcd");
}
inline int write_pcd(lfx_ctx * c, const std::string & path, const float * points, uint64_t n)
{
  char msg[512];
  const int rc = lfx_pcd_write(path.c_str(), points, n, msg, sizeof(msg));
  return rc != LFX_OK ? fail(c, rc, msg) : LFX_OK;
}

}  // namespace lfx_host
