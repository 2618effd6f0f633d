// lfx_deskew.hip -- lfx_deskew_batch, lfx_deskew_batch_trajectory: the sensor's motion during a sweep taken out of the last
// device batch's feature clouds (include/lfx.h, the de-skew section; lfx_kernels_deskew.hpp).  The per-scan constants (per
// segment, along a trajectory) are worked out here, on the host, by the helpers of lfx_pcd.cpp and travel as one table of
// doubles per call.
#include "lfx_internal.hpp"
#include "lfx_kernels_deskew.hpp"

using namespace lfx_host;

namespace
{
bool finite_all(const double * v, int n)
{
  for (int i = 0; i < n; i++) {
    if (!std::isfinite(v[i])) {return false;}
  }
  return true;
}

// where a record's firing time comes from: the kernels' template parameter, or what lfx_deskew_batch refuses about `time`
int time_source(lfx_ctx * c, const lfx_time_field * time, int & src)
{
  src = lfx::kDskFromIndex;
  if (time->source == LFX_TIME_FROM_FIELD) {
    uint32_t size = 4;
    switch (time->datatype) {
      case LFX_FIELD_FLOAT32: src = lfx::kDskF32; break;
      case LFX_FIELD_FLOAT64: src = lfx::kDskF64; size = 8; break;
      case LFX_FIELD_UINT32: src = lfx::kDskU32; break;
      default: return fail(c, LFX_ERR_INVALID_ARGUMENT, "the time field must be FLOAT32, FLOAT64 or UINT32");
    }
    if ((uint64_t)time->offset + size > c->layout.step) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the time field lies past the context's point_step");}
    if (!std::isfinite(time->scale)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the time field's scale must be finite");}
    if (!c->last_points) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the last batch's input points are not known");}
  } else if (time->source != LFX_TIME_FROM_INDEX) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "time->source must be LFX_TIME_FROM_INDEX or LFX_TIME_FROM_FIELD");
  }
  return LFX_OK;
}

template<int SRC>
void launch(dim3 grid, hipStream_t st, const lfx::DeskewArgs & a)
{
  hipLaunchKernelGGL(lfx::deskew_kernel<SRC>, grid, dim3(lfx::kDeskewThreads), 0, st, a);
}

template<int SRC>
void launch_trajectory(dim3 grid, hipStream_t st, const lfx::TrajectoryArgs & a)
{
  hipLaunchKernelGGL(lfx::deskew_trajectory_kernel<SRC>, grid, dim3(lfx::kDeskewThreads), 0, st, a);
}
}  // namespace

namespace lfx_host
{

// Scans first .. first + n - 1 of the last batch by sweeps[0 .. n - 1], into edge_out / surf_out (the context's own clouds:
// in place).  Everything lfx_deskew_batch refuses is refused here, before anything is queued.
int deskew_scans(lfx_ctx * c, const lfx_time_field * time, const lfx_sweep * sweeps, uint32_t first, uint32_t n, int to,
  float4 * edge_out, float4 * surf_out, hipStream_t st)
{
  if (!time || !sweeps) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "time and sweeps are required");}
  if (c->last_batch == 0) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "no batch has been extracted yet");}
  if (n == 0 || first >= c->last_batch || n > c->last_batch - first) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "scans outside the last batch");}
  if (to != LFX_DESKEW_TO_START && to != LFX_DESKEW_TO_END) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "to must be LFX_DESKEW_TO_START or LFX_DESKEW_TO_END");}
  if (!edge_out || !surf_out) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "both outputs, or neither (in place)");}
  int src;
  const int rt = time_source(c, time, src);
  if (rt != LFX_OK) {return rt;}
  for (uint32_t s = 0; s < n; s++) {
    if (!finite_all(sweeps[s].motion, 12)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "sweeps[" + std::to_string(s) + "].motion is not finite");}
    if (src != lfx::kDskFromIndex) {
      if (!std::isfinite(sweeps[s].t0) || !std::isfinite(sweeps[s].t1)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "sweeps[" + std::to_string(s) + "]: t0 / t1 not finite");}
      if (sweeps[s].t1 == sweeps[s].t0) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "sweeps[" + std::to_string(s) + "]: t1 == t0");}
    }
  }
  LFX_HIP(c, hipSetDevice(c->device));
  // the table's blocks: pinned and device, kDeskewSlots of max_batch rows each
  const size_t rows = std::max(c->max_batch, 1u), block = rows * lfx::kDskStride;
  if (!c->d_deskew.p) {
    // all of it or none: a call that fails here leaves nothing half made for the next one to trip over
    hipError_t e = c->h_deskew.reserve(sizeof(double) * block * lfx_ctx::kDeskewSlots);
    for (auto & ev : c->deskew_copied) {
      if (e == hipSuccess && !ev) {e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);}
    }
    if (e == hipSuccess) {e = c->d_deskew.alloc(block * lfx_ctx::kDeskewSlots);}
    if (e != hipSuccess) {
      for (auto & ev : c->deskew_copied) {
        if (ev) {(void)hipEventDestroy(ev); ev = nullptr;}
      }
      return fail(c, LFX_ERR_OUT_OF_MEMORY, std::string("cannot set up the de-skew table: ") + hipGetErrorString(e));
    }
  }
  const uint32_t slot = c->deskew_next;
  c->deskew_next = (slot + 1u) % lfx_ctx::kDeskewSlots;
  LFX_HIP(c, hipEventSynchronize(c->deskew_copied[slot]));     // (the kernel queued eight calls ago, on whichever stream: long done)
  double * h = reinterpret_cast<double *>(c->h_deskew.p) + slot * block, * d = c->d_deskew.p + slot * block;
  for (uint32_t s = 0; s < n; s++) {
    const lfx_sweep & sw = sweeps[s];
    double * T = h + (size_t)s * lfx::kDskStride, w[3], theta;
    lfx_motion_twist(sw.motion, w, &theta);
    for (int a = 0; a < 3; a++) {
      T[lfx::kDskK + a] = theta < 1e-8 ? 0.0 : w[a] / theta;
      T[lfx::kDskW + a] = w[a];
      T[lfx::kDskV + a] = sw.motion[4 * a + 3];
      for (int j = 0; j < 3; j++) {T[lfx::kDskR + 3 * a + j] = sw.motion[4 * a + j];}
    }
    T[lfx::kDskTheta] = theta;
    T[lfx::kDskT0] = src == lfx::kDskFromIndex ? 0.0 : sw.t0;
    T[lfx::kDskInvDt] = src == lfx::kDskFromIndex ? 1.0 : 1.0 / (sw.t1 - sw.t0);
    T[lfx::kDskScale] = src == lfx::kDskFromIndex ? 1.0 : time->scale;
    T[22] = T[23] = 0.0;
  }
  LFX_HIP(c, hipMemcpyAsync(d, h, sizeof(double) * n * lfx::kDskStride, hipMemcpyHostToDevice, st));
  lfx::DeskewArgs a{};
  a.scan_begin = c->scan_begin.p; a.scan_info = c->scan_info.p; a.table = d;
  a.edge_in = c->edge_pts.p; a.surf_in = c->surf_pts.p; a.edge_idx = c->edge_idx.p; a.surf_idx = c->surf_idx.p;
  a.edge_out = edge_out; a.surf_out = surf_out;
  a.pts = static_cast<const uint8_t *>(c->last_points);
  a.step = c->layout.step; a.off = time->offset; a.be = time->big_endian ? 1u : 0u;
  a.first = first; a.to_end = to == LFX_DESKEW_TO_END ? 1u : 0u;
  // (a scan of 64 x 1800 has about 14 k feature records: 8 workgroups walk them in 7 steps; a few scans get more)
  const dim3 grid(n >= 32u ? 8u : 32u, n);
  switch (src) {
    case lfx::kDskF32: launch<lfx::kDskF32>(grid, st, a); break;
    case lfx::kDskF64: launch<lfx::kDskF64>(grid, st, a); break;
    case lfx::kDskU32: launch<lfx::kDskU32>(grid, st, a); break;
    default: launch<lfx::kDskFromIndex>(grid, st, a); break;
  }
  LFX_HIP(c, hipGetLastError());
  // behind the kernel, not the copy: the event guards the slot's device table as well as its pinned block
  LFX_HIP(c, hipEventRecord(c->deskew_copied[slot], st));
  return LFX_OK;
}

// What lfx_deskew_batch_trajectory refuses about trajectories[0 .. n - 1] (what lfx_trajectory_segments refuses about each),
// with the scan named.  Nothing is touched.
int check_trajectories(lfx_ctx * c, const lfx_trajectory * trajectories, uint32_t n)
{
  for (uint32_t s = 0; s < n; s++) {
    const lfx_trajectory & tr = trajectories[s];
    if (tr.n_knots < 2u || tr.n_knots > LFX_MAX_TRAJECTORY_KNOTS || !tr.times || !tr.poses) {
      return fail(c, LFX_ERR_INVALID_ARGUMENT, "trajectories[" + std::to_string(s) + "]: 2 .. 64 knots with times and poses");
    }
    bool ok = finite_all(tr.times, (int)tr.n_knots) && finite_all(tr.poses, 12 * (int)tr.n_knots) && std::isfinite(tr.t_ref);
    for (uint32_t k = 1; ok && k < tr.n_knots; k++) {ok = tr.times[k] > tr.times[k - 1];}
    if (!ok) {
      return fail(c, LFX_ERR_INVALID_ARGUMENT, "trajectories[" + std::to_string(s) +
               "]: times must be finite and strictly ascending, poses and t_ref finite");
    }
  }
  return LFX_OK;
}

// Scans first .. first + n - 1 of the last batch along trajectories[0 .. n - 1].  Everything lfx_deskew_batch_trajectory
// refuses is refused here, before anything is queued.
int deskew_scans_trajectory(lfx_ctx * c, const lfx_time_field * time, const lfx_trajectory * trajectories, uint32_t first, uint32_t n,
  float4 * edge_out, float4 * surf_out, hipStream_t st)
{
  if (!time || !trajectories) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "time and trajectories are required");}
  if (c->last_batch == 0) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "no batch has been extracted yet");}
  if (n == 0 || first >= c->last_batch || n > c->last_batch - first) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "scans outside the last batch");}
  if (!edge_out || !surf_out) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "both outputs, or neither (in place)");}
  int src;
  const int rt = time_source(c, time, src);
  if (rt != LFX_OK) {return rt;}
  const int rk = check_trajectories(c, trajectories, n);
  if (rk != LFX_OK) {return rk;}
  size_t segments = 0;
  for (uint32_t s = 0; s < n; s++) {segments += trajectories[s].n_knots - 1u;}
  LFX_HIP(c, hipSetDevice(c->device));
  // this call's block: the rows of every scan's segments, then where each scan's rows begin
  lfx_ctx::TrajectorySlot & slot = c->trajectory_slots[c->trajectory_next];
  const size_t doubles = segments * lfx::kTrjStride + (n + 2u) / 2u;
  if (!slot.used) {LFX_HIP(c, hipEventCreateWithFlags(&slot.used, hipEventDisableTiming));}
  LFX_HIP(c, hipEventSynchronize(slot.used));                  // (the kernel queued eight calls ago, on whichever stream: long done)
  if (slot.h.reserve(sizeof(double) * doubles) != hipSuccess || hold(slot.d, doubles) != hipSuccess) {
    return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot set up the trajectory table");
  }
  double * h = reinterpret_cast<double *>(slot.h.p);
  uint32_t * begin = reinterpret_cast<uint32_t *>(h + segments * lfx::kTrjStride);
  uint32_t at = 0;
  for (uint32_t s = 0; s < n; s++) {
    begin[s] = at;
    if (lfx_trajectory_segments(trajectories + s, h + (size_t)at * lfx::kTrjStride) != LFX_OK) {
      return fail(c, LFX_ERR_INVALID_ARGUMENT, "trajectories[" + std::to_string(s) + "] is refused by lfx_trajectory_segments");
    }
    at += trajectories[s].n_knots - 1u;
  }
  begin[n] = at;
  c->trajectory_next = (c->trajectory_next + 1u) % lfx_ctx::kDeskewSlots;
  LFX_HIP(c, hipMemcpyAsync(slot.d.p, h, sizeof(double) * doubles, hipMemcpyHostToDevice, st));
  lfx::TrajectoryArgs a{};
  a.scan_begin = c->scan_begin.p; a.scan_info = c->scan_info.p;
  a.table = slot.d.p; a.seg_begin = reinterpret_cast<const uint32_t *>(slot.d.p + segments * lfx::kTrjStride);
  a.edge_in = c->edge_pts.p; a.surf_in = c->surf_pts.p; a.edge_idx = c->edge_idx.p; a.surf_idx = c->surf_idx.p;
  a.edge_out = edge_out; a.surf_out = surf_out;
  a.pts = static_cast<const uint8_t *>(c->last_points);
  a.step = c->layout.step; a.off = time->offset; a.be = time->big_endian ? 1u : 0u;
  a.first = first; a.scale = src == lfx::kDskFromIndex ? 1.0 : time->scale;
  const dim3 grid(n >= 32u ? 8u : 32u, n);                    // (as deskew_scans)
  switch (src) {
    case lfx::kDskF32: launch_trajectory<lfx::kDskF32>(grid, st, a); break;
    case lfx::kDskF64: launch_trajectory<lfx::kDskF64>(grid, st, a); break;
    case lfx::kDskU32: launch_trajectory<lfx::kDskU32>(grid, st, a); break;
    default: launch_trajectory<lfx::kDskFromIndex>(grid, st, a); break;
  }
  LFX_HIP(c, hipGetLastError());
  LFX_HIP(c, hipEventRecord(slot.used, st));                   // behind the kernel: the event guards the device table too
  return LFX_OK;
}

}  // namespace lfx_host

namespace
{
// what both batch de-skews check about the batch and the outputs
int check_batch_outputs(lfx_ctx * c, uint32_t n_scans, const float * d_edge_out, const float * d_surface_out)
{
  if (c->last_batch == 0) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "no batch has been extracted yet");}
  if (n_scans != c->last_batch) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "n_scans (" + std::to_string(n_scans) + ") is not the number of scans of the last batch (" +
             std::to_string(c->last_batch) + ")");
  }
  if ((d_edge_out == nullptr) != (d_surface_out == nullptr)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "both outputs, or neither (in place)");}
  if (c->deskewed_in_place) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the last batch has already been de-skewed in place");}
  if (d_edge_out && (d_edge_out == reinterpret_cast<float *>(c->edge_pts.p) || d_surface_out == reinterpret_cast<float *>(c->surf_pts.p) ||
    d_edge_out == reinterpret_cast<float *>(c->surf_pts.p) || d_surface_out == reinterpret_cast<float *>(c->edge_pts.p)))
  {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "the outputs are the context's own clouds: pass NULL for both to de-skew in place");
  }
  return LFX_OK;
}
}  // namespace

extern "C" int lfx_deskew_batch_trajectory(lfx_ctx * c, const lfx_time_field * time, const lfx_trajectory * trajectories, uint32_t n_scans,
  float * d_edge_out, float * d_surface_out, void * stream)
{
  if (!c) {return LFX_ERR_INVALID_ARGUMENT;}
  const int rb = check_batch_outputs(c, n_scans, d_edge_out, d_surface_out);
  if (rb != LFX_OK) {return rb;}
  const bool in_place = d_edge_out == nullptr;
  const int rc = deskew_scans_trajectory(c, time, trajectories, 0, n_scans, in_place ? c->edge_pts.p : reinterpret_cast<float4 *>(d_edge_out),
    in_place ? c->surf_pts.p : reinterpret_cast<float4 *>(d_surface_out), static_cast<hipStream_t>(stream));
  if (rc == LFX_OK && in_place) {c->deskewed_in_place = true;}
  return rc;
}

extern "C" int lfx_deskew_batch(lfx_ctx * c, const lfx_time_field * time, const lfx_sweep * sweeps, uint32_t n_scans, int to,
  float * d_edge_out, float * d_surface_out, void * stream)
{
  if (!c) {return LFX_ERR_INVALID_ARGUMENT;}
  const int rb = check_batch_outputs(c, n_scans, d_edge_out, d_surface_out);
  if (rb != LFX_OK) {return rb;}
  const bool in_place = d_edge_out == nullptr;
  const int rc = deskew_scans(c, time, sweeps, 0, n_scans, to, in_place ? c->edge_pts.p : reinterpret_cast<float4 *>(d_edge_out),
    in_place ? c->surf_pts.p : reinterpret_cast<float4 *>(d_surface_out), static_cast<hipStream_t>(stream));
  if (rc == LFX_OK && in_place) {c->deskewed_in_place = true;}
  return rc;
}
