// lfx_deskew.hip -- lfx_deskew_batch, lfx_deskew_batch_trajectory: the sensor's motion during a sweep taken out of the last
// device batch's feature clouds (include/lfx.h, the de-skew section; lfx_kernels_deskew.hpp).  The per-scan constants (per
// segment, along a trajectory) are worked out here, on the host, by the pose arithmetic of lfx_pose.cpp, and travel as one
// table of doubles per call (lfx_deskew_rows.hpp).  Both calls share their checks, the ring of slots the tables go out
// through and the launch; each writes its own rows.
#include "lfx_internal.hpp"
#include "lfx_kernels_deskew.hpp"

using namespace lfx_host;

namespace
{
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

// What both calls refuse about the batch, the range of scans, the outputs and `time`, and the source of the times.
// `motions`: the sweeps or the trajectories, named by `required`; a call without a `to` passes a valid one.
int check_call(lfx_ctx * c, const lfx_time_field * time, const void * motions, const char * required, uint32_t first, uint32_t n, int to,
  const float4 * edge_out, const float4 * surf_out, int & src)
{
  if (!time || !motions) {return fail(c, LFX_ERR_INVALID_ARGUMENT, required);}
  if (c->last_batch == 0) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "no batch has been extracted yet");}
  if (n == 0 || first >= c->last_batch || n > c->last_batch - first) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "scans outside the last batch");}
  if (to != LFX_DESKEW_TO_START && to != LFX_DESKEW_TO_END) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "to must be LFX_DESKEW_TO_START or LFX_DESKEW_TO_END");}
  if (!edge_out || !surf_out) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "both outputs, or neither (in place)");}
  return time_source(c, time, src);
}

// The ring's next slot with room for `doubles` on both sides, the kernel that read it last (kDeskewSlots calls ago, on
// whichever stream: long done) waited for.  Without the memory: LFX_ERR_OUT_OF_MEMORY, the runtime's word for it as the
// error text, for the caller to put its own in front of.  A failure leaves the slot valid, with what memory it had or none,
// and the ring where it was.
int take_slot(lfx_ctx * c, size_t doubles, lfx_ctx::DeskewSlot *& slot)
{
  LFX_HIP(c, hipSetDevice(c->device));
  slot = &c->deskew_slots[c->deskew_next];
  hipError_t e;
  const int rs = slot->take(c, doubles, e);
  if (rs != LFX_OK) {return rs;}
  if (e != hipSuccess) {return fail(c, LFX_ERR_OUT_OF_MEMORY, hipGetErrorString(e));}
  c->deskew_next = (c->deskew_next + 1u) % lfx_ctx::kDeskewSlots;
  return LFX_OK;
}

lfx::DeskewRecords records_of(const lfx_ctx * c, const lfx_time_field * time, const double * table, uint32_t first, float4 * edge_out,
  float4 * surf_out)
{
  lfx::DeskewRecords r{};
  r.scan_begin = c->scan_begin.p; r.scan_info = c->scan_info.p; r.table = table;
  r.edge_in = c->edge_pts.p; r.surf_in = c->surf_pts.p; r.edge_idx = c->edge_idx.p; r.surf_idx = c->surf_idx.p;
  r.edge_out = edge_out; r.surf_out = surf_out;
  r.pts = static_cast<const uint8_t *>(c->last_points);
  r.step = c->layout.step; r.off = time->offset; r.be = time->big_endian ? 1u : 0u;
  r.first = first;
  return r;
}

// a kernel's four forms, by the source of the times
template<typename Args>
using Forms = void (*[4])(Args);
static_assert(lfx::kDskFromIndex == 0 && lfx::kDskF32 == 1 && lfx::kDskF64 == 2 && lfx::kDskU32 == 3, "the order of a kernel's forms");
const Forms<lfx::DeskewArgs> kConstantForms = {lfx::deskew_kernel<0>, lfx::deskew_kernel<1>, lfx::deskew_kernel<2>, lfx::deskew_kernel<3>};
const Forms<lfx::TrajectoryArgs> kTrajectoryForms = {lfx::deskew_trajectory_kernel<0>, lfx::deskew_trajectory_kernel<1>,
  lfx::deskew_trajectory_kernel<2>, lfx::deskew_trajectory_kernel<3>};

// The slot's pinned block out to its device table, the kernel over n scans behind it, the slot's event behind the kernel:
// the event guards the device table as well as the pinned block.
template<typename Args>
int launch(lfx_ctx * c, const Forms<Args> & forms, int src, uint32_t n, const Args & a, lfx_ctx::DeskewSlot & slot, size_t doubles, hipStream_t st)
{
  LFX_HIP(c, hipMemcpyAsync(slot.d.p, slot.h.p, sizeof(double) * doubles, hipMemcpyHostToDevice, st));
  // (a scan of 64 x 1800 has about 14 k feature records: by_scan_grid's 8 workgroups walk them in 7 steps; a few scans get more)
  hipLaunchKernelGGL(forms[src], by_scan_grid(n), dim3(lfx::kDeskewThreads), 0, st, a);
  LFX_HIP(c, hipGetLastError());
  return slot.used.done(c, st);
}
}  // namespace

namespace lfx_host
{

// Scans first .. first + n - 1 of the last batch by sweeps[0 .. n - 1], into edge_out / surf_out (the context's own clouds:
// in place).  Everything lfx_deskew_batch refuses is refused here, before anything is queued.
int deskew_scans(lfx_ctx * c, const lfx_time_field * time, const lfx_sweep * sweeps, uint32_t first, uint32_t n, int to,
  float4 * edge_out, float4 * surf_out, hipStream_t st)
{
  int src;
  const int rt = check_call(c, time, sweeps, "time and sweeps are required", first, n, to, edge_out, surf_out, src);
  if (rt != LFX_OK) {return rt;}
  for (uint32_t s = 0; s < n; s++) {
    if (!lfx::finite_run(sweeps[s].motion, 12)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "sweeps[" + std::to_string(s) + "].motion is not finite");}
    if (src != lfx::kDskFromIndex) {
      if (!std::isfinite(sweeps[s].t0) || !std::isfinite(sweeps[s].t1)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "sweeps[" + std::to_string(s) + "]: t0 / t1 not finite");}
      if (sweeps[s].t1 == sweeps[s].t0) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "sweeps[" + std::to_string(s) + "]: t1 == t0");}
    }
  }
  const size_t doubles = (size_t)n * lfx::kDskStride;
  lfx_ctx::DeskewSlot * slot;
  const int rs = take_slot(c, doubles, slot);
  if (rs != LFX_OK) {return rs == LFX_ERR_OUT_OF_MEMORY ? fail(c, rs, "cannot set up the de-skew table: " + c->err) : rs;}
  for (uint32_t s = 0; s < n; s++) {
    const lfx_sweep & sw = sweeps[s];
    double * T = reinterpret_cast<double *>(slot->h.p) + (size_t)s * lfx::kDskStride, w[3], theta;
    lfx_motion_twist(sw.motion, w, &theta);
    lfx::write_twist(T, w, theta);
    for (int a = 0; a < 3; a++) {
      T[lfx::kDskV + a] = sw.motion[4 * a + 3];
      for (int j = 0; j < 3; j++) {T[lfx::kDskR + 3 * a + j] = sw.motion[4 * a + j];}
    }
    T[lfx::kDskT0] = src == lfx::kDskFromIndex ? 0.0 : sw.t0;
    T[lfx::kDskInvDt] = src == lfx::kDskFromIndex ? 1.0 : 1.0 / (sw.t1 - sw.t0);
    T[lfx::kDskScale] = src == lfx::kDskFromIndex ? 1.0 : time->scale;
    T[lfx::kDskScale + 1] = T[lfx::kDskScale + 2] = 0.0;       // (the row's spare doubles)
  }
  const lfx::DeskewArgs a{records_of(c, time, slot->d.p, first, edge_out, surf_out), to == LFX_DESKEW_TO_END ? 1u : 0u};
  return launch(c, kConstantForms, src, n, a, *slot, doubles, st);
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
    if (!lfx::ascending_times(tr.times, tr.n_knots) || !lfx::finite_run(tr.poses, 12 * (size_t)tr.n_knots) || !std::isfinite(tr.t_ref)) {
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
  int src;
  const int rt = check_call(c, time, trajectories, "time and trajectories are required", first, n, LFX_DESKEW_TO_START, edge_out, surf_out, src);
  if (rt != LFX_OK) {return rt;}
  const int rk = check_trajectories(c, trajectories, n);
  if (rk != LFX_OK) {return rk;}
  size_t segments = 0;
  for (uint32_t s = 0; s < n; s++) {segments += trajectories[s].n_knots - 1u;}
  // this call's block: the rows of every scan's segments, then where each scan's rows begin
  const size_t rows = segments * lfx::kTrjStride, doubles = rows + (n + 2u) / 2u;
  lfx_ctx::DeskewSlot * slot;
  const int rs = take_slot(c, doubles, slot);
  if (rs != LFX_OK) {return rs == LFX_ERR_OUT_OF_MEMORY ? fail(c, rs, "cannot set up the trajectory table") : rs;}
  double * h = reinterpret_cast<double *>(slot->h.p);
  uint32_t * begin = reinterpret_cast<uint32_t *>(h + rows);
  uint32_t at = 0;
  for (uint32_t s = 0; s < n; s++) {
    begin[s] = at;
    if (lfx_trajectory_segments(trajectories + s, h + (size_t)at * lfx::kTrjStride) != LFX_OK) {
      return fail(c, LFX_ERR_INVALID_ARGUMENT, "trajectories[" + std::to_string(s) + "] is refused by lfx_trajectory_segments");
    }
    at += trajectories[s].n_knots - 1u;
  }
  begin[n] = at;
  const lfx::TrajectoryArgs a{reinterpret_cast<const uint32_t *>(slot->d.p + rows), records_of(c, time, slot->d.p, first, edge_out, surf_out),
    src == lfx::kDskFromIndex ? 1.0 : time->scale};
  return launch(c, kTrajectoryForms, src, n, a, *slot, doubles, st);
}

}  // namespace lfx_host

namespace
{
// What both batch calls do around `scans(edge_out, surf_out)`, their de-skew of the whole batch: the checks of the batch and
// the outputs ahead of it, the in-place mark behind it.
template<typename Scans>
int deskew_batch(lfx_ctx * c, uint32_t n_scans, float * d_edge_out, float * d_surface_out, Scans scans)
{
  if (!c) {return LFX_ERR_INVALID_ARGUMENT;}
  const int rb = check_last_batch(c, n_scans);
  if (rb != LFX_OK) {return rb;}
  if ((d_edge_out == nullptr) != (d_surface_out == nullptr)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "both outputs, or neither (in place)");}
  if (c->deskewed_in_place) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the last batch has already been de-skewed in place");}
  if (d_edge_out && (d_edge_out == reinterpret_cast<float *>(c->edge_pts.p) || d_surface_out == reinterpret_cast<float *>(c->surf_pts.p) ||
    d_edge_out == reinterpret_cast<float *>(c->surf_pts.p) || d_surface_out == reinterpret_cast<float *>(c->edge_pts.p)))
  {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "the outputs are the context's own clouds: pass NULL for both to de-skew in place");
  }
  const bool in_place = d_edge_out == nullptr;
  const int rc = scans(in_place ? c->edge_pts.p : reinterpret_cast<float4 *>(d_edge_out), in_place ? c->surf_pts.p : reinterpret_cast<float4 *>(d_surface_out));
  if (rc == LFX_OK && in_place) {c->deskewed_in_place = true;}
  return rc;
}
}  // namespace

extern "C" int lfx_deskew_batch_trajectory(lfx_ctx * c, const lfx_time_field * time, const lfx_trajectory * trajectories, uint32_t n_scans,
  float * d_edge_out, float * d_surface_out, void * stream)
{
  return deskew_batch(c, n_scans, d_edge_out, d_surface_out, [&](float4 * edge, float4 * surf) {
             return deskew_scans_trajectory(c, time, trajectories, 0, n_scans, edge, surf, static_cast<hipStream_t>(stream));
           });
}

extern "C" int lfx_deskew_batch(lfx_ctx * c, const lfx_time_field * time, const lfx_sweep * sweeps, uint32_t n_scans, int to,
  float * d_edge_out, float * d_surface_out, void * stream)
{
  return deskew_batch(c, n_scans, d_edge_out, d_surface_out, [&](float4 * edge, float4 * surf) {
             return deskew_scans(c, time, sweeps, 0, n_scans, to, edge, surf, static_cast<hipStream_t>(stream));
           });
}
