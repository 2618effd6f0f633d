// lfx_localize.hip -- the consumer of the two clouds: map index, residual rows, the optimizer, Localizer::Update
// (lfx_kernels_localize.hpp).
#include "lfx_internal.hpp"
#include "lfx_kernels_localize.hpp"
#include "lfx_kernels_report.hpp"

using namespace lfx_host;

// ---------------------------------------------------------------------------- the map (KDTreeEigen's place)
struct lfx_map
{
  int device = 0;
  DevBuf<float4> pts;                    // the map's own copy of the points (sorted by cell when there is a grid)
  DevBuf<uint32_t> start;                // first point of every cell, + 1
  lfx::MapIndex index{};
  float cell = 0.f;
  DevBuf<uint32_t> cell_count, partial;  // map_rebuild only: the build's scratch, kept between rebuilds
};

namespace
{
// the grid of a map over [lo, hi]: cubic cells of the asked size, grown until the grid has at most 2^25 cells
void grid_of(const double lo[3], const double hi[3], float cell_size, double & h, int dims[3])
{
  h = (double)cell_size;
  const double limit = 33554432.;
  for (;;) {
    double cells = 1.;
    for (int a = 0; a < 3; a++) {
      const double na = std::floor((hi[a] - lo[a]) / h) + 1.;
      dims[a] = na > 2147483647. ? 2147483647 : (int)na;
      cells *= na;
    }
    if (cells <= limit) {break;}
    h *= std::max(1.05, std::cbrt(cells / limit));
  }
}

// The index of map m over the n_points >= 1 records at src (m->pts holds that many): a grid of cells of cell_size over
// [lo, hi], the bounds of the points as map_bounds_kernel finds them -- points per cell, the cells' first points by an
// exclusive scan, the points into their cells -- or, cell_size 0, a copy of the points.  The cells' starts and the build's
// scratch are held as hold() holds them (`exact`: no larger than needed).  Nothing is waited for.
hipError_t build_index(lfx_map * m, const float4 * src, uint32_t n_points, float cell_size, const double lo[3], const double hi[3],
  DevBuf<uint32_t> & cell_count, DevBuf<uint32_t> & partial, bool exact, hipStream_t st)
{
  lfx::MapIndex & mi = m->index;
  mi.pts = m->pts.p; mi.start = nullptr; mi.n = n_points;
  mi.ox = mi.oy = mi.oz = 0.; mi.h = 0.; mi.inv_h = 0.; mi.nx = mi.ny = mi.nz = 1;
  if (cell_size == 0.f) {return hipMemcpyAsync(m->pts.p, src, sizeof(float4) * (size_t)n_points, hipMemcpyDeviceToDevice, st);}
  double h;
  int dims[3];
  grid_of(lo, hi, cell_size, h, dims);
  const size_t cells = (size_t)dims[0] * dims[1] * dims[2];
  const uint32_t n_blocks = (uint32_t)((cells + lfx::kScanItems - 1) / lfx::kScanItems);
  hipError_t e = hold(m->start, cells + 1, exact);
  if (e == hipSuccess) {e = hold(cell_count, cells, exact);}
  if (e == hipSuccess) {e = hold(partial, (size_t)n_blocks + 1, exact);}
  if (e == hipSuccess) {e = hipMemsetAsync(cell_count.p, 0, cells * sizeof(uint32_t), st);}
  if (e != hipSuccess) {return e;}
  mi.ox = lo[0]; mi.oy = lo[1]; mi.oz = lo[2]; mi.h = h; mi.inv_h = 1. / h; mi.nx = dims[0]; mi.ny = dims[1]; mi.nz = dims[2];
  m->cell = (float)h;
  const dim3 per_point((n_points + 255u) / 256u);
  hipLaunchKernelGGL(lfx::map_count_kernel, per_point, dim3(256), 0, st, mi, src, cell_count.p);
  hipLaunchKernelGGL(lfx::cell_block_sum_kernel, dim3(n_blocks), dim3(lfx::kScanThreads), 0, st, cell_count.p, cells, partial.p);
  hipLaunchKernelGGL(lfx::cell_partial_scan_kernel, dim3(1), dim3(lfx::kScanThreads), 0, st, partial.p, n_blocks);
  hipLaunchKernelGGL(lfx::cell_start_kernel, dim3(n_blocks), dim3(lfx::kScanThreads), 0, st, cell_count.p, cells, partial.p, m->start.p, n_points);
  hipLaunchKernelGGL(lfx::map_scatter_kernel, per_point, dim3(256), 0, st, mi, src, cell_count.p, m->start.p, m->pts.p);
  e = hipGetLastError();
  if (e == hipSuccess) {mi.start = m->start.p;}
  return e;
}

// Eigen::Quaterniond(Matrix3d) of a pose's rotation (the branch on the trace, then on the largest diagonal entry), on the
// host: what lfx_scan_to_map_residuals hands its kernels beside pose[12], and what the report pass of run_align is given
void map_pose_of(const double pose[12], lfx::MapPose & P)
{
  for (int i = 0; i < 12; i++) {P.m[i] = pose[i];}
  auto M = [&](int r, int col) {return pose[4 * r + col];};
  double q[3], w, t = M(0, 0) + M(1, 1) + M(2, 2);
  if (t > 0.) {
    t = std::sqrt(t + 1.0);
    w = 0.5 * t;
    t = 0.5 / t;
    q[0] = (M(2, 1) - M(1, 2)) * t; q[1] = (M(0, 2) - M(2, 0)) * t; q[2] = (M(1, 0) - M(0, 1)) * t;
  } else {
    int i = 0;
    if (M(1, 1) > M(0, 0)) {i = 1;}
    if (M(2, 2) > M(i, i)) {i = 2;}
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(M(i, i) - M(j, j) - M(k, k) + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    w = (M(k, j) - M(j, k)) * t;
    q[j] = (M(j, i) + M(i, j)) * t;
    q[k] = (M(k, i) + M(i, k)) * t;
  }
  P.qw = w; P.qx = q[0]; P.qy = q[1]; P.qz = q[2];
}

void launch_rows(bool surface, const lfx::RowsOfKind & R, const lfx::MapPose & P, uint32_t k, uint32_t n_clouds, uint32_t longest,
  const lfx::AlignState * states, hipStream_t st)
{
  const bool wave = R.mi.start != nullptr;            // a grid: one query per wave; no grid: one per thread, the map through LDS
  const dim3 grid(wave ? longest : (longest + 127u) / 128u, n_clouds), block(wave ? 64 : 128);
#define LFX_ROWS(S, M) hipLaunchKernelGGL((lfx::scan_to_map_kernel<S, M>), grid, block, 0, st, R.mi, P, k, R.pts, R.begin, R.count, \
    R.count_stride, R.residual, R.jacobian, states, R.row_begin)
  if (wave) {
    if (surface) {LFX_ROWS(true, lfx::kSearchGridWave);} else {LFX_ROWS(false, lfx::kSearchGridWave);}
  } else {
    if (surface) {LFX_ROWS(true, lfx::kSearchWholeMap);} else {LFX_ROWS(false, lfx::kSearchWholeMap);}
  }
#undef LFX_ROWS
}
}  // namespace

extern "C" {

int lfx_map_create(lfx_ctx * c, const float * d_points, uint32_t n_points, float cell_size, lfx_map ** out, void * stream)
{
  if (!c || !d_points || !out || n_points == 0) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!(cell_size >= 0.f) || !std::isfinite(cell_size)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "cell_size must be >= 0 (0: no grid)");}
  LFX_HIP(c, hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  lfx_map * m = new (std::nothrow) lfx_map();
  if (!m) {return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the map");}
  m->device = c->device;
  auto give_up = [&](int code, const char * why) {lfx_map_destroy(m); return fail(c, code, why);};
  if (m->pts.alloc(n_points) != hipSuccess) {return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the map's points");}
  const float4 * src = reinterpret_cast<const float4 *>(d_points);
  double lo[3] = {0., 0., 0.}, hi[3] = {0., 0., 0.};
  if (cell_size != 0.f) {                              // bounds of the map
    DevBuf<uint32_t> d_bounds;
    if (d_bounds.alloc(6) != hipSuccess) {return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the map's bounds");}
    const uint32_t init[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u};
    uint32_t got[6];
    hipError_t e = hipMemcpyAsync(d_bounds.p, init, sizeof(init), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
      const uint32_t blocks = std::min<uint32_t>((n_points + 255u) / 256u, 2048u);
      hipLaunchKernelGGL(lfx::map_bounds_kernel, dim3(blocks), dim3(256), 0, st, src, n_points, d_bounds.p);
      e = hipMemcpyAsync(got, d_bounds.p, sizeof(got), hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) {e = hipStreamSynchronize(st);}
    if (e != hipSuccess) {return give_up(LFX_ERR_HIP, hipGetErrorString(e));}
    for (int a = 0; a < 3; a++) {
      lo[a] = lfx::float_of_order(got[a]); hi[a] = lfx::float_of_order(got[3 + a]);
      if (!std::isfinite(lo[a]) || !std::isfinite(hi[a])) {return give_up(LFX_ERR_INVALID_ARGUMENT, "the map holds a point that is not finite");}
    }
  }
  DevBuf<uint32_t> cell_count, partial;                // the build's scratch, this call's own
  hipError_t e = build_index(m, src, n_points, cell_size, lo, hi, cell_count, partial, true, st);
  if (e == hipSuccess) {e = hipStreamSynchronize(st);}
  if (e == hipErrorOutOfMemory) {return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the map's cells");}
  if (e != hipSuccess) {return give_up(LFX_ERR_HIP, hipGetErrorString(e));}
  *out = m;
  return LFX_OK;
}

void lfx_map_destroy(lfx_map * m)
{
  if (!m) {return;}
  (void)hipSetDevice(m->device);
  delete m;
}

int lfx_map_create_host(lfx_ctx * c, const float * points, uint32_t n_points, float cell_size, lfx_map ** out, void * stream)
{
  if (!c || !points || !out || n_points == 0) {return LFX_ERR_INVALID_ARGUMENT;}
  LFX_HIP(c, hipSetDevice(c->device));
  DevBuf<float> staged;
  if (staged.alloc(4 * (size_t)n_points) != hipSuccess) {return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot stage the map's points");}
  hipError_t e = hipMemcpyAsync(staged.p, points, sizeof(float) * 4 * (size_t)n_points, hipMemcpyHostToDevice, static_cast<hipStream_t>(stream));
  if (e == hipSuccess) {e = hipStreamSynchronize(static_cast<hipStream_t>(stream));}
  if (e != hipSuccess) {return fail(c, LFX_ERR_HIP, hipGetErrorString(e));}
  return lfx_map_create(c, staged.p, n_points, cell_size, out, stream);
}

int lfx_map_info(const lfx_map * m, uint32_t * n_points, float * cell_size, int32_t dims[3])
{
  if (!m) {return LFX_ERR_INVALID_ARGUMENT;}
  if (n_points) {*n_points = m->index.n;}
  if (cell_size) {*cell_size = m->index.start ? m->cell : 0.f;}
  if (dims) {dims[0] = m->index.nx; dims[1] = m->index.ny; dims[2] = m->index.nz;}
  return LFX_OK;
}

int lfx_map_nearest(
  lfx_ctx * c, const lfx_map * m, const double * d_queries, uint32_t n_queries, uint32_t k, double * d_neighbours,
  double * d_squared_distances, uint32_t * d_indices, void * stream)
{
  if (!c || !m || !d_queries) {return LFX_ERR_INVALID_ARGUMENT;}
  if (k == 0 || k > (uint32_t)lfx::kNearestMax || m->index.n < k) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "k must be in [1, 16] and the map must hold that many points");
  }
  if (check_device(c, m->device, "the map") != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (n_queries == 0) {return LFX_OK;}
  LFX_HIP(c, hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (m->index.start) {
    hipLaunchKernelGGL(lfx::map_nearest_kernel<lfx::kSearchGridWave>, dim3(n_queries), dim3(64), 0, st, m->index, d_queries,
      n_queries, k, d_neighbours, d_squared_distances, d_indices);
  } else {
    hipLaunchKernelGGL(lfx::map_nearest_kernel<lfx::kSearchWholeMap>, dim3((n_queries + 127u) / 128u), dim3(128), 0, st, m->index,
      d_queries, n_queries, k, d_neighbours, d_squared_distances, d_indices);
  }
  LFX_HIP(c, hipGetLastError());
  return LFX_OK;
}

}  // extern "C"

namespace lfx_host
{
lfx_map * map_new(int device)
{
  lfx_map * m = new (std::nothrow) lfx_map();
  if (m) {m->device = device;}
  return m;
}

// The index of lfx_map_create over n_points records at d_points, rebuilt in place: the map keeps its buffers (grown by half
// again when they must grow), the bounds come from the caller ([lo, hi] of the points, as map_bounds_kernel would find
// them), nothing is waited for.  The same grid, the same cells, the same kernels as lfx_map_create; n_points >= 1.
int map_rebuild(lfx_ctx * c, lfx_map * m, const float * d_points, uint32_t n_points, float cell_size, const double lo[3],
  const double hi[3], hipStream_t st)
{
  LFX_HIP(c, hold(m->pts, n_points));
  LFX_HIP(c, build_index(m, reinterpret_cast<const float4 *>(d_points), n_points, cell_size, lo, hi, m->cell_count, m->partial, false, st));
  return LFX_OK;
}
}  // namespace lfx_host

// ---------------------------------------------------------------------------- scan-to-map residuals
extern "C" {

int lfx_scan_to_map_residuals(
  lfx_ctx * c, int kind, const lfx_map * map, const double pose[12], uint32_t n_neighbors,
  const float * d_points, const uint32_t * d_begin, const uint32_t * d_count, uint32_t count_stride, uint32_t n_clouds,
  uint32_t max_points_per_cloud, double * d_residual, double * d_jacobian, void * stream)
{
  if (!c || !map || !pose || !d_points || !d_begin || !d_count || !d_residual || !d_jacobian || n_clouds == 0 || count_stride == 0 ||
    (kind != LFX_RESIDUAL_EDGE && kind != LFX_RESIDUAL_SURFACE))
  {
    return LFX_ERR_INVALID_ARGUMENT;
  }
  if (n_neighbors == 0 || n_neighbors > (uint32_t)lfx::kNearestMax || map->index.n < n_neighbors || (kind == LFX_RESIDUAL_SURFACE && n_neighbors < 3)) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "n_neighbors must be in [1, 16] (>= 3 for planes) and the map must hold that many points");
  }
  if (check_device(c, map->device, "the map") != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (max_points_per_cloud == 0) {return LFX_OK;}
  LFX_HIP(c, hipSetDevice(c->device));
  lfx::MapPose P;
  map_pose_of(pose, P);
  const lfx::RowsOfKind R{map->index, reinterpret_cast<const float4 *>(d_points), d_begin, d_count, count_stride, d_residual, d_jacobian,
    nullptr, nullptr, nullptr};
  launch_rows(kind == LFX_RESIDUAL_SURFACE, R, P, n_neighbors, n_clouds, max_points_per_cloud, nullptr, static_cast<hipStream_t>(stream));
  LFX_HIP(c, hipGetLastError());
  return LFX_OK;
}

int lfx_edge_residuals(
  lfx_ctx * c, const lfx_map * map, const double pose[12], uint32_t n_neighbors, double * d_residual, double * d_jacobian,
  void * stream)
{
  if (!c) {return LFX_ERR_INVALID_ARGUMENT;}
  if (c->last_batch == 0) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "no batch has been extracted yet");}
  uint32_t longest = 0;
  for (uint32_t s = 0; s < c->last_batch; s++) {
    const uint32_t n = c->h_scan_begin[s + 1] - c->h_scan_begin[s];
    longest = n > longest ? n : longest;                 // a scan has no more edge points than points
  }
  return lfx_scan_to_map_residuals(c, LFX_RESIDUAL_EDGE, map, pose, n_neighbors, reinterpret_cast<const float *>(c->edge_pts.p),
           c->scan_begin.p, c->scan_info.p + lfx::kInfoEdge, 4, c->last_batch, longest, d_residual, d_jacobian, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------- the optimizer around the rows
namespace
{
struct AlignProblem                     // what Problem::Make reads
{
  // rows of dimension 3: the edge clouds against their map, or the point pairs X, Y (then `edge` holds begin, count, longest
  // and total alone); rows of dimension 1: the downsampled surface clouds against theirs
  const lfx_map * edge_map = nullptr, * surface_map = nullptr;
  CloudSpan edge, surface;
  const double * X = nullptr, * Y = nullptr;
  uint32_t n_neighbors = 0;
};

// The host's wait for records the kernels write into pinned memory: on the records themselves first (the thread that ends a
// scan sets its done word behind a system-scope fence; a blocking wait on the stream wakes 30-50 us late, a third of what a
// whole scan's alignment takes), then until the stream has drained what was queued behind them
template<typename AllDone>
hipError_t wait_for_records(AllDone all_done, hipStream_t st)
{
  hipError_t q = hipErrorNotReady;
  for (uint32_t spins = 0; q == hipErrorNotReady; spins++) {
    if (all_done() || (spins & 63u) == 63u) {q = hipStreamQuery(st);}
    if (spins > (1u << 24)) {q = hipStreamSynchronize(st);}         // (seconds: something else holds the stream)
  }
  return q;
}

int run_align(lfx_ctx * c, const AlignProblem & pr, uint32_t n_clouds, int max_iter, const double * initial_poses,
  lfx_align_result * results, hipStream_t st, lfx_align_report * reports = nullptr)
{
  static_assert(sizeof(lfx::AlignReport) == sizeof(lfx_align_report), "the device's record is lfx_align_report");
  static_assert(sizeof(lfx::AlignState) % 8 == 0, "AlignState is an array of doubles' worth");
  if (n_clouds > 65535u) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "at most 65535 scans per alignment call");}   // (a launch's y extent)
  const size_t state_d = sizeof(lfx::AlignState) / 8 * (size_t)n_clouds;
  const size_t total3 = pr.edge.total, total1 = pr.surface.total, rows = total3 + total1;
  const size_t partial_d = (size_t)n_clouds * lfx::kAlignSlices * lfx::kAlignTile;
  const size_t nbr_d = (size_t)lfx::kNearestMax / 2 * rows;                   // the searches' results: 16 words per row
  const size_t reach_d = rows;                                               // and how far each row's 16th neighbour was
  const bool report = reports != nullptr && pr.X == nullptr;
  const size_t sums_d = report ? sizeof(lfx::ReportSums) / 8 * (size_t)n_clouds : 0;
  const size_t need = state_d + 24 * total3 + 8 * total1 + rows + partial_d + nbr_d + reach_d + (n_clouds + 1) / 2 + 9 + sums_d;
  if (hold(c->align_scratch, need, true) != hipSuccess) {
    return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the rows of the scan-to-map alignment");
  }
  double * w = c->align_scratch.p;
  lfx::AlignState * states = reinterpret_cast<lfx::AlignState *>(w); w += state_d;
  double * r3 = w; w += 3 * total3;
  double * J3 = w; w += 21 * total3;
  double * r1 = w; w += total1;
  double * J1 = w; w += 7 * total1;
  double * d_weights = w; w += rows;
  double * d_partials = w; w += partial_d;
  uint32_t * nbr3 = reinterpret_cast<uint32_t *>(w), * nbr1 = nbr3 + (size_t)lfx::kNearestMax * total3; w += nbr_d;
  double * reach3 = w, * reach1 = w + total3; w += reach_d;
  uint32_t * d_tickets = reinterpret_cast<uint32_t *>(w); w += (n_clouds + 1) / 2;
  uint32_t * d_active = reinterpret_cast<uint32_t *>(w); w += 9;
  lfx::ReportSums * d_sums = reinterpret_cast<lfx::ReportSums *>(w);
  // Pinned host memory, read and written by the kernels themselves: [the caller's poses | a result record per scan].  No
  // copy is queued in either direction; the thread that ends a scan's iterations writes its record.
  const size_t pose_bytes = 96 * (size_t)n_clouds;
  // (with reports, behind those: [the report pass's poses | a report per scan | its done word])
  const size_t out_bytes = sizeof(lfx::AlignOut) * (size_t)n_clouds;
  const size_t report_bytes = report ? (sizeof(lfx::ReportPose) + sizeof(lfx::AlignReport) + 8) * (size_t)n_clouds : 0;
  LFX_HIP(c, c->h_align.reserve(pose_bytes + out_bytes + report_bytes));
  std::memcpy(c->h_align.p, initial_poses, pose_bytes);
  volatile lfx::AlignOut * out = reinterpret_cast<volatile lfx::AlignOut *>(c->h_align.p + pose_bytes);
  void * d_pinned = nullptr;
  LFX_HIP(c, hipHostGetDevicePointer(&d_pinned, c->h_align.p, 0));
  const double * d_initial = static_cast<const double *>(d_pinned);
  lfx::AlignOut * d_out = reinterpret_cast<lfx::AlignOut *>(static_cast<uint8_t *>(d_pinned) + pose_bytes);
  hipLaunchKernelGGL(lfx::align_begin_kernel, dim3((n_clouds + 63u) / 64u), dim3(64), 0, st, states, d_initial, n_clouds, d_active,
    d_tickets, d_out);
  // the rows of either kind, as every kernel from here on is handed them (the point pairs: no map, no points, no surface rows)
  const lfx::MapPose none{};
  const lfx::MapIndex no_map{};
  auto rows_of = [&](const lfx_map * m, const CloudSpan & k, double * r, double * J, uint32_t * nbr, double * reach) {
      return lfx::RowsOfKind{m ? m->index : no_map, reinterpret_cast<const float4 *>(k.points), k.begin, k.count, k.count_stride, r, J,
               k.row_begin, nbr, reach};
    };
  const lfx::RowsOfKind e = rows_of(pr.edge_map, pr.edge, r3, J3, nbr3, reach3), f = rows_of(pr.surface_map, pr.surface, r1, J1, nbr1, reach1);
  const lfx::StepRows e_rows = lfx::step_rows(e), f_rows = lfx::step_rows(f);          // (the step kernels only address rows)
  const uint32_t longest3 = pr.edge.longest, longest1 = pr.surface.longest;
  auto make_rows = [&](int iter) {                  // Problem::Make at the states' poses
      if (pr.X) {
        if (longest3) {
          hipLaunchKernelGGL(lfx::pair_rows_kernel, dim3((longest3 + 127u) / 128u, n_clouds), dim3(128), 0, st, pr.X, pr.Y,
            e.begin, e.count, r3, J3, states);
        }
      } else if (e.mi.start && f.mi.start) {
        // both maps have grids: the searches of both kinds in one launch, one wave per query; then the rows, one thread per query
        if (longest3 + longest1) {
          const uint32_t w3 = (longest3 + lfx::kSearchWaves - 1u) / lfx::kSearchWaves, w1 = (longest1 + lfx::kSearchWaves - 1u) / lfx::kSearchWaves;
          hipLaunchKernelGGL(lfx::map_search_kernel, dim3(w3 + w1, n_clouds), dim3(64 * lfx::kSearchWaves), 0, st, e, f, w3,
            pr.n_neighbors, states, iter);
          const uint32_t g3 = (longest3 + lfx::kRowThreads - 1u) / lfx::kRowThreads, g1 = (longest1 + lfx::kRowThreads - 1u) / lfx::kRowThreads;
          hipLaunchKernelGGL(lfx::rows_from_neighbours_kernel, dim3(g3 + g1, n_clouds), dim3(lfx::kRowThreads), 0, st, e, f, g3,
            pr.n_neighbors, states);
        }
      } else {
        if (longest3) {launch_rows(false, e, none, pr.n_neighbors, n_clouds, longest3, states, st);}
        if (longest1) {launch_rows(true, f, none, pr.n_neighbors, n_clouds, longest1, states, st);}
      }
    };
  auto iteration = [&](int iter) {
      make_rows(iter);
      hipLaunchKernelGGL(lfx::align_scale_kernel, dim3(n_clouds), dim3(lfx::kScaleThreads), 0, st, states, iter, e_rows, f_rows,
        d_weights, d_active, d_out);
      hipLaunchKernelGGL(lfx::align_update_kernel, dim3(lfx::kAlignSlices, n_clouds), dim3(lfx::kAlignThreads), 0, st, states, iter,
        max_iter, e_rows, f_rows, d_weights, d_partials, d_tickets, d_active, d_out);
    };
  // As many iterations as the previous call needed are queued at once (a finished scan's kernels return at once, but a launch
  // is a launch); only then does the host look -- at the records in its own memory -- and, where a scan still iterates,
  // goes on one iteration at a time.
  int launched = 0, target = std::min(max_iter, std::max(1, c->align_guess));
  for (;;) {
    for (; launched < target; launched++) {iteration(launched);}
    LFX_HIP(c, hipGetLastError());
    auto all_done = [&]() {
        for (uint32_t s = 0; s < n_clouds; s++) {if (out[s].done == 0) {return false;}}
        return true;
      };
    const hipError_t q = wait_for_records(all_done, st);
    LFX_HIP(c, q);
    if (all_done()) {break;}
    if (launched >= max_iter) {return fail(c, LFX_ERR_HIP, "the alignment did not finish within its iterations");}   // (cannot happen)
    target = launched + 1;
  }
  int needed = 1;
  for (uint32_t s = 0; s < n_clouds; s++) {
    for (int i = 0; i < 12; i++) {results[s].pose[i] = out[s].pose[i];}
    results[s].error = out[s].error; results[s].error_scale = out[s].scale;
    results[s].iteration = out[s].iteration; results[s].code = out[s].code;
    needed = std::max(needed, std::min(out[s].iteration + 1, max_iter));
  }
  c->align_guess = needed;
  if (!reports) {return LFX_OK;}
  // The reports: one more Problem::Make at the poses that were returned -- each handed over as lfx_scan_to_map_residuals
  // hands a pose to the same row kernels, so the rows are the ones a caller gets there -- for the scans that have a pose to
  // speak of, then the two report kernels.  The step kernels are not run: nothing moves.
  std::memset(reports, 0, sizeof(lfx_align_report) * (size_t)n_clouds);
  if (!report) {return LFX_OK;}
  uint8_t * h_rep = c->h_align.p + pose_bytes + out_bytes;
  lfx::ReportPose * h_pose = reinterpret_cast<lfx::ReportPose *>(h_rep);
  volatile lfx::AlignReport * h_report = reinterpret_cast<volatile lfx::AlignReport *>(h_rep + sizeof(lfx::ReportPose) * (size_t)n_clouds);
  volatile int32_t * h_done = reinterpret_cast<volatile int32_t *>(h_rep + (sizeof(lfx::ReportPose) + sizeof(lfx::AlignReport)) * (size_t)n_clouds);
  uint32_t to_run = 0;
  for (uint32_t s = 0; s < n_clouds; s++) {
    const int code = results[s].code;
    const bool run = LFX_ALIGN_SUCCESS(code) || code == LFX_ALIGN_MAX_ITERATION;
    map_pose_of(results[s].pose, h_pose[s].pose);
    h_pose[s].run = run ? 1 : 0; h_pose[s].pad = 0;
    h_done[s] = run ? 0 : 1;
    to_run += run ? 1u : 0u;
  }
  if (to_run == 0) {return LFX_OK;}
  uint8_t * d_rep = static_cast<uint8_t *>(d_pinned) + pose_bytes + out_bytes;
  hipLaunchKernelGGL(lfx::report_begin_kernel, dim3((n_clouds + 63u) / 64u), dim3(64), 0, st, states,
    reinterpret_cast<const lfx::ReportPose *>(d_rep), n_clouds, d_tickets);
  make_rows(1);                                       // (not the first search of these queries: it starts from the last one's reach)
  hipLaunchKernelGGL(lfx::align_report_scale_kernel, dim3(n_clouds), dim3(lfx::kScaleThreads), 0, st, states, e_rows, f_rows, d_weights, d_sums);
  hipLaunchKernelGGL(lfx::align_report_kernel, dim3(lfx::kAlignSlices, n_clouds), dim3(lfx::kAlignThreads), 0, st, states, e_rows, f_rows,
    d_weights, d_sums, d_partials, d_tickets,
    reinterpret_cast<lfx::AlignReport *>(d_rep + sizeof(lfx::ReportPose) * (size_t)n_clouds),
    reinterpret_cast<int32_t *>(d_rep + (sizeof(lfx::ReportPose) + sizeof(lfx::AlignReport)) * (size_t)n_clouds));
  LFX_HIP(c, hipGetLastError());
  auto all_reported = [&]() {
      for (uint32_t s = 0; s < n_clouds; s++) {if (h_done[s] == 0) {return false;}}
      return true;
    };
  const hipError_t q = wait_for_records(all_reported, st);
  LFX_HIP(c, q);
  if (!all_reported()) {return fail(c, LFX_ERR_HIP, "the alignment's reports were not written");}   // (cannot happen)
  for (uint32_t s = 0; s < n_clouds; s++) {
    if (h_pose[s].run && h_report[s].valid) {
      std::memcpy(&reports[s], const_cast<lfx::AlignReport *>(&h_report[s]), sizeof(lfx_align_report));
    }
  }
  return LFX_OK;
}
}  // namespace

extern "C" {

const char * lfx_align_message(int code)
{
  switch (code) {                         // the texts of optimization_result.hpp:43-79
    case LFX_ALIGN_CONVERGED: return "Optimization successfully converged";
    case LFX_ALIGN_LARGER_ERROR: return "The error is larger than previous iteration";
    case LFX_ALIGN_LARGER_SCALE: return "The scale is larger than previous iteration";
    case LFX_ALIGN_MAX_ITERATION: return "The iteration reached the maximum value";
    case LFX_ALIGN_EMPTY_INPUT: return "The input data is empty";
    case LFX_ALIGN_NO_PLANE: return "No surface neighbourhood spans a plane";
    case LFX_ALIGN_NOT_RUN: return "The scan was not aligned";
    default: return "unknown";
  }
}

}  // extern "C"

namespace lfx_host
{
int align_clouds(
  lfx_ctx * c, const lfx_map * edge_map, const lfx_map * surface_map, uint32_t n_neighbors, int max_iter, const CloudSpan & edge,
  const CloudSpan & surface, uint32_t n_clouds, const double * initial_poses, lfx_align_result * results, void * stream,
  lfx_align_report * reports)
{
  if (!c || !edge_map || !surface_map || !edge.points || !edge.begin || !edge.count || !surface.points ||
    !surface.begin || !surface.count || !initial_poses || !results || n_clouds == 0 || edge.count_stride == 0 ||
    surface.count_stride == 0)
  {
    return LFX_ERR_INVALID_ARGUMENT;
  }
  if (max_iter < 1) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "max_iter must be >= 1");}
  if (n_neighbors < 3 || n_neighbors > (uint32_t)lfx::kNearestMax || edge_map->index.n < n_neighbors || surface_map->index.n < n_neighbors) {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "n_neighbors must be in [3, 16] and both maps must hold that many points");
  }
  if (check_device(c, edge_map->device, "a map") != LFX_OK || check_device(c, surface_map->device, "a map") != LFX_OK) {
    return LFX_ERR_INVALID_ARGUMENT;
  }
  LFX_HIP(c, hipSetDevice(c->device));
  AlignProblem pr;
  pr.edge_map = edge_map; pr.surface_map = surface_map;
  pr.edge = edge; pr.surface = surface;
  pr.n_neighbors = n_neighbors;
  return run_align(c, pr, n_clouds, max_iter, initial_poses, results, static_cast<hipStream_t>(stream), reports);
}
}  // namespace lfx_host

extern "C" {

int lfx_scan_to_map_align(
  lfx_ctx * c, const lfx_map * edge_map, const lfx_map * surface_map, uint32_t n_neighbors, int max_iter,
  const float * d_edge_points, const uint32_t * d_edge_begin, const uint32_t * d_edge_count, uint32_t edge_count_stride,
  uint32_t max_edge_points_per_cloud, size_t total_edge_points,
  const float * d_surface_points, const uint32_t * d_surface_begin, const uint32_t * d_surface_count,
  uint32_t surface_count_stride, uint32_t max_surface_points_per_cloud, size_t total_surface_points,
  uint32_t n_clouds, const double * initial_poses, lfx_align_result * results, void * stream)
{
  const CloudSpan edge{d_edge_points, d_edge_begin, d_edge_count, edge_count_stride, max_edge_points_per_cloud, total_edge_points};
  const CloudSpan surface{d_surface_points, d_surface_begin, d_surface_count, surface_count_stride, max_surface_points_per_cloud,
    total_surface_points};
  return align_clouds(c, edge_map, surface_map, n_neighbors, max_iter, edge, surface, n_clouds, initial_poses, results, stream);
}

int lfx_scan_to_map_align_report(
  lfx_ctx * c, const lfx_map * edge_map, const lfx_map * surface_map, uint32_t n_neighbors, int max_iter,
  const float * d_edge_points, const uint32_t * d_edge_begin, const uint32_t * d_edge_count, uint32_t edge_count_stride,
  uint32_t max_edge_points_per_cloud, size_t total_edge_points,
  const float * d_surface_points, const uint32_t * d_surface_begin, const uint32_t * d_surface_count,
  uint32_t surface_count_stride, uint32_t max_surface_points_per_cloud, size_t total_surface_points,
  uint32_t n_clouds, const double * initial_poses, lfx_align_result * results, lfx_align_report * reports, void * stream)
{
  if (!reports) {return LFX_ERR_INVALID_ARGUMENT;}
  const CloudSpan edge{d_edge_points, d_edge_begin, d_edge_count, edge_count_stride, max_edge_points_per_cloud, total_edge_points};
  const CloudSpan surface{d_surface_points, d_surface_begin, d_surface_count, surface_count_stride, max_surface_points_per_cloud,
    total_surface_points};
  return align_clouds(c, edge_map, surface_map, n_neighbors, max_iter, edge, surface, n_clouds, initial_poses, results, stream, reports);
}

int lfx_align_point_pairs(
  lfx_ctx * c, const double * d_source, const double * d_target, const uint32_t * d_begin, const uint32_t * d_count,
  uint32_t max_points_per_cloud, size_t total_points, uint32_t n_clouds, int max_iter, const double * initial_poses,
  lfx_align_result * results, void * stream)
{
  if (!c || !d_source || !d_target || !d_begin || !d_count || !initial_poses || !results || n_clouds == 0) {return LFX_ERR_INVALID_ARGUMENT;}
  if (max_iter < 1) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "max_iter must be >= 1");}
  LFX_HIP(c, hipSetDevice(c->device));
  AlignProblem pr;
  pr.X = d_source; pr.Y = d_target;
  pr.edge = CloudSpan{nullptr, d_begin, d_count, 1, max_points_per_cloud, total_points};
  return run_align(c, pr, n_clouds, max_iter, initial_poses, results, static_cast<hipStream_t>(stream));
}

}  // extern "C"

namespace
{
// lfx_localize_batch and lfx_localize_host, with or without the reports
int localize_batch(
  lfx_ctx * c, const lfx_map * edge_map, const lfx_map * surface_map, uint32_t n_neighbors, int max_iter, float surface_leaf,
  uint32_t n_scans, const double * initial_poses, lfx_align_result * results, lfx_align_report * reports, void * stream)
{
  if (!c || !initial_poses || !results) {return LFX_ERR_INVALID_ARGUMENT;}
  const int rb = check_last_batch(c, n_scans);
  if (rb != LFX_OK) {return rb;}
  LFX_HIP(c, hipSetDevice(c->device));
  const uint32_t batch = c->last_batch;
  const size_t total = c->h_scan_begin[batch];
  hipStream_t st = static_cast<hipStream_t>(stream);
  // A few scans: nothing is asked of the device before the alignment.  The rows' scratch is sized by a bound (a scan has no
  // more edge points, and no more surface points, than points: 400 bytes per input point), the rows of scan s start where
  // its points do, and the launches are sized by the previous call's longest clouds (the kernels stride over what there is).
  const bool by_bound = 400u * total <= ((size_t)192 << 20);      // (four 64 x 1800 scans; the scratch only ever grows)
  // the downsampled clouds, then counts, status and the two tables of row starts; the clouds' lengths left in pinned memory
  BatchFront front;
  LFX_TRY(batch_front(c, c->align_surface, 4, true, c->h_loc, 0, false, surface_leaf, st, front));
  uint32_t * d_row3 = front.down_status + batch, * d_row1 = d_row3 + batch;
  volatile uint32_t * lengths = front.lengths;
  auto remember = [&]() {
      uint32_t e = 0, f = 0;
      for (uint32_t s = 0; s < batch; s++) {e = std::max(e, (uint32_t)lengths[2 * s]); f = std::max(f, (uint32_t)lengths[2 * s + 1]);}
      c->loc_guess[0] = e; c->loc_guess[1] = f;
    };
  CloudSpan edge{reinterpret_cast<const float *>(c->edge_pts.p), c->scan_begin.p, c->scan_info.p + lfx::kInfoEdge, 4};
  CloudSpan surface{front.down, c->scan_begin.p, front.down_count, 1};
  if (by_bound) {
    edge.longest = c->loc_guess[0] ? c->loc_guess[0] + c->loc_guess[0] / 8u : 4096u;
    surface.longest = c->loc_guess[1] ? c->loc_guess[1] + c->loc_guess[1] / 8u : 2048u;
    edge.total = surface.total = total;
    const int ra = align_clouds(c, edge_map, surface_map, n_neighbors, max_iter, edge, surface, batch, initial_poses, results, stream, reports);
    if (ra == LFX_OK) {remember();}
    return ra;
  }
  // Many scans: the clouds' real lengths first (one wait), so that the rows are packed -- scan s's rows start at the number of
  // edge (downsampled surface) points of the scans before it, 400 bytes per row of a few thousand rows per scan instead of
  // per input point
  LFX_HIP(c, hipStreamSynchronize(st));
  LFX_HIP(c, c->h_align.reserve(8 * (size_t)batch));
  uint32_t * rows = reinterpret_cast<uint32_t *>(c->h_align.p);
  for (uint32_t s = 0; s < batch; s++) {
    rows[s] = (uint32_t)edge.total; rows[batch + s] = (uint32_t)surface.total;
    edge.total += lengths[2 * s]; surface.total += lengths[2 * s + 1];
  }
  remember();
  edge.longest = c->loc_guess[0]; surface.longest = c->loc_guess[1];
  edge.row_begin = d_row3; surface.row_begin = d_row1;
  LFX_HIP(c, hipMemcpyAsync(d_row3, rows, sizeof(uint32_t) * 2 * batch, hipMemcpyHostToDevice, st));
  LFX_HIP(c, hipStreamSynchronize(st));              // (run_align lays its own records over the pinned block)
  return align_clouds(c, edge_map, surface_map, n_neighbors, max_iter, edge, surface, batch, initial_poses, results, stream, reports);
}

int localize_host(
  lfx_ctx * c, const lfx_map * edge_map, const lfx_map * surface_map, uint32_t n_neighbors, int max_iter, float surface_leaf,
  const float * edge_points, uint32_t n_edge, const float * surface_points, uint32_t n_surface, const double initial_pose[12],
  lfx_align_result * result, lfx_align_report * report, void * stream)
{
  if (!c || !edge_map || !surface_map || !initial_pose || !result || (n_edge && !edge_points) || (n_surface && !surface_points)) {
    return LFX_ERR_INVALID_ARGUMENT;
  }
  LFX_HIP(c, hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  // [edge | surface | downsampled surface] records of 4 floats, then the scan's words
  const size_t ne = n_edge, ns = n_surface;
  if (hold(c->align_surface, 4 * (ne + 2 * ns + 2) + kScanWords, true) != hipSuccess) {
    return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the scan's clouds");
  }
  float * d_edge = c->align_surface.p, * d_surface = d_edge + 4 * (ne + 1), * d_down = d_surface + 4 * (ns + 1);
  uint32_t * d_words = reinterpret_cast<uint32_t *>(d_down + 4 * ns);
  LFX_HIP(c, c->h_align.reserve(sizeof(uint32_t) * kScanWords));
  uint32_t * h_words = reinterpret_cast<uint32_t *>(c->h_align.p);
  if (n_edge) {LFX_HIP(c, hipMemcpyAsync(d_edge, edge_points, sizeof(float) * 4 * ne, hipMemcpyHostToDevice, st));}
  if (n_surface) {LFX_HIP(c, hipMemcpyAsync(d_surface, surface_points, sizeof(float) * 4 * ns, hipMemcpyHostToDevice, st));}
  CloudSpan edge, surface;
  LFX_TRY(scan_front(c, h_words, d_words, d_edge, n_edge, d_surface, n_surface, surface_leaf, d_down, nullptr, st, edge, surface));
  // the downsampled count back (one wait); with no surface cloud, the words have left the pinned block: the alignment stages
  // through it too
  if (n_surface) {LFX_HIP(c, hipMemcpyAsync(h_words + kScanDownCount, d_words + kScanDownCount, sizeof(uint32_t), hipMemcpyDeviceToHost, st));}
  LFX_HIP(c, hipStreamSynchronize(st));
  surface.longest = n_surface ? h_words[kScanDownCount] : 0u;
  return align_clouds(c, edge_map, surface_map, n_neighbors, max_iter, edge, surface, 1, initial_pose, result, stream, report);
}
}  // namespace

extern "C" {

int lfx_localize_batch(
  lfx_ctx * c, const lfx_map * edge_map, const lfx_map * surface_map, uint32_t n_neighbors, int max_iter, float surface_leaf,
  uint32_t n_scans, const double * initial_poses, lfx_align_result * results, void * stream)
{
  return localize_batch(c, edge_map, surface_map, n_neighbors, max_iter, surface_leaf, n_scans, initial_poses, results, nullptr, stream);
}

int lfx_localize_batch_report(
  lfx_ctx * c, const lfx_map * edge_map, const lfx_map * surface_map, uint32_t n_neighbors, int max_iter, float surface_leaf,
  uint32_t n_scans, const double * initial_poses, lfx_align_result * results, lfx_align_report * reports, void * stream)
{
  if (!reports) {return LFX_ERR_INVALID_ARGUMENT;}
  return localize_batch(c, edge_map, surface_map, n_neighbors, max_iter, surface_leaf, n_scans, initial_poses, results, reports, stream);
}

int lfx_localize_host(
  lfx_ctx * c, const lfx_map * edge_map, const lfx_map * surface_map, uint32_t n_neighbors, int max_iter, float surface_leaf,
  const float * edge_points, uint32_t n_edge, const float * surface_points, uint32_t n_surface, const double initial_pose[12],
  lfx_align_result * result, void * stream)
{
  return localize_host(c, edge_map, surface_map, n_neighbors, max_iter, surface_leaf, edge_points, n_edge, surface_points, n_surface,
           initial_pose, result, nullptr, stream);
}

int lfx_localize_host_report(
  lfx_ctx * c, const lfx_map * edge_map, const lfx_map * surface_map, uint32_t n_neighbors, int max_iter, float surface_leaf,
  const float * edge_points, uint32_t n_edge, const float * surface_points, uint32_t n_surface, const double initial_pose[12],
  lfx_align_result * result, lfx_align_report * report, void * stream)
{
  if (!report) {return LFX_ERR_INVALID_ARGUMENT;}
  return localize_host(c, edge_map, surface_map, n_neighbors, max_iter, surface_leaf, edge_points, n_edge, surface_points, n_surface,
           initial_pose, result, report, stream);
}

}  // extern "C"
