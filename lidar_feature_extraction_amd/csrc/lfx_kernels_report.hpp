// lfx_kernels_report.hpp -- how good a returned pose is: the information matrix of the alignment at that pose, its
// eigen-decomposition, a covariance, the degeneracy test and the fit's counts (lfx_align_report, include/lfx.h).
//
// The reference computes D = sum J^T J and A = sum w J^T J in every iteration (optimizer.cpp:40-72), asks D one yes / no
// question (IsDegenerate) and throws both away; its node publishes a constant covariance (subscriber.hpp:158-169).  Here
// the sums are taken once more at the pose the alignment RETURNED: run_align sets the scans' states to those poses
// (report_begin_kernel), runs the search and row kernels of an iteration, and then, instead of the two step kernels (which
// carry the stopping logic and move the pose),
//   align_report_scale_kernel  one workgroup per scan: ComputeErrors, Scale, ComputeWeights as align_scale_kernel has them
//                              (the medians need the whole scan in one workgroup), and the scalar sums and counts;
//   align_report_kernel        kAlignSlices workgroups per scan: D and A on the f64 matrix unit in align_update_kernel's tile
//                              layout, waves then slices added in a fixed order; the workgroup that finishes last completes
//                              the record (two threads of two waves: the two eigen-solves side by side) and writes it
//                              to pinned host memory.
// No floating-point atomics and no agent-scope fence: two calls on the same inputs give the same bytes.
#pragma once

#include "lfx_kernels_localize.hpp"

#pragma clang fp contract(off)

namespace lfx
{

struct AlignReport                        // lfx_align_report, field for field (lfx_localize.hip asserts the size)
{
  double information[36], eigenvalues[6], eigenvectors[36], covariance[36];
  double sigma2, min_eigenvalue_d, error, error_scale, rms_edge, rms_surface;
  uint32_t n_edge, n_surface, n_edge_inliers, n_surface_inliers, n_surface_no_plane;
  int32_t rank, degenerate, valid;
};

struct ReportPose                         // what the host hands the report pass, per scan (pinned host memory)
{
  MapPose pose;                           // result.pose and Eigen::Quaterniond of its rotation, as lfx_scan_to_map_residuals derives it
  int32_t run, pad;                       // 0: no report for this scan (its kernels return at once)
};

struct ReportSums                         // from align_report_scale_kernel to align_report_kernel, per scan
{
  double e_edge, e_surface, weighted_error, weighted_dim, scale;
  uint32_t n_edge, n_surface, n_edge_inliers, n_surface_inliers, n_surface_no_plane, pad;
};

__global__ void report_begin_kernel(AlignState * __restrict__ states, const ReportPose * __restrict__ in, uint32_t n,
  uint32_t * __restrict__ tickets)
{
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) {return;}
  tickets[s] = 0u;
  const ReportPose p = in[s];
  AlignState & st = states[s];
  st.pose = p.pose;                        // (prev_m stays: the searches bound how far a query has moved since their last run)
  st.done = p.run ? 0 : 1;
  st.surface_rows_with_plane = 0;
}

// ComputeErrors / NormalizeErrorScale / ComputeWeights (optimizer.cpp:100-128) at the report's pose: the weights of the
// scan's residuals into `weights` (rows of scan s from b3 + b1, as align_scale_kernel leaves them), the sums
// over residuals into sums[s].  Sums in a fixed tree order.
__global__ __launch_bounds__(kScaleThreads) void align_report_scale_kernel(
  const AlignState * __restrict__ states, StepRows e, StepRows f, double * __restrict__ weights, ReportSums * __restrict__ sums)
{
  constexpr int T = kScaleThreads, W = T / 64;
  const uint32_t s = blockIdx.x;
  const int tid = threadIdx.x;
  __shared__ __attribute__((aligned(8))) uint32_t sh[kSelectWords];
  __shared__ double keys_lds[kAlignKeysLds];
  __shared__ double part[W][4];
  __shared__ uint32_t cnt[W][3];
  const StepExtents x = step_extents(states[s], e, f, s);
  if (x.done) {return;}
  const double * r3 = e.residual, * r1 = f.residual, * J1 = f.jacobian;
  const uint32_t n3 = x.n3, b3 = x.b3, n1 = x.n1, b1 = x.b1, n = n3 + n1;
  if (n == 0u) {
    if (tid == 0) {sums[s] = ReportSums{};}
    return;
  }
  double * w_out = weights + (size_t)b3 + b1;
  double * key = n <= (uint32_t)kAlignKeysLds ? keys_lds : w_out;     // (a longer scan: the keys pass through the weights' place)
  if (tid < 256) {sh[tid] = 0u;}
  for (uint32_t i = tid; i < n; i += T) {key[i] = row_error(x, r3, r1, i);}
  __syncthreads();
  const double median = workgroup_median(key, n, sh);
  for (uint32_t i = tid; i < n; i += T) {key[i] = fabs(key[i] - median);}
  __syncthreads();
  const double scale = 1.482602218505602 * workgroup_median(key, n, sh);
  __syncthreads();
  double se3 = 0., se1 = 0., swe = 0., swd = 0.;
  uint32_t in3 = 0, in1 = 0, zero = 0;
  for (uint32_t i = tid; i < n; i += T) {
    const double err = row_error(x, r3, r1, i), en = err / (scale + 1e-16);
    const bool inlier = en < 1.345 * 1.345;
    const double w = inlier ? 1. : 1.345 / sqrt(en);
    w_out[i] = w;
    swe += w * err;
    if (i < n3) {
      se3 += err; swd += 3. * w; in3 += inlier ? 1u : 0u;
    } else {
      const double * J = J1 + 7 * ((size_t)b1 + (i - n3));
      se1 += err; swd += w; in1 += inlier ? 1u : 0u;
      zero += J[4] == 0. && J[5] == 0. && J[6] == 0. ? 1u : 0u;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    se3 += __shfl_xor(se3, off, 64); se1 += __shfl_xor(se1, off, 64); swe += __shfl_xor(swe, off, 64); swd += __shfl_xor(swd, off, 64);
    in3 += (uint32_t)__shfl_xor((int)in3, off, 64); in1 += (uint32_t)__shfl_xor((int)in1, off, 64);
    zero += (uint32_t)__shfl_xor((int)zero, off, 64);
  }
  if ((tid & 63) == 0) {
    part[tid >> 6][0] = se3; part[tid >> 6][1] = se1; part[tid >> 6][2] = swe; part[tid >> 6][3] = swd;
    cnt[tid >> 6][0] = in3; cnt[tid >> 6][1] = in1; cnt[tid >> 6][2] = zero;
  }
  __syncthreads();
  if (tid != 0) {return;}
  ReportSums o{};
  for (int wv = 0; wv < W; wv++) {
    o.e_edge += part[wv][0]; o.e_surface += part[wv][1]; o.weighted_error += part[wv][2]; o.weighted_dim += part[wv][3];
    o.n_edge_inliers += cnt[wv][0]; o.n_surface_inliers += cnt[wv][1]; o.n_surface_no_plane += cnt[wv][2];
  }
  o.scale = scale; o.n_edge = n3; o.n_surface = n1;
  sums[s] = o;
}

// Cyclic Jacobi on the symmetric N x N matrix a (row-major, both triangles): on return its diagonal holds the eigenvalues
// and, with VECTORS, column k of v the unit eigenvector of a[k][k].  Sweeps until the off-diagonal norm is below 2^-50 of
// the diagonal's; false if kJacobiSweeps sweeps did not get there (a NaN never does).  Every index is a constant after
// unrolling: the matrices live in registers.
constexpr int kJacobiSweeps = 30;
template<int N, bool VECTORS>
__device__ __forceinline__ bool jacobi_eigen(double (&a)[N * N], double (&v)[N * N])
{
  if (VECTORS) {
#pragma unroll
    for (int i = 0; i < N * N; i++) {v[i] = i / N == i % N ? 1. : 0.;}
  }
  for (int sweep = 0; sweep <= kJacobiSweeps; sweep++) {
    double off = 0., diag = 0.;
#pragma unroll
    for (int p = 0; p < N; p++) {
      diag += a[N * p + p] * a[N * p + p];
#pragma unroll
      for (int q = p + 1; q < N; q++) {off += a[N * p + q] * a[N * p + q];}
    }
    if (2. * off <= 7.888609052210118e-31 * diag) {return true;}          // 2^-100: the norms' squares
    if (sweep == kJacobiSweeps) {break;}
#pragma unroll
    for (int p = 0; p < N; p++) {
#pragma unroll
      for (int q = p + 1; q < N; q++) {
        const double apq = a[N * p + q];
        if (apq != 0.) {
          const double theta = (a[N * q + q] - a[N * p + p]) / (2. * apq);
          const double t = (theta < 0. ? -1. : 1.) / (fabs(theta) + sqrt(theta * theta + 1.));
          const double c = 1. / sqrt(t * t + 1.), sn = t * c;
#pragma unroll
          for (int k = 0; k < N; k++) {                                 // a <- a J
            const double akp = a[N * k + p], akq = a[N * k + q];
            a[N * k + p] = c * akp - sn * akq;
            a[N * k + q] = sn * akp + c * akq;
          }
#pragma unroll
          for (int k = 0; k < N; k++) {                                 // a <- J^T a
            const double apk = a[N * p + k], aqk = a[N * q + k];
            a[N * p + k] = c * apk - sn * aqk;
            a[N * q + k] = sn * apk + c * aqk;
          }
          a[N * p + q] = 0.; a[N * q + p] = 0.;
          if (VECTORS) {
#pragma unroll
            for (int k = 0; k < N; k++) {
              const double vkp = v[N * k + p], vkq = v[N * k + q];
              v[N * k + p] = c * vkp - sn * vkq;
              v[N * k + q] = sn * vkp + c * vkq;
            }
          }
        }
      }
    }
  }
  return false;
}

// The rest of a scan's report, on two threads of different waves side by side (each eigen-solve is a chain of dependent
// rotations: one thread after the other took 73 us for a scan): total = the 16 x 16 tile of sums (D in rows 0-6, A in rows
// 8-14).  o is the record's place in pinned host memory, written field by field and never read (the record built in
// registers first would be 248 of them); the caller sets `valid` from what the two return.
// D's part: IsDegenerate and the smallest eigenvalue.
__device__ __forceinline__ bool report_finish_d(const double * total, AlignReport & o)
{
  double D[49], unused[49];
#pragma unroll
  for (int a = 0; a < 7; a++) {                              // the upper triangle, mirrored
#pragma unroll
    for (int c = a; c < 7; c++) {D[7 * a + c] = total[16 * a + c]; D[7 * c + a] = total[16 * a + c];}
  }
  o.degenerate = is_degenerate7(D, 0.1) ? 1 : 0;
  const bool ok = jacobi_eigen<7, false>(D, unused);
  double dmin = D[0];
#pragma unroll
  for (int a = 1; a < 7; a++) {dmin = D[8 * a] < dmin ? D[8 * a] : dmin;}
  o.min_eigenvalue_d = dmin;
  return ok;
}

// A's part: H, its eigen-decomposition, the covariance, the scalars and the counts.
__device__ __forceinline__ bool report_finish_h(const double * total, const MapPose & P, const ReportSums & sm, AlignReport & o)
{
  double A[49];
#pragma unroll
  for (int a = 0; a < 7; a++) {
#pragma unroll
    for (int c = a; c < 7; c++) {A[7 * a + c] = total[16 * (8 + a) + c]; A[7 * c + a] = total[16 * (8 + a) + c];}
  }
  // H = M^T A M, M = MakeM(q) (optimizer.cpp:74-85): [0.5 * LeftMultiplicationMatrix(q)[:, 1:4], 0; 0, I]
  const double w = P.qw, x = P.qx, y = P.qy, z = P.qz;
  const double L[16] = {w, -x, -y, -z, x, w, -z, y, y, z, w, -x, z, -y, x, w};
  double M[42];
#pragma unroll
  for (int i = 0; i < 42; i++) {M[i] = 0.;}
#pragma unroll
  for (int r = 0; r < 4; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) {M[6 * r + c] = 0.5 * L[4 * r + 1 + c];}
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {M[6 * (4 + a) + 3 + a] = 1.;}
  double AM[42], H[36], V[36];
#pragma unroll
  for (int r = 0; r < 7; r++) {
#pragma unroll
    for (int c = 0; c < 6; c++) {
      double sum = 0.;
#pragma unroll
      for (int k = 0; k < 7; k++) {sum += A[7 * r + k] * M[6 * k + c];}
      AM[6 * r + c] = sum;
    }
  }
  bool nan = false;
#pragma unroll
  for (int r = 0; r < 6; r++) {
#pragma unroll
    for (int c = r; c < 6; c++) {
      double sum = 0.;
#pragma unroll
      for (int k = 0; k < 7; k++) {sum += M[6 * k + r] * AM[6 * k + c];}
      H[6 * r + c] = sum; H[6 * c + r] = sum;
      nan = nan || sum != sum;
    }
  }
#pragma unroll
  for (int i = 0; i < 36; i++) {o.information[i] = H[i];}
  const bool ok = !nan && jacobi_eigen<6, true>(H, V);
  // ascending eigenvalues, their vectors as rows, the largest-magnitude component of each positive
  double lam[6], vec[36];
#pragma unroll
  for (int k = 0; k < 6; k++) {
    lam[k] = H[7 * k];
#pragma unroll
    for (int c = 0; c < 6; c++) {vec[6 * k + c] = V[6 * c + k];}
  }
#pragma unroll
  for (int pass = 0; pass < 5; pass++) {
#pragma unroll
    for (int k = 0; k < 5 - pass; k++) {
      const bool swap = lam[k + 1] < lam[k];
      const double lo = swap ? lam[k + 1] : lam[k], hi = swap ? lam[k] : lam[k + 1];
      lam[k] = lo; lam[k + 1] = hi;
#pragma unroll
      for (int c = 0; c < 6; c++) {
        const double u0 = vec[6 * k + c], u1 = vec[6 * (k + 1) + c];
        vec[6 * k + c] = swap ? u1 : u0; vec[6 * (k + 1) + c] = swap ? u0 : u1;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 6; k++) {
    double big = vec[6 * k];
#pragma unroll
    for (int c = 1; c < 6; c++) {big = fabs(vec[6 * k + c]) > fabs(big) ? vec[6 * k + c] : big;}
    const double sign = big < 0. ? -1. : 1.;
#pragma unroll
    for (int c = 0; c < 6; c++) {vec[6 * k + c] *= sign;}
  }
  const double dim = sm.weighted_dim - 6.;
  const double sigma2 = dim > 0. ? sm.weighted_error / dim : __longlong_as_double(0x7FF8000000000000ll);
  const double floor_ = 1e-9 * lam[5];
  int rank = 0;
  double inv[6];
#pragma unroll
  for (int k = 0; k < 6; k++) {
    rank += lam[k] > floor_ ? 1 : 0;
    inv[k] = sigma2 / (lam[k] > floor_ ? lam[k] : floor_);
    o.eigenvalues[k] = lam[k];
  }
#pragma unroll
  for (int i = 0; i < 36; i++) {o.eigenvectors[i] = vec[i];}
#pragma unroll
  for (int r = 0; r < 6; r++) {
#pragma unroll
    for (int c = r; c < 6; c++) {
      double sum = 0.;
#pragma unroll
      for (int k = 0; k < 6; k++) {sum += inv[k] * (vec[6 * k + r] * vec[6 * k + c]);}
      o.covariance[6 * r + c] = sum; o.covariance[6 * c + r] = sum;
    }
  }
  o.sigma2 = sigma2;
  o.error = sm.e_edge + sm.e_surface; o.error_scale = sm.scale;
  o.rms_edge = sm.n_edge ? sqrt(sm.e_edge / (double)sm.n_edge) : 0.;
  o.rms_surface = sm.n_surface ? sqrt(sm.e_surface / (double)sm.n_surface) : 0.;
  o.n_edge = sm.n_edge; o.n_surface = sm.n_surface;
  o.n_edge_inliers = sm.n_edge_inliers; o.n_surface_inliers = sm.n_surface_inliers; o.n_surface_no_plane = sm.n_surface_no_plane;
  o.rank = rank;
  return ok;
}

// The sums of the report, kAlignSlices workgroups per scan (blockIdx.y): normal_equation_sums as align_update_kernel takes
// them (its comment has the operand and result lanes), D in rows 0-6 and A in rows 8-14 of the 16 x 16 tile; the workgroup
// that draws the last ticket completes the record.  out / out_done: pinned host memory.
__global__ __launch_bounds__(kAlignThreads) void align_report_kernel(
  const AlignState * __restrict__ states, StepRows e, StepRows f, const double * __restrict__ weights,
  const ReportSums * __restrict__ sums, double * __restrict__ partials, uint32_t * __restrict__ tickets,
  AlignReport * __restrict__ out, int32_t * __restrict__ out_done)
{
  const uint32_t s = blockIdx.y;
  const int tid = threadIdx.x;
  __shared__ double total[kAlignTile];
  __shared__ uint32_t d_ok;
  const StepExtents x = step_extents(states[s], e, f, s);
  if (x.done) {return;}
  if (!normal_equation_sums(x, e, f, weights, partials, tickets, s, blockIdx.x, total)) {return;}
  const ReportSums sm = sums[s];
  const bool rows = sm.n_edge + sm.n_surface != 0u;
  if (tid == 64) {                                           // (wave 1: D's eigenvalues beside H's)
    d_ok = rows && report_finish_d(total, out[s]) ? 1u : 0u;
    __threadfence_system();
  }
  bool ok = false;
  if (tid == 0 && rows) {ok = report_finish_h(total, states[s].pose, sm, out[s]);}
  __syncthreads();
  if (tid != 0) {return;}
  tickets[s] = 0u;
  out[s].valid = ok && d_ok != 0u ? 1 : 0;                   // (0: the host leaves the caller's record all zero)
  __threadfence_system();
  *reinterpret_cast<volatile int32_t *>(&out_done[s]) = 1;
}

}  // namespace lfx
