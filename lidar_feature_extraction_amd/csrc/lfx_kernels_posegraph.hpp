// lfx_kernels_posegraph.hpp -- the kernels of the pose-graph optimiser (include/lfx.h, the pose graph section;
// lfx_posegraph.hip launches them).  One Gauss-Newton iteration of (H + lambda I) delta = -g over a graph that is a chain plus
// a few loops: H = P + Jt^T Jt, P block-tridiagonal in node order (lambda I and the chain edges), Jt the loop edges' rows
// whitened by their information (Omega = C C^T, Jt = sqrt(w) C^T J).  The step is
//   y0 = P^-1 (-g),  Y = P^-1 Jt^T,  S = I + Jt Y,  delta = y0 - Y S^-1 (Jt y0)
// which is the step of S = W^-1 + J Y (lfx.h) with both sides of S multiplied by sqrt(w) C^T: S has no eigenvalue below 1.
//
// Priors (unary terms: lfx.h, PRIORS) touch P's diagonal blocks and the gradient only: a kernel of their own linearises them,
// the per-node assembly walks a node's priors after its edges, the reduction passes over them after the edges.  Every loop
// over priors runs zero times for a graph without them, which therefore computes, byte for byte, what it always did.
//
// No floating-point atomic anywhere: every sum has a fixed order (an edge's sums are one thread's, a node's gradient walks
// the node's incidence list in edge order and then its priors in prior order, the reductions are a strided pass per thread
// and a tree), so the same inputs give the same bytes.  A pivot that is not positive sets the status word; every kernel but the linearisation and the reduction returns at
// once when it is set.  Built with contraction off, as the rest of the library.
#pragma once

#include "lfx_kernels_common.hpp"

namespace lfx
{

constexpr int kPgThreads = 256;          // the reductions, the S kernels, the step
constexpr int kPgWave = 64;              // the chain kernels and the per-node assembly: one wave per workgroup
constexpr int kPgPanel = 48;             // panel width of the S factor (8 loop edges)
constexpr int kPgTile = 16;              // the trailing update's tile
constexpr int kPgLin = 88;               // doubles of an edge's linearisation: r[6], q[6] = w Omega r, w, rho, 2 spare, A_i[36], A_j[36]
constexpr int kPgPlin = 52;              // doubles of a prior's linearisation: r[6], q[6] = w Omega r, w, rho, 2 spare, A[36]
constexpr uint32_t kPgNone = 0xFFFFFFFFu;
constexpr uint32_t kPgEdgeRobust = 1u;   // LFX_EDGE_ROBUST
constexpr uint32_t kPgPriorRobust = 1u;  // LFX_PRIOR_ROBUST
constexpr uint32_t kPgPriorPosition = 2u;  // LFX_PRIOR_POSITION
enum PgStatus : uint32_t {kPgOk = 0, kPgChainPivot = 1, kPgLoopInformation = 2, kPgLoopPivot = 3};

struct PgEdge                            // lfx_pose_graph_edge as the device holds it (400 bytes)
{
  uint32_t i, j, flags, loop;            // loop: the edge's place among the loop edges, kPgNone for a chain edge
  double z[12];
  double omega[36];
};
struct PgPrior                           // lfx_pose_graph_prior as the caller wrote it (416 bytes)
{
  uint32_t node, flags;
  double z[12];
  double omega[36];                      // a position prior's block in the lower right, zeros outside it
  double lever[3];
};
struct PgRecord                          // what the host reads once per iteration
{
  double chi2, max_step;
  uint32_t status, n_down;
  double chi2_prior;                     // the priors' share of chi2
  uint32_t n_down_prior, spare;
};

struct PgArgs
{
  double * poses;                        // [N][12]
  const uint8_t * fixed;                 // [N]
  const PgEdge * edges;                  // [E]
  double * lin;                          // [E][kPgLin]
  double * loop_j;                       // [L][2][36]: the whitened rows of loop edge l, side i then side j (zero for a fixed node)
  const uint32_t * node_begin, * inc;    // incidence: node k's entries inc[node_begin[k] .. node_begin[k + 1]), each edge * 2 + side
  const uint32_t * chain_edge;           // [N]: the chain edge k -> k + 1, or kPgNone
  const uint32_t * loop_edge;            // [L]: the loop edges in edge order
  double * grad;                         // [N][6]
  double * diag, * off;                  // [N][36] each: P's blocks (k, k) and (k + 1, k)
  double * fac_l, * fac_m;               // [N][36] each: L_k (its diagonal holds 1 / L_k(r, r)) and M_k, P = (L, M)(L, M)^T
  double * y;                            // [6 N][ldy]: column 0 is y0, column 1 + 6 l + c the loop edge l's row c
  double * s;                            // [6 L][6 L]: S, then its Cholesky factor in the lower triangle
  double * z;                            // [6 L]: Jt y0, then S^-1 of it
  double * step_max;                     // [N]
  uint32_t * status;
  PgRecord * record;
  uint32_t n_nodes, n_edges, n_loop, ldy;
  double huber_delta, damping;
  const PgPrior * priors;                // [P]
  double * plin;                         // [P][kPgPlin]
  const uint32_t * prior_begin, * prior_inc;   // node k's priors prior_inc[prior_begin[k] .. prior_begin[k + 1]), in prior order
  uint32_t n_priors;
};

// ---------------------------------------------------------------------------------------------- small fixed-size arithmetic
__device__ inline double pg_dot3(double a0, double b0, double a1, double b1, double a2, double b2) {return (a0 * b0 + a1 * b1) + a2 * b2;}

// the larger of two values, a NaN kept (fmax drops it; the host must see a step that is not a number)
__device__ inline double pg_max(double a, double b) {return (a != a || b != b) ? a + b : fmax(a, b);}

// c = a^T b, 3 x 3 row-major
__device__ inline void pg_tmul3(const double * a, const double * b, double * c)
{
  for (int r = 0; r < 3; r++) {
    for (int k = 0; k < 3; k++) {c[3 * r + k] = pg_dot3(a[r], b[k], a[3 + r], b[3 + k], a[6 + r], b[6 + k]);}
  }
}

// the lower Cholesky factor of the 6 x 6 matrix a (its lower triangle is read), in place; false on a pivot that is not > 0
__device__ inline bool pg_chol6(double * a)
{
  bool ok = true;
  for (int j = 0; j < 6; j++) {
    double p = a[7 * j];
    for (int m = 0; m < j; m++) {p -= a[6 * j + m] * a[6 * j + m];}
    ok = ok && (p > 0.0);
    const double d = sqrt(p);
    a[7 * j] = d;
    for (int r = j + 1; r < 6; r++) {
      double v = a[6 * r + j];
      for (int m = 0; m < j; m++) {v -= a[6 * r + m] * a[6 * j + m];}
      a[6 * r + j] = v / d;
    }
  }
  return ok;
}

// ---------------------------------------------------------------------------------------------- 1. linearise
// An edge's r = (phi, t_E) and its Jacobians A_i, A_j at the poses pi, pj ([R | t], 12 doubles each) under the measurement z.
// The one routine of every relative-pose term: an edge passes its two nodes, a pose prior the identity and its node.
__device__ inline void pg_edge_terms(const double * pi, const double * pj, const double * z, double * res, double * Ai, double * Aj)
{
  double Ri[9], Rj[9], Rz[9], ti[3], tj[3], tz[3];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) {Ri[3 * r + c] = pi[4 * r + c]; Rj[3 * r + c] = pj[4 * r + c]; Rz[3 * r + c] = z[4 * r + c];}
    ti[r] = pi[4 * r + 3]; tj[r] = pj[4 * r + 3]; tz[r] = z[4 * r + 3];
  }
  double M[9], RE[9], RzRi[9], d[3], tE[3];
  pg_tmul3(Ri, Rj, M);                 // R_i^T R_j
  pg_tmul3(Rz, M, RE);                 // R_Z^T R_i^T R_j
  const double dt[3] = {tj[0] - ti[0], tj[1] - ti[1], tj[2] - ti[2]};
  for (int r = 0; r < 3; r++) {d[r] = pg_dot3(Ri[r], dt[0], Ri[3 + r], dt[1], Ri[6 + r], dt[2]);}
  const double dz[3] = {d[0] - tz[0], d[1] - tz[1], d[2] - tz[2]};
  for (int r = 0; r < 3; r++) {tE[r] = pg_dot3(Rz[r], dz[0], Rz[3 + r], dz[1], Rz[6 + r], dz[2]);}
  // (R_Z^T R_i^T)(r, c) = sum_k R_Z(k, r) R_i(c, k)
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) {RzRi[3 * r + c] = pg_dot3(Rz[r], Ri[3 * c], Rz[3 + r], Ri[3 * c + 1], Rz[6 + r], Ri[3 * c + 2]);}
  }
  // Log
  const double v[3] = {0.5 * (RE[7] - RE[5]), 0.5 * (RE[2] - RE[6]), 0.5 * (RE[3] - RE[1])};
  const double nv = sqrt(pg_dot3(v[0], v[0], v[1], v[1], v[2], v[2]));
  const double theta = atan2(nv, 0.5 * (((RE[0] + RE[4]) + RE[8]) - 1.0));
  double phi[3];
  const double scale = nv < 1e-10 ? 1.0 : theta / nv;
  for (int r = 0; r < 3; r++) {phi[r] = nv < 1e-10 ? v[r] : v[r] * scale;}
  // J_r^-1(phi) = I + [phi]x / 2 + c [phi]x^2
  const double cc = theta < 1e-4 ? 1.0 / 12.0 + theta * theta / 720.0 : 1.0 / (theta * theta) - (1.0 + cos(theta)) / (2.0 * theta * sin(theta));
  const double px[9] = {0.0, -phi[2], phi[1], phi[2], 0.0, -phi[0], -phi[1], phi[0], 0.0};
  double Jri[9];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) {
      const double p2 = pg_dot3(px[3 * r], px[c], px[3 * r + 1], px[3 + c], px[3 * r + 2], px[6 + c]);
      Jri[3 * r + c] = ((r == c ? 1.0 : 0.0) + 0.5 * px[3 * r + c]) + cc * p2;
    }
  }
  for (int k = 0; k < 36; k++) {Ai[k] = 0.0; Aj[k] = 0.0;}
  const double dx[9] = {0.0, -d[2], d[1], d[2], 0.0, -d[0], -d[1], d[0], 0.0};
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) {
      Aj[6 * r + c] = Jri[3 * r + c];
      Aj[6 * (3 + r) + 3 + c] = RzRi[3 * r + c];
      // -Jri R_j^T R_i = -Jri M^T
      Ai[6 * r + c] = -pg_dot3(Jri[3 * r], M[3 * c], Jri[3 * r + 1], M[3 * c + 1], Jri[3 * r + 2], M[3 * c + 2]);
      Ai[6 * (3 + r) + c] = pg_dot3(Rz[r], dx[c], Rz[3 + r], dx[3 + c], Rz[6 + r], dx[6 + c]);
      Ai[6 * (3 + r) + 3 + c] = -RzRi[3 * r + c];
    }
  }
  for (int r = 0; r < 3; r++) {res[r] = phi[r]; res[3 + r] = tE[r];}
}

// q = Omega r, rho = r^T Omega r and w = 1, or Huber's where `robust` and s = sqrt(r^T Omega r) lies beyond huber_delta:
// the cost and the weight of every term, edge or prior.  q comes back unweighted.
__device__ inline void pg_weigh(const double * omega, const double * res, bool robust, double huber_delta, double * q, double & w, double & rho)
{
  double s2 = 0.0;
  for (int r = 0; r < 6; r++) {
    double acc = 0.0;
    for (int c = 0; c < 6; c++) {acc += omega[6 * r + c] * res[c];}
    q[r] = acc;
  }
  for (int r = 0; r < 6; r++) {s2 += res[r] * q[r];}
  w = 1.0; rho = s2;
  if (robust) {
    const double s = sqrt(s2 > 0.0 ? s2 : 0.0);
    if (s > huber_delta) {
      w = huber_delta / s;
      rho = 2.0 * huber_delta * s - huber_delta * huber_delta;
    }
  }
}

// One thread per edge: r, w, rho, q = w Omega r, A_i, A_j (lfx.h states them); a loop edge also gets its whitened rows.
// Not gated on the status word, which this kernel itself may set (a loop edge's information without a Cholesky factor): every
// edge's values are written whatever another workgroup found, so chi^2 and lfx_pose_graph_edge_chi2 never depend on the order
// the workgroups ran in.
__global__ __launch_bounds__(kPgWave) void pose_graph_linearize_kernel(PgArgs a)
{
  const uint32_t e = blockIdx.x * kPgWave + threadIdx.x;
  if (e >= a.n_edges) {return;}
  const PgEdge & ed = a.edges[e];
  double res[6], Ai[36], Aj[36], q[6], w, rho;
  pg_edge_terms(a.poses + 12 * (size_t)ed.i, a.poses + 12 * (size_t)ed.j, ed.z, res, Ai, Aj);
  pg_weigh(ed.omega, res, (ed.flags & kPgEdgeRobust) != 0u, a.huber_delta, q, w, rho);
  double * out = a.lin + (size_t)kPgLin * e;
  for (int r = 0; r < 6; r++) {out[r] = res[r]; out[6 + r] = w * q[r];}
  out[12] = w; out[13] = rho; out[14] = 0.0; out[15] = 0.0;
  for (int k = 0; k < 36; k++) {out[16 + k] = Ai[k]; out[52 + k] = Aj[k];}
  if (ed.loop != kPgNone) {
    double C[36];
    for (int k = 0; k < 36; k++) {C[k] = ed.omega[k];}
    if (!pg_chol6(C)) {*a.status = kPgLoopInformation; return;}      // (every writer writes the same kind of value: any non-zero refuses the call)
    const double sw = sqrt(w);
    const bool fi = a.fixed[ed.i] != 0, fj = a.fixed[ed.j] != 0;
    double * ji = a.loop_j + (size_t)72 * ed.loop, * jj = ji + 36;
    // (sqrt(w) C^T A)(r, c) = sqrt(w) sum_{m >= r} C(m, r) A(m, c)
    for (int r = 0; r < 6; r++) {
      for (int c = 0; c < 6; c++) {
        double si = 0.0, sj = 0.0;
        for (int m = r; m < 6; m++) {si += C[6 * m + r] * Ai[6 * m + c]; sj += C[6 * m + r] * Aj[6 * m + c];}
        ji[6 * r + c] = fi ? 0.0 : sw * si;
        jj[6 * r + c] = fj ? 0.0 : sw * sj;
      }
    }
  }
}

// One thread per prior: r, q = w Omega r, w, rho and A, the Jacobian by the node's increment (lfx.h states both kinds).
// A pose prior is the edge from the identity to its node, through pg_edge_terms; a position prior is written out here.  Not
// gated on the status word, as the edges' kernel: chi^2 and lfx_pose_graph_prior_chi2 hold whatever else was found.
__global__ __launch_bounds__(kPgWave) void pose_graph_prior_kernel(PgArgs a)
{
  const uint32_t p = blockIdx.x * kPgWave + threadIdx.x;
  if (p >= a.n_priors) {return;}
  const PgPrior & pr = a.priors[p];
  const double * pk = a.poses + 12 * (size_t)pr.node;
  double res[6], A[36], q[6], w, rho;
  if (pr.flags & kPgPriorPosition) {
    const double l[3] = {pr.lever[0], pr.lever[1], pr.lever[2]};
    const double lx[9] = {0.0, -l[2], l[1], l[2], 0.0, -l[0], -l[1], l[0], 0.0};
    for (int k = 0; k < 36; k++) {A[k] = 0.0;}
    for (int r = 0; r < 3; r++) {
      res[r] = 0.0;
      res[3 + r] = (pk[4 * r + 3] + pg_dot3(pk[4 * r], l[0], pk[4 * r + 1], l[1], pk[4 * r + 2], l[2])) - pr.z[4 * r + 3];
      for (int c = 0; c < 3; c++) {
        A[6 * (3 + r) + c] = -pg_dot3(pk[4 * r], lx[c], pk[4 * r + 1], lx[3 + c], pk[4 * r + 2], lx[6 + c]);   // -R_k [l]x
        A[6 * (3 + r) + 3 + c] = r == c ? 1.0 : 0.0;
      }
    }
  } else {
    const double identity[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    double Ai[36];
    pg_edge_terms(identity, pk, pr.z, res, Ai, A);
  }
  pg_weigh(pr.omega, res, (pr.flags & kPgPriorRobust) != 0u, a.huber_delta, q, w, rho);
  double * out = a.plin + (size_t)kPgPlin * p;
  for (int r = 0; r < 6; r++) {out[r] = res[r]; out[6 + r] = w * q[r];}
  out[12] = w; out[13] = rho; out[14] = 0.0; out[15] = 0.0;
  for (int k = 0; k < 36; k++) {out[16 + k] = A[k];}
}

// One wave per node: lanes 0 .. 35 the entries (r, c) of P's blocks (k, k) and (k + 1, k), lanes 0 .. 5 the gradient.
// block (k, k) = lambda I + A^T w Omega A of the chain edges at k; block (k + 1, k) = A_j^T w Omega A_i of the chain edge
// k -> k + 1.  A fixed node has the identity, no coupling and no gradient.
__device__ inline double pg_at_w_b(const double * A, const double * omega, double w, const double * B, int r, int c)
{
  // (A^T (w Omega) B)(r, c) = sum_m A(m, r) * (w * sum_n Omega(m, n) B(n, c))
  double acc = 0.0;
  for (int m = 0; m < 6; m++) {
    double t = 0.0;
    for (int n = 0; n < 6; n++) {t += omega[6 * m + n] * B[6 * n + c];}
    acc += A[6 * m + r] * (w * t);
  }
  return acc;
}

__global__ __launch_bounds__(kPgWave) void pose_graph_node_kernel(PgArgs a)
{
  const uint32_t k = blockIdx.x, lane = threadIdx.x;
  if (k >= a.n_nodes || *a.status != kPgOk) {return;}
  const bool fixed = a.fixed[k] != 0;
  if (lane < 36u) {
    const int r = (int)lane / 6, c = (int)lane % 6;
    double dd = r == c ? (fixed ? 1.0 : a.damping) : 0.0, oo = 0.0;
    if (!fixed) {
      const uint32_t ce = a.chain_edge[k], pe = k > 0u ? a.chain_edge[k - 1u] : kPgNone;
      if (pe != kPgNone) {                             // the chain edge k - 1 -> k: this node is its j
        const double * L = a.lin + (size_t)kPgLin * pe;
        dd += pg_at_w_b(L + 52, a.edges[pe].omega, L[12], L + 52, r, c);
      }
      if (ce != kPgNone) {                             // the chain edge k -> k + 1: this node is its i
        const double * L = a.lin + (size_t)kPgLin * ce;
        dd += pg_at_w_b(L + 16, a.edges[ce].omega, L[12], L + 16, r, c);
        if (!a.fixed[k + 1u]) {oo = pg_at_w_b(L + 52, a.edges[ce].omega, L[12], L + 16, r, c);}
      }
      if (a.n_priors) {                                // the node's priors, in prior order: the diagonal block alone
        for (uint32_t t = a.prior_begin[k]; t < a.prior_begin[k + 1u]; t++) {
          const uint32_t p = a.prior_inc[t];
          const double * L = a.plin + (size_t)kPgPlin * p;
          dd += pg_at_w_b(L + 16, a.priors[p].omega, L[12], L + 16, r, c);
        }
      }
    }
    a.diag[(size_t)36 * k + lane] = dd;
    a.off[(size_t)36 * k + lane] = oo;
  }
  if (lane < 6u) {
    double g = 0.0;
    if (!fixed) {
      for (uint32_t t = a.node_begin[k]; t < a.node_begin[k + 1u]; t++) {
        const uint32_t code = a.inc[t];
        const double * L = a.lin + (size_t)kPgLin * (code >> 1);
        const double * A = L + ((code & 1u) ? 52 : 16);
        double acc = 0.0;
        for (int m = 0; m < 6; m++) {acc += A[6 * m + lane] * L[6 + m];}
        g += acc;
      }
      if (a.n_priors) {
        for (uint32_t t = a.prior_begin[k]; t < a.prior_begin[k + 1u]; t++) {
          const double * L = a.plin + (size_t)kPgPlin * a.prior_inc[t];
          double acc = 0.0;
          for (int m = 0; m < 6; m++) {acc += L[16 + 6 * m + lane] * L[6 + m];}
          g += acc;
        }
      }
    }
    a.grad[(size_t)6 * k + lane] = g;
  }
}

// chi^2 (edges, then priors), the largest step and the count of down-weighted edges: a strided pass per thread, then a tree,
// one workgroup.  The priors' own share and count are reduced apart, by the same tree once more, where there are priors.
// Always runs: it is what carries the status word to the host.
__global__ __launch_bounds__(kPgThreads) void pose_graph_reduce_kernel(PgArgs a, uint32_t slot, int with_step)
{
  __shared__ double sum[kPgThreads], top[kPgThreads];
  __shared__ uint32_t cnt[kPgThreads];
  const uint32_t t = threadIdx.x;
  double s = 0.0, m = 0.0;
  uint32_t n = 0;
  for (uint32_t e = t; e < a.n_edges; e += kPgThreads) {
    const double * L = a.lin + (size_t)kPgLin * e;
    s += L[13];
    n += L[12] < 1.0 ? 1u : 0u;
  }
  // ... then over the priors, into the same sum; their own share and their own count beside it
  double sp = 0.0;
  uint32_t np = 0;
  for (uint32_t p = t; p < a.n_priors; p += kPgThreads) {
    const double * L = a.plin + (size_t)kPgPlin * p;
    s += L[13];
    sp += L[13];
    np += L[12] < 1.0 ? 1u : 0u;
  }
  if (with_step) {
    for (uint32_t k = t; k < a.n_nodes; k += kPgThreads) {m = pg_max(m, a.step_max[k]);}
  }
  sum[t] = s; top[t] = m; cnt[t] = n;
  __syncthreads();
  for (uint32_t h = kPgThreads / 2; h > 0; h >>= 1) {
    if (t < h) {sum[t] += sum[t + h]; top[t] = pg_max(top[t], top[t + h]); cnt[t] += cnt[t + h];}
    __syncthreads();
  }
  const double all = sum[0];
  const uint32_t edges_down = cnt[0];
  double share = 0.0;
  uint32_t down = 0;
  if (a.n_priors) {                                     // (uniform) the same tree once more, for the priors' own figures
    __syncthreads();
    sum[t] = sp; cnt[t] = np;
    __syncthreads();
    for (uint32_t h = kPgThreads / 2; h > 0; h >>= 1) {
      if (t < h) {sum[t] += sum[t + h]; cnt[t] += cnt[t + h];}
      __syncthreads();
    }
    share = sum[0]; down = cnt[0];
  }
  if (t == 0) {
    PgRecord r;
    r.chi2 = all; r.max_step = top[0]; r.status = *a.status; r.n_down = edges_down;
    r.chi2_prior = share; r.n_down_prior = down; r.spare = 0u;
    a.record[slot] = r;
  }
}

// ---------------------------------------------------------------------------------------------- 2. chain factor
// Block Cholesky of the tridiagonal P, sequential in k, one wave: S_k = D_k - M_{k-1} M_{k-1}^T (lane (r, c) one entry),
// L_k = chol(S_k) (6 x 6: every lane the same 56 operations in registers, which costs the wave what one lane costs and needs
// no exchange), M_k = O_k L_k^-T (lane (r, c) runs row r's substitution as far as c).  The next node's blocks are loaded
// while this one's are worked on.
__global__ __launch_bounds__(kPgWave) void pose_graph_chain_factor_kernel(PgArgs a)
{
  __shared__ double Sl[36], Ml[36], Ol[36];
  const uint32_t lane = threadIdx.x, N = a.n_nodes;
  if (*a.status != kPgOk || N == 0u) {return;}
  const bool on = lane < 36u;
  const int r = on ? (int)lane / 6 : 0, c = on ? (int)lane % 6 : 0;
  if (on) {Ml[lane] = 0.0;}
  double dn = on ? a.diag[lane] : 0.0, of = on ? a.off[lane] : 0.0;
  __syncthreads();
  for (uint32_t k = 0; k < N; k++) {
    const double dk = dn, ok = of;
    if (on && k + 1u < N) {dn = a.diag[(size_t)36 * (k + 1u) + lane]; of = a.off[(size_t)36 * (k + 1u) + lane];}
    if (on) {
      double s = dk;
      for (int m = 0; m < 6; m++) {s -= Ml[6 * r + m] * Ml[6 * c + m];}
      Sl[lane] = s;
      Ol[lane] = ok;
    }
    __syncthreads();
    double L[36];
    for (int i = 0; i < 6; i++) {
      for (int j = 0; j <= i; j++) {L[6 * i + j] = Sl[6 * i + j];}
    }
    const bool good = pg_chol6(L);
    if (!good) {
      if (lane == 0u) {*a.status = kPgChainPivot;}
      return;                                           // (uniform: every lane factored the same block)
    }
    double mine = 0.0, inv[6];
    for (int j = 0; j < 6; j++) {inv[j] = 1.0 / L[7 * j];}
    if (on) {
      // row r of M: M(r, j) = (O(r, j) - sum_{m < j} M(r, m) L(j, m)) / L(j, j)
      // (the whole row, every index a constant, so that it stays in registers; the lane keeps entry c)
      double row[6];
      for (int j = 0; j < 6; j++) {
        double v = Ol[6 * r + j];
        for (int m = 0; m < j; m++) {v -= row[m] * L[6 * j + m];}
        row[j] = v * inv[j];
        mine = j == c ? row[j] : mine;
      }
    }
    __syncthreads();                                    // (everyone has read Sl, Ol and the previous Ml)
    if (on) {
      Ml[lane] = mine;
      a.fac_m[(size_t)36 * k + lane] = mine;
      double keep = 0.0;
      for (int i = 0; i < 6; i++) {
        for (int j = 0; j <= i; j++) {keep = (i == r && j == c) ? (i == j ? inv[i] : L[6 * i + j]) : keep;}
      }
      a.fac_l[(size_t)36 * k + lane] = keep;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------- 3. chain solve
// P x = b for 6 L + 1 right-hand sides, one column per lane: column 0 is -g, column 1 + 6 l + c is row c of loop edge l
// (two blocks, read from loop_j, nothing of it stored as a matrix).  Forward over the nodes, then backward; the factor's
// blocks are the same for every lane, a column's entries lie side by side in y.
__global__ __launch_bounds__(kPgWave) void pose_graph_chain_solve_kernel(PgArgs a)
{
  const uint32_t col = blockIdx.x * kPgWave + threadIdx.x, N = a.n_nodes;
  if (*a.status != kPgOk || col >= 6u * a.n_loop + 1u) {return;}
  uint32_t ni = kPgNone, nj = kPgNone;
  double ji[6] = {0, 0, 0, 0, 0, 0}, jj[6] = {0, 0, 0, 0, 0, 0};
  if (col > 0u) {
    const uint32_t l = (col - 1u) / 6u, c = (col - 1u) % 6u;
    const PgEdge & ed = a.edges[a.loop_edge[l]];
    ni = ed.i; nj = ed.j;
    for (int m = 0; m < 6; m++) {ji[m] = a.loop_j[(size_t)72 * l + 6u * c + m]; jj[m] = a.loop_j[(size_t)72 * l + 36u + 6u * c + m];}
  }
  const size_t ld = a.ldy;
  double prev[6] = {0, 0, 0, 0, 0, 0};
  for (uint32_t k = 0; k < N; k++) {
    double b[6];
    if (col == 0u) {
      for (int m = 0; m < 6; m++) {b[m] = -a.grad[(size_t)6 * k + m];}
    } else {
      for (int m = 0; m < 6; m++) {b[m] = (k == ni ? ji[m] : 0.0) + (k == nj ? jj[m] : 0.0);}
    }
    if (k > 0u) {
      const double * M = a.fac_m + (size_t)36 * (k - 1u);
      for (int r = 0; r < 6; r++) {
        double acc = 0.0;
        for (int m = 0; m < 6; m++) {acc += M[6 * r + m] * prev[m];}
        b[r] -= acc;
      }
    }
    const double * L = a.fac_l + (size_t)36 * k;
    for (int r = 0; r < 6; r++) {
      double v = b[r];
      for (int m = 0; m < r; m++) {v -= L[6 * r + m] * prev[m];}
      // (prev is overwritten entry by entry: entries below r are already this node's)
      b[r] = v;
      prev[r] = v * L[7 * r];
    }
    for (int r = 0; r < 6; r++) {a.y[((size_t)6 * k + r) * ld + col] = prev[r];}
  }
  double next[6] = {0, 0, 0, 0, 0, 0};
  for (uint32_t k = N; k-- > 0u; ) {
    double b[6];
    for (int r = 0; r < 6; r++) {b[r] = a.y[((size_t)6 * k + r) * ld + col];}
    if (k + 1u < N) {
      const double * M = a.fac_m + (size_t)36 * k;      // block (k + 1, k): its transpose couples x_{k+1} into row k
      for (int m = 0; m < 6; m++) {
        double acc = 0.0;
        for (int r = 0; r < 6; r++) {acc += M[6 * r + m] * next[r];}
        b[m] -= acc;
      }
    }
    const double * L = a.fac_l + (size_t)36 * k;
    for (int r = 5; r >= 0; r--) {
      double v = b[r];
      for (int m = r + 1; m < 6; m++) {v -= L[6 * m + r] * next[m];}
      next[r] = v * L[7 * r];
    }
    for (int r = 0; r < 6; r++) {a.y[((size_t)6 * k + r) * ld + col] = next[r];}
  }
}

// ---------------------------------------------------------------------------------------------- 4. S: assemble and factor
// S(p, q) = [p == q] + Jt(p, :) Y(:, q) for q <= p, and z(p) = Jt(p, :) y0 (the column q == n of the launch).
__global__ __launch_bounds__(kPgThreads) void pose_graph_s_assemble_kernel(PgArgs a)
{
  const uint32_t n = 6u * a.n_loop;
  const uint32_t q = blockIdx.x * kPgThreads + threadIdx.x, p = blockIdx.y;
  if (*a.status != kPgOk || p >= n || q > n || (q > p && q < n)) {return;}
  const uint32_t l = p / 6u, c = p % 6u;
  const PgEdge & ed = a.edges[a.loop_edge[l]];
  const double * ji = a.loop_j + (size_t)72 * l + 6u * c, * jj = ji + 36;
  const size_t ld = a.ldy, col = q == n ? 0u : 1u + q;
  double acc = 0.0;
  for (int m = 0; m < 6; m++) {acc += ji[m] * a.y[((size_t)6 * ed.i + m) * ld + col];}
  double acc2 = 0.0;
  for (int m = 0; m < 6; m++) {acc2 += jj[m] * a.y[((size_t)6 * ed.j + m) * ld + col];}
  if (q == n) {a.z[p] = acc + acc2;} else {a.s[(size_t)p * n + q] = (p == q ? 1.0 : 0.0) + (acc + acc2);}
}

// The diagonal block [p0, p0 + nb) of S factored in LDS, right-looking, one workgroup.
__global__ __launch_bounds__(kPgThreads) void pose_graph_s_diag_kernel(PgArgs a, uint32_t p0, uint32_t nb)
{
  __shared__ double B[kPgPanel][kPgPanel + 1];
  __shared__ double pivot;
  __shared__ uint32_t bad;
  const uint32_t n = 6u * a.n_loop, t = threadIdx.x;
  if (*a.status != kPgOk) {return;}
  if (t == 0) {bad = 0u;}
  for (uint32_t i = t; i < nb * nb; i += kPgThreads) {
    const uint32_t r = i / nb, c = i % nb;
    B[r][c] = c <= r ? a.s[(size_t)(p0 + r) * n + p0 + c] : 0.0;
  }
  __syncthreads();
  for (uint32_t j = 0; j < nb; j++) {
    if (t == 0) {
      const double p = B[j][j];
      if (!(p > 0.0)) {bad = 1u;}
      pivot = sqrt(p);
      B[j][j] = pivot;
    }
    __syncthreads();
    if (bad) {
      if (t == 0) {*a.status = kPgLoopPivot;}
      return;
    }
    const double d = pivot;
    if (t > j && t < nb) {B[t][j] /= d;}
    __syncthreads();
    const uint32_t m = nb - j - 1u;                     // the trailing block's lower triangle
    for (uint32_t i = t; i < m * m; i += kPgThreads) {
      const uint32_t r = j + 1u + i / m, c = j + 1u + i % m;
      if (c <= r) {B[r][c] -= B[r][j] * B[c][j];}
    }
    __syncthreads();
  }
  for (uint32_t i = t; i < nb * nb; i += kPgThreads) {
    const uint32_t r = i / nb, c = i % nb;
    if (c <= r) {a.s[(size_t)(p0 + r) * n + p0 + c] = B[r][c];}
  }
}

// The rows below a full panel: row r's entries x solve x L_pp^T = a, one thread per row.
__global__ __launch_bounds__(kPgThreads) void pose_graph_s_panel_kernel(PgArgs a, uint32_t p0)
{
  __shared__ double Lp[kPgPanel][kPgPanel + 1];
  const uint32_t n = 6u * a.n_loop, t = threadIdx.x;
  if (*a.status != kPgOk) {return;}
  for (uint32_t i = t; i < kPgPanel * kPgPanel; i += kPgThreads) {
    const uint32_t r = i / kPgPanel, c = i % kPgPanel;
    Lp[r][c] = c <= r ? a.s[(size_t)(p0 + r) * n + p0 + c] : 0.0;
  }
  __syncthreads();
  const uint32_t row = p0 + kPgPanel + blockIdx.x * kPgThreads + t;
  if (row >= n) {return;}
  double * src = a.s + (size_t)row * n + p0;
  double x[kPgPanel];
  for (int c = 0; c < kPgPanel; c++) {x[c] = src[c];}
  for (int c = 0; c < kPgPanel; c++) {
    double v = x[c];
    for (int m = 0; m < c; m++) {v -= x[m] * Lp[c][m];}
    x[c] = v / Lp[c][c];
  }
  for (int c = 0; c < kPgPanel; c++) {src[c] = x[c];}
}

// The trailing update behind a full panel: S(r, c) -= sum_m S(r, p0 + m) S(c, p0 + m) for p0 + 48 <= c <= r, a tile of
// 16 x 16 entries per workgroup, the two strips of the panel in LDS.  Tiles above the diagonal return.
__global__ __launch_bounds__(kPgThreads) void pose_graph_s_update_kernel(PgArgs a, uint32_t p0)
{
  __shared__ double Rr[kPgTile][kPgPanel + 1], Cc[kPgTile][kPgPanel + 1];
  const uint32_t n = 6u * a.n_loop, t = threadIdx.x, base = p0 + kPgPanel;
  if (*a.status != kPgOk || blockIdx.x > blockIdx.y) {return;}
  const uint32_t r0 = base + blockIdx.y * kPgTile, c0 = base + blockIdx.x * kPgTile;
  for (uint32_t i = t; i < kPgTile * kPgPanel; i += kPgThreads) {
    const uint32_t rr = i / kPgPanel, m = i % kPgPanel;
    Rr[rr][m] = r0 + rr < n ? a.s[(size_t)(r0 + rr) * n + p0 + m] : 0.0;
    Cc[rr][m] = c0 + rr < n ? a.s[(size_t)(c0 + rr) * n + p0 + m] : 0.0;
  }
  __syncthreads();
  const uint32_t tr = t / kPgTile, tc = t % kPgTile, r = r0 + tr, c = c0 + tc;
  if (r >= n || c > r) {return;}
  double acc = 0.0;
  for (int m = 0; m < kPgPanel; m++) {acc += Rr[tr][m] * Cc[tc][m];}
  a.s[(size_t)r * n + c] -= acc;
}

// z = S^-1 z through the factor, blocks of 64, one workgroup: a block's own triangle is solved by the first wave with the
// running entries in registers and each solved entry passed on by a shuffle; the rest of z is then updated by everyone.
__global__ __launch_bounds__(kPgThreads) void pose_graph_s_solve_kernel(PgArgs a)
{
  __shared__ double zb[kPgWave];
  const uint32_t n = 6u * a.n_loop, t = threadIdx.x;
  if (*a.status != kPgOk) {return;}
  const double * S = a.s;
  for (uint32_t s0 = 0; s0 < n; s0 += kPgWave) {       // L w = z
    const uint32_t nb = n - s0 < (uint32_t)kPgWave ? n - s0 : (uint32_t)kPgWave;
    if (t < (uint32_t)kPgWave) {
      const bool in = t < nb;
      const size_t row = (size_t)(s0 + (in ? t : 0u)) * n + s0;
      double acc = in ? a.z[s0 + t] : 0.0;
      const double inv = in ? 1.0 / S[row + t] : 0.0;
      for (uint32_t j = 0; j < nb; j++) {
        const double zj = __shfl(acc * inv, (int)j, kPgWave);
        if (t == j) {zb[j] = zj;}
        if (in && t > j) {acc -= S[row + j] * zj;}
      }
    }
    __syncthreads();
    if (t < nb) {a.z[s0 + t] = zb[t];}
    for (uint32_t r = s0 + nb + t; r < n; r += kPgThreads) {
      const double * L = S + (size_t)r * n + s0;
      double acc = 0.0;
      for (uint32_t j = 0; j < nb; j++) {acc += L[j] * zb[j];}
      a.z[r] -= acc;
    }
    __syncthreads();
  }
  const uint32_t blocks = (n + kPgWave - 1u) / kPgWave;
  for (uint32_t bi = blocks; bi-- > 0u; ) {            // L^T x = w
    const uint32_t s0 = bi * kPgWave, nb = n - s0 < (uint32_t)kPgWave ? n - s0 : (uint32_t)kPgWave;
    if (t < (uint32_t)kPgWave) {
      const bool in = t < nb;
      double acc = in ? a.z[s0 + t] : 0.0;
      const double inv = in ? 1.0 / S[(size_t)(s0 + t) * n + s0 + t] : 0.0;
      for (uint32_t j = nb; j-- > 0u; ) {
        const double xj = __shfl(acc * inv, (int)j, kPgWave);
        if (t == j) {zb[j] = xj;}
        if (in && t < j) {acc -= S[(size_t)(s0 + j) * n + s0 + t] * xj;}
      }
    }
    __syncthreads();
    if (t < nb) {a.z[s0 + t] = zb[t];}
    for (uint32_t k = t; k < s0; k += kPgThreads) {
      double acc = 0.0;
      for (uint32_t j = 0; j < nb; j++) {acc += S[(size_t)(s0 + j) * n + k] * zb[j];}
      a.z[k] -= acc;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------- 5. step and retract
// One workgroup per node: delta = y0 - Y z (a strided pass per thread over the columns, then a tree), then the node's pose
// is moved: R <- R Exp(a), t <- t + b, and R is brought back to the orthonormal matrices by one step of the polar
// iteration, R <- R (3 I - R^T R) / 2, which squares its distance from them.
__global__ __launch_bounds__(kPgThreads) void pose_graph_step_kernel(PgArgs a)
{
  __shared__ double part[6][kPgThreads];
  const uint32_t k = blockIdx.x, t = threadIdx.x, n = 6u * a.n_loop, T = blockDim.x;
  if (*a.status != kPgOk || k >= a.n_nodes) {return;}
  const size_t ld = a.ldy;
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (uint32_t q = t; q < n; q += T) {
    const double zq = a.z[q];
    for (int r = 0; r < 6; r++) {acc[r] += a.y[((size_t)6 * k + r) * ld + 1u + q] * zq;}
  }
  for (int r = 0; r < 6; r++) {part[r][t] = acc[r];}
  __syncthreads();
  for (uint32_t h = T / 2; h > 0; h >>= 1) {
    if (t < h) {
      for (int r = 0; r < 6; r++) {part[r][t] += part[r][t + h];}
    }
    __syncthreads();
  }
  if (t != 0) {return;}
  double d[6], top = 0.0;
  for (int r = 0; r < 6; r++) {
    d[r] = a.y[((size_t)6 * k + r) * ld] - part[r][0];
    top = pg_max(top, fabs(d[r]));
  }
  if (a.fixed[k]) {a.step_max[k] = 0.0; return;}
  a.step_max[k] = top;
  // a step of exactly zero (a node no edge touches) moves nothing: the polar step below would still round the rotation
  // again, and the pose would not come back as it went in
  if (top == 0.0) {return;}
  double * p = a.poses + 12 * (size_t)k;
  const double th2 = pg_dot3(d[0], d[0], d[1], d[1], d[2], d[2]), th = sqrt(th2);
  // Exp(a) = I + A [a]x + B [a]x^2
  const double A = th < 1e-4 ? 1.0 - th2 / 6.0 : sin(th) / th;
  const double B = th < 1e-4 ? 0.5 - th2 / 24.0 : (1.0 - cos(th)) / th2;
  const double ax[9] = {0.0, -d[2], d[1], d[2], 0.0, -d[0], -d[1], d[0], 0.0};
  double E[9], R[9], Q[9], G[9];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) {
      const double a2 = pg_dot3(ax[3 * r], ax[c], ax[3 * r + 1], ax[3 + c], ax[3 * r + 2], ax[6 + c]);
      E[3 * r + c] = ((r == c ? 1.0 : 0.0) + A * ax[3 * r + c]) + B * a2;
    }
  }
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) {R[3 * r + c] = pg_dot3(p[4 * r], E[c], p[4 * r + 1], E[3 + c], p[4 * r + 2], E[6 + c]);}
  }
  pg_tmul3(R, R, G);
  for (int i = 0; i < 9; i++) {G[i] = (i % 4 == 0 ? 1.5 : 0.0) - 0.5 * G[i];}
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) {Q[3 * r + c] = pg_dot3(R[3 * r], G[c], R[3 * r + 1], G[3 + c], R[3 * r + 2], G[6 + c]);}
  }
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) {p[4 * r + c] = Q[3 * r + c];}
    p[4 * r + 3] += d[3 + r];
  }
}

// ---------------------------------------------------------------------------------------------- 6. covariances
// Sigma = (H + lambda I)^-1 = P^-1 - V V^T with V = Y L_S^-T (Woodbury on H = P + Jt^T Jt, S = I + Jt Y = L_S L_S^T), from
// the factor, Y and L_S that kernels 2 to 4 leave (lfx_posegraph.hip runs them once more, on the final linearisation).
// What is new: the selected inverse of the chain factor, the rows of Y solved against L_S in place, and the 6 x 6 products.
// The same rules as above: no atomic, every sum in a fixed order, every kernel returns at once when the status word is set.
struct PgMargArgs
{
  double * ginv;                         // [N][36]: G_k = (P^-1)(k, k), exactly symmetric
  double * tblk;                         // [N][36]: T_k = -L_k^-T M_k^T, so that (P^-1)(k, m) = T_k (P^-1)(k + 1, m) for m > k
  double * cov;                          // [N][36]: Sigma_kk
  const uint32_t * pairs;                // [n][2]: i < j
  double * cross;                        // [n][36]: Sigma_ij
};

constexpr int kPgRows = 64;              // the rows of Y one workgroup of the solve takes
constexpr int kPgCols = 32;              // the columns of one pass of its trailing update
constexpr int kPgPairs = 64;             // the pairs of one launch of the joint kernel

// The selected inverse of P = (L, M)(L, M)^T, backward over the nodes, one wave, lane (r, c) one entry as in the factor:
//   G_{N-1} = L^-T L^-1,  T_k = -L_k^-T M_k^T,  G_k = L_k^-T L_k^-1 + T_k G_{k+1} T_k^T
// L_k^-1 is every lane's own 6 x 6 triangular inverse in registers (fac_l's diagonal already holds 1 / L(r, r)); the
// products go through LDS.  Lane (r, c) and lane (c, r) evaluate the same expression, so G is symmetric bit for bit.  The
// blocks of node k - 1 are loaded while node k's are worked on.
__global__ __launch_bounds__(kPgWave) void pose_graph_chain_inverse_kernel(PgArgs a, PgMargArgs g)
{
  __shared__ double Ll[36], Ml[36], Il[36], Tl[36], Gl[36], Xl[36];
  const uint32_t lane = threadIdx.x, N = a.n_nodes;
  if (*a.status != kPgOk || N == 0u) {return;}
  const bool on = lane < 36u;
  const int r = on ? (int)lane / 6 : 0, c = on ? (int)lane % 6 : 0;
  const int hi = r > c ? r : c, lo = r > c ? c : r;
  double ln = on ? a.fac_l[(size_t)36 * (N - 1u) + lane] : 0.0, mn = on ? a.fac_m[(size_t)36 * (N - 1u) + lane] : 0.0;
  for (uint32_t k = N; k-- > 0u; ) {
    const bool last = k + 1u == N;
    if (on) {Ll[lane] = ln; Ml[lane] = mn;}
    if (on && k > 0u) {ln = a.fac_l[(size_t)36 * (k - 1u) + lane]; mn = a.fac_m[(size_t)36 * (k - 1u) + lane];}
    __syncthreads();
    double L[36], I[36];
    for (int i = 0; i < 6; i++) {
      for (int j = 0; j <= i; j++) {L[6 * i + j] = Ll[6 * i + j];}
    }
    // L^-1, column by column: I(j, j) = 1 / L(j, j), I(i, j) = -(sum_{j <= m < i} L(i, m) I(m, j)) / L(i, i)
    double mine = 0.0;
    for (int j = 0; j < 6; j++) {
      I[7 * j] = L[7 * j];
      for (int i = j + 1; i < 6; i++) {
        double v = 0.0;
        for (int m = j; m < i; m++) {v += L[6 * i + m] * I[6 * m + j];}
        I[6 * i + j] = -v * L[7 * i];
      }
      for (int i = j; i < 6; i++) {mine = (i == r && j == c) ? I[6 * i + j] : mine;}
    }
    if (on) {Il[lane] = mine;}                        // (zero above the diagonal)
    __syncthreads();
    double t = 0.0, w = 0.0;
    if (on) {
      // T(r, c) = -sum_{m >= r} L^-1(m, r) M(c, m);  W(hi, lo) = sum_{m >= hi} L^-1(m, hi) L^-1(m, lo)
      if (!last) {
        for (int m = r; m < 6; m++) {t += Il[6 * m + r] * Ml[6 * c + m];}
        t = -t;
      }
      for (int m = hi; m < 6; m++) {w += Il[6 * m + hi] * Il[6 * m + lo];}
      Tl[lane] = t;
    }
    __syncthreads();
    if (on && !last) {                                  // X = T G_{k+1}
      double x = 0.0;
      for (int m = 0; m < 6; m++) {x += Tl[6 * r + m] * Gl[6 * m + c];}
      Xl[lane] = x;
    }
    __syncthreads();
    if (on) {
      double v = w;
      if (!last) {
        double u = 0.0;
        for (int m = 0; m < 6; m++) {u += Xl[6 * hi + m] * Tl[6 * lo + m];}
        v = w + u;
      }
      g.ginv[(size_t)36 * k + lane] = v;
      g.tblk[(size_t)36 * k + lane] = t;
      Gl[lane] = v;                                     // (everyone read G_{k+1} before the barrier above)
    }
    __syncthreads();
  }
}

// V = Y(:, 1 .. 6 L) L_S^-T in place: every row v of Y solves v L_S^T = y, a forward substitution of length 6 L that no other
// row takes part in.  A workgroup takes kPgRows rows and walks L_S in panels of kPgPanel columns: the tile's panel columns
// and the panel's diagonal block go to LDS, one thread per row solves its 48 entries there (rows per lane, in LDS, where a
// row stride of 49 doubles keeps 32 lanes on 32 bank pairs); then the trailing update of the tile's remaining columns,
// kPgCols at a pass, with COLUMNS per lane: consecutive lanes read and write consecutive doubles of one row of Y, whose rows
// start one double past a multiple of eight and so can be walked along, not across.  An entry's sums have one
// order whatever the tile it falls in.
__global__ __launch_bounds__(kPgThreads) void pose_graph_y_solve_kernel(PgArgs a)
{
  __shared__ double V[kPgRows][kPgPanel + 1], Lp[kPgPanel][kPgPanel + 1], Ls[kPgCols][kPgPanel + 1];
  const uint32_t n = 6u * a.n_loop, rows = 6u * a.n_nodes, t = threadIdx.x, row0 = blockIdx.x * kPgRows;
  if (*a.status != kPgOk || row0 >= rows) {return;}
  const size_t ld = a.ldy;
  for (uint32_t p0 = 0; p0 < n; p0 += kPgPanel) {
    const uint32_t nb = n - p0 < (uint32_t)kPgPanel ? n - p0 : (uint32_t)kPgPanel;
    for (uint32_t i = t; i < kPgRows * kPgPanel; i += kPgThreads) {
      const uint32_t rr = i / kPgPanel, m = i % kPgPanel;
      V[rr][m] = (row0 + rr < rows && m < nb) ? a.y[(size_t)(row0 + rr) * ld + 1u + p0 + m] : 0.0;
    }
    for (uint32_t i = t; i < kPgPanel * kPgPanel; i += kPgThreads) {
      const uint32_t rr = i / kPgPanel, m = i % kPgPanel;
      Lp[rr][m] = (rr < nb && m <= rr) ? a.s[(size_t)(p0 + rr) * n + p0 + m] : (rr == m ? 1.0 : 0.0);
    }
    __syncthreads();
    if (t < (uint32_t)kPgRows) {
      double x[kPgPanel];
      for (int cc = 0; cc < kPgPanel; cc++) {x[cc] = V[t][cc];}
      for (int cc = 0; cc < kPgPanel; cc++) {
        double v = x[cc];
        for (int m = 0; m < cc; m++) {v -= x[m] * Lp[cc][m];}
        x[cc] = v / Lp[cc][cc];
      }
      for (int cc = 0; cc < kPgPanel; cc++) {V[t][cc] = x[cc];}
    }
    __syncthreads();
    for (uint32_t i = t; i < kPgRows * kPgPanel; i += kPgThreads) {
      const uint32_t rr = i / kPgPanel, m = i % kPgPanel;
      if (row0 + rr < rows && m < nb) {a.y[(size_t)(row0 + rr) * ld + 1u + p0 + m] = V[rr][m];}
    }
    // y(row, c) -= sum_m v(row, p0 + m) L_S(c, p0 + m) for c >= p0 + 48 (there are such columns behind a full panel only)
    const uint32_t tc = t % kPgCols, tr = t / kPgCols;
    for (uint32_t c0 = p0 + kPgPanel; c0 < n; c0 += kPgCols) {
      __syncthreads();                                  // (the previous pass has read Ls)
      for (uint32_t i = t; i < kPgCols * kPgPanel; i += kPgThreads) {
        const uint32_t cc = i / kPgPanel, m = i % kPgPanel;
        Ls[cc][m] = c0 + cc < n ? a.s[(size_t)(c0 + cc) * n + p0 + m] : 0.0;
      }
      __syncthreads();
      constexpr int kPer = kPgRows / (kPgThreads / kPgCols);   // 8 rows per thread, kPgThreads / kPgCols apart
      double acc[kPer];
      for (int q = 0; q < kPer; q++) {acc[q] = 0.0;}
      for (int m = 0; m < kPgPanel; m++) {
        const double l = Ls[tc][m];
        for (int q = 0; q < kPer; q++) {acc[q] += V[tr + (kPgThreads / kPgCols) * q][m] * l;}
      }
      if (c0 + tc < n) {
        for (int q = 0; q < kPer; q++) {
          const uint32_t row = row0 + tr + (kPgThreads / kPgCols) * q;
          if (row < rows) {a.y[(size_t)row * ld + 1u + c0 + tc] -= acc[q];}
        }
      }
    }
    __syncthreads();                                    // (V, Lp and Ls are rewritten by the next panel)
  }
}

// One workgroup per node: Sigma_kk = G_k - V_k V_k^T, V_k the node's six solved rows.  21 dot products of length 6 L, a
// strided pass per thread and a tree, then the lower triangle mirrored.  Zeros for a fixed node.
__global__ __launch_bounds__(kPgThreads) void pose_graph_marginal_kernel(PgArgs a, PgMargArgs g)
{
  __shared__ double part[21][kPgThreads];
  const uint32_t k = blockIdx.x, t = threadIdx.x, n = 6u * a.n_loop, T = blockDim.x;
  if (*a.status != kPgOk || k >= a.n_nodes) {return;}
  const size_t ld = a.ldy;
  double acc[21];
  for (int i = 0; i < 21; i++) {acc[i] = 0.0;}
  for (uint32_t q = t; q < n; q += T) {
    double v[6];
    for (int r = 0; r < 6; r++) {v[r] = a.y[((size_t)6 * k + r) * ld + 1u + q];}
    int i = 0;
    for (int r = 0; r < 6; r++) {
      for (int c = 0; c <= r; c++) {acc[i++] += v[r] * v[c];}
    }
  }
  for (int i = 0; i < 21; i++) {part[i][t] = acc[i];}
  __syncthreads();
  for (uint32_t h = T / 2; h > 0; h >>= 1) {
    if (t < h) {
      for (int i = 0; i < 21; i++) {part[i][t] += part[i][t + h];}
    }
    __syncthreads();
  }
  if (t >= 36u) {return;}
  const uint32_t r = t / 6u, c = t % 6u, hi = r > c ? r : c, lo = r > c ? c : r;
  const double v = g.ginv[(size_t)36 * k + 6u * hi + lo] - part[hi * (hi + 1u) / 2u + lo][0];
  g.cov[(size_t)36 * k + t] = a.fixed[k] ? 0.0 : v;
}

// One wave per pair (i, j), i < j: Sigma_ij = (T_i T_{i+1} ... T_{j-1}) G_j - V_i V_j^T.  The product runs from the right,
// X <- T_k X for k = j - 1 down to i, one 6 x 6 product per node between the two, lane (r, c) one entry.  The 36 dot products
// of length 6 L: a strided pass per lane (lane t the columns t, t + 64, ...: six rows of each node read along), then a tree.
// Zeros where either node is fixed.
__global__ __launch_bounds__(kPgWave) void pose_graph_joint_kernel(PgArgs a, PgMargArgs g, uint32_t n_pairs)
{
  __shared__ double part[36][kPgWave];
  __shared__ double Xl[36], Tl[36];
  const uint32_t p = blockIdx.x, lane = threadIdx.x, n = 6u * a.n_loop;
  if (*a.status != kPgOk || p >= n_pairs) {return;}
  const uint32_t i = g.pairs[2u * p], j = g.pairs[2u * p + 1u];
  if (i >= j || j >= a.n_nodes) {return;}              // (the host sends sorted pairs of nodes; nothing else is walked)
  const bool on = lane < 36u;
  const int r = on ? (int)lane / 6 : 0, c = on ? (int)lane % 6 : 0;
  if (a.fixed[i] || a.fixed[j]) {
    if (on) {g.cross[(size_t)36 * p + lane] = 0.0;}
    return;
  }
  const size_t ld = a.ldy;
  double acc[36];
  for (int m = 0; m < 36; m++) {acc[m] = 0.0;}
  for (uint32_t q = lane; q < n; q += kPgWave) {
    double vi[6], vj[6];
    for (int m = 0; m < 6; m++) {vi[m] = a.y[((size_t)6 * i + m) * ld + 1u + q]; vj[m] = a.y[((size_t)6 * j + m) * ld + 1u + q];}
    for (int rr = 0; rr < 6; rr++) {
      for (int cc = 0; cc < 6; cc++) {acc[6 * rr + cc] += vi[rr] * vj[cc];}
    }
  }
  for (int m = 0; m < 36; m++) {part[m][lane] = acc[m];}
  if (on) {Xl[lane] = g.ginv[(size_t)36 * j + lane];}
  __syncthreads();
  for (uint32_t h = kPgWave / 2; h > 0; h >>= 1) {
    if (lane < h) {
      for (int m = 0; m < 36; m++) {part[m][lane] += part[m][lane + h];}
    }
    __syncthreads();
  }
  double tn = on ? g.tblk[(size_t)36 * (j - 1u) + lane] : 0.0;
  for (uint32_t k = j; k-- > i; ) {
    if (on) {Tl[lane] = tn;}
    if (on && k > i) {tn = g.tblk[(size_t)36 * (k - 1u) + lane];}
    __syncthreads();
    double x = 0.0;
    if (on) {
      for (int m = 0; m < 6; m++) {x += Tl[6 * r + m] * Xl[6 * m + c];}
    }
    __syncthreads();                                    // (everyone has read Xl)
    if (on) {Xl[lane] = x;}
    __syncthreads();
  }
  if (on) {g.cross[(size_t)36 * p + lane] = Xl[lane] - part[lane][0];}
}

}  // namespace lfx
