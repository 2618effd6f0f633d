// lfx_posegraph.hip -- the pose graph (include/lfx.h, the pose graph section; lfx_kernels_posegraph.hpp): nodes and edges
// kept on the device, Gauss-Newton over them with the chain-and-loop solver.  The host keeps what it needs to check a call
// before anything is queued (the edges' ends, which nodes are fixed) and builds the node -> (edge, side) incidence lists,
// stable by edge id, whenever edges were added, and the node -> prior lists beside them.  Everything is allocated by
// lfx_pose_graph_create, but the priors' four blocks: lfx_pose_graph_reserve_priors (the config's ABI is closed), and the
// covariances' six: lfx_pose_graph_reserve_marginals.  The covariances (lfx_pose_graph_marginals, _joint_covariances) are
// computed once after an optimise, from the linearisation it leaves, and kept until the graph is next written.
#include "lfx_internal.hpp"
#include "lfx_kernels_posegraph.hpp"

#include <algorithm>
#include <cstdint>

using namespace lfx_host;

static_assert(sizeof(lfx::PgEdge) == sizeof(lfx_pose_graph_edge) && sizeof(lfx::PgEdge) == 400, "an edge goes up as the caller wrote it, but for one word");
static_assert(lfx::kPgEdgeRobust == LFX_EDGE_ROBUST, "the kernels' flag is the header's");
static_assert(sizeof(lfx_pose_graph_prior) == 416 && sizeof(lfx::PgPrior) == 416, "a prior goes up as the caller wrote it");
static_assert(lfx::kPgPriorRobust == LFX_PRIOR_ROBUST && lfx::kPgPriorPosition == LFX_PRIOR_POSITION, "the kernels' flags are the header's");

struct lfx_pose_graph
{
  int device = 0;
  lfx_pose_graph_config cfg{};
  uint32_t n_nodes = 0, n_edges = 0, n_chain = 0, n_loop = 0, ldy_cap = 0;
  uint32_t n_priors = 0, max_priors = 0;  // max_priors: what lfx_pose_graph_reserve_priors allocated (0: nothing yet)
  uint32_t prior_down = 0;               // of the last optimise: the priors with w < 1 and their share of chi2_final
  double prior_chi2 = 0.0;
  bool released = false, first_fixed = false;   // lfx_pose_graph_release_first; what set_fixed(0, .) asked last
  uint64_t device_bytes = 0;
  // the host's copy of the topology
  std::vector<uint32_t> edge_i, edge_j, edge_loop, chain_edge, prior_node;
  std::vector<uint8_t> fixed;
  bool topology_stale = true;            // edges or nodes were added since the lists went up
  bool linearised = false;               // lin holds the edges' values at the poses the last optimise left
  // what goes up: rewritten only once the graph's last queued call has passed
  std::vector<lfx::PgEdge> stage_edges;
  std::vector<uint32_t> stage_lists, stage_prior_lists;
  std::vector<lfx::PgPrior> stage_priors;
  mutable std::vector<double> stage_lin;
  DevBuf<double> poses, backup, lin, loop_j, grad, diag, off, fac_l, fac_m, y, s, z, step_max;
  DevBuf<uint8_t> d_fixed;
  DevBuf<lfx::PgEdge> edges;
  DevBuf<uint32_t> node_begin, inc, d_chain_edge, loop_edge, status;
  DevBuf<lfx::PgPrior> priors;           // these four by lfx_pose_graph_reserve_priors
  DevBuf<double> plin;
  DevBuf<uint32_t> prior_begin, prior_inc;
  DevBuf<lfx::PgRecord> record;
  // the covariances (lfx_pose_graph_reserve_marginals allocates them): G_k, T_k, Sigma_kk, a status word of their own, and
  // one launch's pairs with their cross blocks
  DevBuf<double> ginv, tblk, cov, cross;
  DevBuf<uint32_t> pairs, mstatus;
  bool marg_reserved = false;
  bool marg_current = false;             // cov holds every node's block of the last optimise's linearisation (marg_code says how it went)
  bool fixed_stale = false;              // set_fixed or release_first since the last linearisation: H on the device is another graph's
  int32_t marg_code = 0;
  std::vector<double> stage_cov, stage_cross;
  std::vector<uint32_t> stage_pairs;
  PinnedBuf h_record;
  PinnedBuf h_poses;                     // poses on their way up ([max_nodes][12]): pinned, so that the copy is queued and the call returns
  Tail tail;                             // behind the last call that touched the graph: order_behind before a call's own
                                         // work, done after it; settle before the host's staging vectors are rewritten
};

namespace
{

struct Timed : TimedSpan                 // whenever profiling is on: the sampling interval counts batches, and there are none here
{
  Timed(lfx_ctx * c, KernelSlot k, hipStream_t s)
  : TimedSpan(c, c->profiling, k, s) {}
};

int check_graph(lfx_ctx * c, const lfx_pose_graph * g) {return check_device(c, g->device, "the pose graph");}

uint32_t ldy_of(uint32_t n_loop) {return (6u * n_loop + 1u + 7u) & ~7u;}

lfx::PgArgs args_of(lfx_pose_graph * g)
{
  lfx::PgArgs a{};
  a.poses = g->poses.p; a.fixed = g->d_fixed.p; a.edges = g->edges.p; a.lin = g->lin.p; a.loop_j = g->loop_j.p;
  a.node_begin = g->node_begin.p; a.inc = g->inc.p; a.chain_edge = g->d_chain_edge.p; a.loop_edge = g->loop_edge.p;
  a.grad = g->grad.p; a.diag = g->diag.p; a.off = g->off.p; a.fac_l = g->fac_l.p; a.fac_m = g->fac_m.p;
  a.y = g->y.p; a.s = g->s.p; a.z = g->z.p; a.step_max = g->step_max.p; a.status = g->status.p; a.record = g->record.p;
  a.n_nodes = g->n_nodes; a.n_edges = g->n_edges; a.n_loop = g->n_loop; a.ldy = ldy_of(g->n_loop);
  a.huber_delta = g->cfg.huber_delta; a.damping = g->cfg.damping;
  a.priors = g->priors.p; a.plin = g->plin.p; a.prior_begin = g->prior_begin.p; a.prior_inc = g->prior_inc.p; a.n_priors = g->n_priors;
  return a;
}

// the lists the kernels walk: node_begin [N + 1], inc [2 E], chain_edge [N], loop_edge [L], one block
int upload_topology(Call & call, lfx_pose_graph * g)
{
  lfx_ctx * c = call.c;
  hipStream_t st = call.st;
  const uint32_t N = g->n_nodes, E = g->n_edges, L = g->n_loop;
  LFX_TRY(call.after(g->tail));
  std::vector<uint32_t> & w = g->stage_lists;
  w.assign((size_t)N + 1u + 2u * (size_t)E + N + L, 0u);
  uint32_t * begin = w.data(), * inc = begin + N + 1u, * chain = inc + 2u * (size_t)E, * loops = chain + N;
  for (uint32_t e = 0; e < E; e++) {begin[g->edge_i[e] + 1u]++; begin[g->edge_j[e] + 1u]++;}
  for (uint32_t k = 0; k < N; k++) {begin[k + 1u] += begin[k];}
  std::vector<uint32_t> at(begin, begin + N);
  for (uint32_t e = 0; e < E; e++) {              // ascending e: every node's list is in edge order
    inc[at[g->edge_i[e]]++] = 2u * e;
    inc[at[g->edge_j[e]]++] = 2u * e + 1u;
    if (g->edge_loop[e] != lfx::kPgNone) {loops[g->edge_loop[e]] = e;}
  }
  for (uint32_t k = 0; k < N; k++) {chain[k] = g->chain_edge[k];}
  LFX_HIP(c, hipMemcpyAsync(g->node_begin.p, begin, sizeof(uint32_t) * ((size_t)N + 1u), hipMemcpyHostToDevice, st));
  if (E) {LFX_HIP(c, hipMemcpyAsync(g->inc.p, inc, sizeof(uint32_t) * 2u * (size_t)E, hipMemcpyHostToDevice, st));}
  LFX_HIP(c, hipMemcpyAsync(g->d_chain_edge.p, chain, sizeof(uint32_t) * N, hipMemcpyHostToDevice, st));
  if (L) {LFX_HIP(c, hipMemcpyAsync(g->loop_edge.p, loops, sizeof(uint32_t) * L, hipMemcpyHostToDevice, st));}
  if (const uint32_t P = g->n_priors) {           // prior_begin [N + 1], prior_inc [P]: every node's list in prior order
    std::vector<uint32_t> & v = g->stage_prior_lists;
    v.assign((size_t)N + 1u + P, 0u);
    uint32_t * pb = v.data(), * pi = pb + N + 1u;
    for (uint32_t p = 0; p < P; p++) {pb[g->prior_node[p] + 1u]++;}
    for (uint32_t k = 0; k < N; k++) {pb[k + 1u] += pb[k];}
    std::vector<uint32_t> pat(pb, pb + N);
    for (uint32_t p = 0; p < P; p++) {pi[pat[g->prior_node[p]]++] = p;}
    LFX_HIP(c, hipMemcpyAsync(g->prior_begin.p, pb, sizeof(uint32_t) * ((size_t)N + 1u), hipMemcpyHostToDevice, st));
    LFX_HIP(c, hipMemcpyAsync(g->prior_inc.p, pi, sizeof(uint32_t) * P, hipMemcpyHostToDevice, st));
  }
  g->topology_stale = false;
  return LFX_OK;
}

// r, w, rho and the Jacobians of every edge, the gradient and P's blocks, chi^2 into record[slot]
int launch_linearize(lfx_ctx * c, const lfx::PgArgs & a, uint32_t slot, bool with_step, hipStream_t st)
{
  {
    Timed t(c, kSlotPgLinearize, st);             // (the priors' kernel inside the edges' span: the slots stay as they are)
    if (a.n_edges) {
      hipLaunchKernelGGL(lfx::pose_graph_linearize_kernel, dim3((a.n_edges + lfx::kPgWave - 1u) / lfx::kPgWave), dim3(lfx::kPgWave), 0, st, a);
    }
    if (a.n_priors) {
      hipLaunchKernelGGL(lfx::pose_graph_prior_kernel, dim3((a.n_priors + lfx::kPgWave - 1u) / lfx::kPgWave), dim3(lfx::kPgWave), 0, st, a);
    }
  }
  LFX_HIP(c, hipGetLastError());
  {
    Timed t(c, kSlotPgNode, st);
    hipLaunchKernelGGL(lfx::pose_graph_node_kernel, dim3(a.n_nodes), dim3(lfx::kPgWave), 0, st, a);
  }
  LFX_HIP(c, hipGetLastError());
  {
    Timed t(c, kSlotPgReduce, st);
    hipLaunchKernelGGL(lfx::pose_graph_reduce_kernel, dim3(1), dim3(lfx::kPgThreads), 0, st, a, slot, with_step ? 1 : 0);
  }
  LFX_HIP(c, hipGetLastError());
  return LFX_OK;
}

// one Gauss-Newton step from the linearisation that is on the device: factor P, solve, S, the step, the poses moved
int launch_step(lfx_ctx * c, const lfx::PgArgs & a, hipStream_t st)
{
  const uint32_t n = 6u * a.n_loop, P = lfx::kPgPanel;
  {
    Timed t(c, kSlotPgChainFactor, st);
    hipLaunchKernelGGL(lfx::pose_graph_chain_factor_kernel, dim3(1), dim3(lfx::kPgWave), 0, st, a);
  }
  LFX_HIP(c, hipGetLastError());
  {
    Timed t(c, kSlotPgChainSolve, st);
    hipLaunchKernelGGL(lfx::pose_graph_chain_solve_kernel, dim3((n + 1u + lfx::kPgWave - 1u) / lfx::kPgWave), dim3(lfx::kPgWave), 0, st, a);
  }
  LFX_HIP(c, hipGetLastError());
  if (n) {
    {
      Timed t(c, kSlotPgAssemble, st);
      hipLaunchKernelGGL(lfx::pose_graph_s_assemble_kernel, dim3((n + 1u + lfx::kPgThreads - 1u) / lfx::kPgThreads, n), dim3(lfx::kPgThreads), 0, st, a);
    }
    LFX_HIP(c, hipGetLastError());
    // blocked right-looking Cholesky, a sequence of launches: the number of panels is known here
    for (uint32_t p0 = 0; p0 < n; p0 += P) {
      const uint32_t nb = std::min(P, n - p0);
      {
        Timed t(c, kSlotPgDiag, st);
        hipLaunchKernelGGL(lfx::pose_graph_s_diag_kernel, dim3(1), dim3(lfx::kPgThreads), 0, st, a, p0, nb);
      }
      LFX_HIP(c, hipGetLastError());
      if (p0 + P >= n) {break;}                        // (nothing below a last panel, full or not)
      const uint32_t below = n - (p0 + P);
      {
        Timed t(c, kSlotPgPanel, st);
        hipLaunchKernelGGL(lfx::pose_graph_s_panel_kernel, dim3((below + lfx::kPgThreads - 1u) / lfx::kPgThreads), dim3(lfx::kPgThreads), 0, st, a, p0);
      }
      LFX_HIP(c, hipGetLastError());
      const uint32_t tiles = (below + lfx::kPgTile - 1u) / lfx::kPgTile;
      {
        Timed t(c, kSlotPgUpdate, st);
        hipLaunchKernelGGL(lfx::pose_graph_s_update_kernel, dim3(tiles, tiles), dim3(lfx::kPgThreads), 0, st, a, p0);
      }
      LFX_HIP(c, hipGetLastError());
    }
    {
      Timed t(c, kSlotPgSolve, st);
      hipLaunchKernelGGL(lfx::pose_graph_s_solve_kernel, dim3(1), dim3(lfx::kPgThreads), 0, st, a);
    }
    LFX_HIP(c, hipGetLastError());
  }
  {
    Timed t(c, kSlotPgStep, st);
    hipLaunchKernelGGL(lfx::pose_graph_step_kernel, dim3(a.n_nodes), dim3(n > 64u ? lfx::kPgThreads : lfx::kPgWave), 0, st, a);
  }
  LFX_HIP(c, hipGetLastError());
  return LFX_OK;
}

int check_config(lfx_ctx * c, const lfx_pose_graph_config * f)
{
  if (f->max_nodes < 1u || f->max_edges < 1u) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "max_nodes and max_edges must be >= 1");}
  if (f->max_loop_edges > LFX_POSE_GRAPH_MAX_LOOP_EDGES) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "max_loop_edges must be <= 10000");}
  if (f->max_iter < 1u || f->max_iter > 1000u) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "max_iter must be in 1 .. 1000");}
  if (!std::isfinite(f->damping) || f->damping < 0.0 || !std::isfinite(f->tolerance) || f->tolerance < 0.0 || !std::isfinite(f->huber_delta) ||
    !(f->huber_delta > 0.0))
  {
    return fail(c, LFX_ERR_INVALID_ARGUMENT, "damping and tolerance must be finite and >= 0, huber_delta finite and > 0");
  }
  return LFX_OK;
}

// the edges' values at the poses on the device (after a refused or diverged call put the initial poses back)
int relinearize(lfx_ctx * c, lfx_pose_graph * g, const lfx::PgArgs & a, hipStream_t st)
{
  LFX_HIP(c, hipMemsetAsync(g->status.p, 0, sizeof(uint32_t), st));
  return launch_linearize(c, a, 0u, false, st);
}

// The front half of launch_step once more, on the linearisation that is on the device, for the covariances: factor P, solve
// for Y, assemble and factor S -- no solve for z and no step, so the poses are never touched (y0 and z are scratch here).
// A launcher of its own: launch_step stays as it is, and so do the bytes an optimise computes.
int launch_factor(lfx_ctx * c, const lfx::PgArgs & a, hipStream_t st)
{
  const uint32_t n = 6u * a.n_loop, P = lfx::kPgPanel;
  hipLaunchKernelGGL(lfx::pose_graph_chain_factor_kernel, dim3(1), dim3(lfx::kPgWave), 0, st, a);
  LFX_HIP(c, hipGetLastError());
  hipLaunchKernelGGL(lfx::pose_graph_chain_solve_kernel, dim3((n + 1u + lfx::kPgWave - 1u) / lfx::kPgWave), dim3(lfx::kPgWave), 0, st, a);
  LFX_HIP(c, hipGetLastError());
  if (n == 0u) {return LFX_OK;}
  hipLaunchKernelGGL(lfx::pose_graph_s_assemble_kernel, dim3((n + 1u + lfx::kPgThreads - 1u) / lfx::kPgThreads, n), dim3(lfx::kPgThreads), 0, st, a);
  LFX_HIP(c, hipGetLastError());
  for (uint32_t p0 = 0; p0 < n; p0 += P) {
    hipLaunchKernelGGL(lfx::pose_graph_s_diag_kernel, dim3(1), dim3(lfx::kPgThreads), 0, st, a, p0, std::min(P, n - p0));
    LFX_HIP(c, hipGetLastError());
    if (p0 + P >= n) {break;}
    const uint32_t below = n - (p0 + P), tiles = (below + lfx::kPgTile - 1u) / lfx::kPgTile;
    hipLaunchKernelGGL(lfx::pose_graph_s_panel_kernel, dim3((below + lfx::kPgThreads - 1u) / lfx::kPgThreads), dim3(lfx::kPgThreads), 0, st, a, p0);
    LFX_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(lfx::pose_graph_s_update_kernel, dim3(tiles, tiles), dim3(lfx::kPgThreads), 0, st, a, p0);
    LFX_HIP(c, hipGetLastError());
  }
  return LFX_OK;
}

lfx::PgMargArgs marg_args_of(lfx_pose_graph * g)
{
  lfx::PgMargArgs m{};
  m.ginv = g->ginv.p; m.tblk = g->tblk.p; m.cov = g->cov.p; m.pairs = g->pairs.p; m.cross = g->cross.p;
  return m;
}

// what lfx_pose_graph_marginals and lfx_pose_graph_joint_covariances both refuse
int check_marginals(lfx_ctx * c, const lfx_pose_graph * g)
{
  if (!g->marg_reserved) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "lfx_pose_graph_reserve_marginals has not been called");}
  if (!g->linearised || g->fixed_stale) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the graph has changed since the last lfx_pose_graph_optimize");}
  return LFX_OK;
}

// Every node's Sigma_kk on the device (cov), G_k, T_k and V beside it for the joint blocks: the whole graph's work, once per
// optimise.  Synchronous: the status word comes back.  The kernels run on the covariances' own status word.
int ensure_marginals(Call & k, lfx_pose_graph * g)
{
  if (g->marg_current) {return k.read(g->tail);}
  lfx_ctx * c = k.c;
  hipStream_t st = k.st;
  LFX_TRY(k.behind(g->tail));
  lfx::PgArgs a = args_of(g);
  a.status = g->mstatus.p;
  const lfx::PgMargArgs m = marg_args_of(g);
  const uint32_t n = 6u * a.n_loop;
  LFX_HIP(c, hipMemsetAsync(g->mstatus.p, 0, sizeof(uint32_t), st));
  LFX_TRY(launch_factor(c, a, st));
  hipLaunchKernelGGL(lfx::pose_graph_chain_inverse_kernel, dim3(1), dim3(lfx::kPgWave), 0, st, a, m);
  LFX_HIP(c, hipGetLastError());
  if (n) {
    hipLaunchKernelGGL(lfx::pose_graph_y_solve_kernel, dim3((6u * a.n_nodes + lfx::kPgRows - 1u) / lfx::kPgRows), dim3(lfx::kPgThreads), 0, st, a);
    LFX_HIP(c, hipGetLastError());
  }
  hipLaunchKernelGGL(lfx::pose_graph_marginal_kernel, dim3(a.n_nodes), dim3(n > 64u ? lfx::kPgThreads : lfx::kPgWave), 0, st, a, m);
  LFX_HIP(c, hipGetLastError());
  LFX_TRY(read_block(c, g->h_record, g->mstatus.p, sizeof(uint32_t), st));
  g->marg_code = *reinterpret_cast<const uint32_t *>(g->h_record.p) == lfx::kPgOk ? LFX_POSE_GRAPH_CONVERGED : LFX_POSE_GRAPH_NOT_POSITIVE_DEFINITE;
  g->marg_current = true;
  return k.finish();
}

}  // namespace

extern "C" {

void lfx_pose_graph_default_config(lfx_pose_graph_config * config)
{
  if (!config) {return;}
  *config = lfx_pose_graph_config{};
  config->max_loop_edges = 512u;
  config->max_iter = 10u;
  config->damping = 1e-6;
  config->tolerance = 1e-9;
  config->huber_delta = 3.0;
}

int lfx_pose_graph_create(lfx_ctx * c, const lfx_pose_graph_config * config, lfx_pose_graph ** out)
{
  if (!c) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!config || !out) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "config and out are required");}
  LFX_TRY(check_config(c, config));
  LFX_HIP(c, hipSetDevice(c->device));
  lfx_pose_graph * g = new (std::nothrow) lfx_pose_graph();
  if (!g) {return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the pose graph");}
  g->device = c->device;
  g->cfg = *config;
  const size_t N = config->max_nodes, E = config->max_edges, L = config->max_loop_edges, n = 6u * L;
  g->ldy_cap = ldy_of(config->max_loop_edges);
  auto give_up = [&](int code, const std::string & why) {(void)hipGetLastError(); lfx_pose_graph_destroy(g); return fail(c, code, why);};
  DevTotal m;
  m.get(g->poses, 12u * N); m.get(g->backup, 12u * N); m.get(g->d_fixed, N); m.get(g->edges, E); m.get(g->lin, (size_t)lfx::kPgLin * E);
  m.get(g->loop_j, 72u * std::max<size_t>(L, 1u)); m.get(g->node_begin, N + 1u); m.get(g->inc, 2u * E); m.get(g->d_chain_edge, N);
  m.get(g->loop_edge, std::max<size_t>(L, 1u)); m.get(g->grad, 6u * N); m.get(g->diag, 36u * N); m.get(g->off, 36u * N); m.get(g->fac_l, 36u * N);
  m.get(g->fac_m, 36u * N); m.get(g->y, 6u * N * g->ldy_cap); m.get(g->s, std::max<size_t>(n * n, 1u)); m.get(g->z, std::max<size_t>(n, 1u));
  m.get(g->step_max, N); m.get(g->status, 1u); m.get(g->record, (size_t)config->max_iter + 2u);
  if (!m.ok) {return give_up(LFX_ERR_OUT_OF_MEMORY, m.refusal("the pose graph"));}
  g->device_bytes = m.bytes;
  if (g->h_record.reserve(sizeof(lfx::PgRecord) * ((size_t)config->max_iter + 2u)) != hipSuccess) {
    return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the pose graph's status record");
  }
  if (g->h_poses.reserve(sizeof(double) * 12u * N) != hipSuccess) {
    return give_up(LFX_ERR_OUT_OF_MEMORY, "cannot allocate the pose graph's staging block");
  }
  g->edge_i.reserve(E); g->edge_j.reserve(E); g->edge_loop.reserve(E);
  g->chain_edge.reserve(N); g->fixed.reserve(N);
  *out = g;
  return LFX_OK;
}

void lfx_pose_graph_destroy(lfx_pose_graph * g) {destroy_on(g);}

int lfx_pose_graph_info(const lfx_pose_graph * g, lfx_pose_graph_info_t * info)
{
  if (!g || !info) {return LFX_ERR_INVALID_ARGUMENT;}
  info->n_nodes = g->n_nodes; info->n_edges = g->n_edges; info->n_chain = g->n_chain; info->n_loop = g->n_loop;
  info->device_bytes = g->device_bytes;
  return LFX_OK;
}

int lfx_pose_graph_add_nodes(lfx_ctx * c, lfx_pose_graph * g, const double * poses, uint32_t n, uint32_t * first_id, void * stream)
{
  if (!c || !g || (n && !poses)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_graph(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!finite_all(poses, 12u * (size_t)n)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "a pose that is not finite");}
  if (n > g->cfg.max_nodes - g->n_nodes) {
    return fail(c, LFX_ERR_CAPACITY, "the pose graph holds " + std::to_string(g->n_nodes) + " of " + std::to_string(g->cfg.max_nodes) +
             " nodes: no room for " + std::to_string(n) + " more");
  }
  if (first_id) {*first_id = g->n_nodes;}
  if (n == 0) {return LFX_OK;}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.after(g->tail));
  const uint32_t first = g->n_nodes;
  g->fixed.resize((size_t)first + n, 0);
  g->chain_edge.resize((size_t)first + n, lfx::kPgNone);
  if (first == 0u) {g->fixed[0] = (!g->released || g->first_fixed) ? 1 : 0;}
  LFX_TRY(send_block(c, g->h_poses, g->poses.p + 12u * (size_t)first, poses, sizeof(double) * 12u * n, k.st));
  LFX_HIP(c, hipMemcpyAsync(g->d_fixed.p + first, g->fixed.data() + first, n, hipMemcpyHostToDevice, k.st));
  g->n_nodes += n;
  g->topology_stale = true;
  g->linearised = false;
  g->marg_current = false;
  return k.finish();
}

int lfx_pose_graph_set_fixed(lfx_ctx * c, lfx_pose_graph * g, uint32_t node, int fixed, void * stream)
{
  if (!c || !g) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_graph(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (node >= g->n_nodes) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "node " + std::to_string(node) + " is not in the graph");}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.after(g->tail));
  if (node == 0u) {g->first_fixed = fixed != 0;}
  g->marg_current = false;
  g->fixed_stale = true;
  g->fixed[node] = ((node == 0u && !g->released) || fixed) ? 1 : 0;
  LFX_HIP(c, hipMemcpyAsync(g->d_fixed.p + node, g->fixed.data() + node, 1, hipMemcpyHostToDevice, k.st));
  return k.finish();
}

int lfx_pose_graph_add_edges(lfx_ctx * c, lfx_pose_graph * g, const lfx_pose_graph_edge * edges, uint32_t n, void * stream)
{
  if (!c || !g || (n && !edges)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_graph(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  // every edge is checked, and the chain / loop split of the call worked out, before anything is touched
  std::vector<uint32_t> loop_of(n, lfx::kPgNone);
  std::vector<uint8_t> chain_new(n ? g->n_nodes : 0u, 0);  // nodes whose chain edge is one of this call's
  uint32_t loops = 0;
  for (uint32_t k = 0; k < n; k++) {
    const lfx_pose_graph_edge & e = edges[k];
    const std::string which = "edge " + std::to_string(k) + " of the call: ";
    if (e.i >= g->n_nodes || e.j >= g->n_nodes) {return fail(c, LFX_ERR_INVALID_ARGUMENT, which + "an end that is not a node of the graph");}
    if (e.i == e.j) {return fail(c, LFX_ERR_INVALID_ARGUMENT, which + "i == j");}
    if (e.flags & ~LFX_EDGE_ROBUST) {return fail(c, LFX_ERR_INVALID_ARGUMENT, which + "unknown flags");}
    if (!finite_all(e.z, 12) || !finite_all(e.information, 36)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, which + "a value that is not finite");}
    double top = 0.0;
    for (int i = 0; i < 36; i++) {top = std::max(top, std::fabs(e.information[i]));}
    for (int r = 0; r < 6; r++) {
      for (int q = 0; q < r; q++) {
        if (std::fabs(e.information[6 * r + q] - e.information[6 * q + r]) > 1e-9 * top) {
          return fail(c, LFX_ERR_INVALID_ARGUMENT, which + "the information matrix is not symmetric");
        }
      }
    }
    const bool chain = e.j == e.i + 1u && g->chain_edge[e.i] == lfx::kPgNone && !chain_new[e.i];
    if (chain) {chain_new[e.i] = 1;} else {loop_of[k] = g->n_loop + loops++;}
  }
  if (n > g->cfg.max_edges - g->n_edges) {
    return fail(c, LFX_ERR_CAPACITY, "the pose graph holds " + std::to_string(g->n_edges) + " of " + std::to_string(g->cfg.max_edges) +
             " edges: no room for " + std::to_string(n) + " more");
  }
  if (loops > g->cfg.max_loop_edges - g->n_loop) {
    return fail(c, LFX_ERR_CAPACITY, "the pose graph holds " + std::to_string(g->n_loop) + " of " + std::to_string(g->cfg.max_loop_edges) +
             " loop edges: no room for " + std::to_string(loops) + " more");
  }
  if (n == 0) {return LFX_OK;}
  Call call(c, stream);
  LFX_TRY(call.open());
  LFX_TRY(call.after(g->tail));
  g->stage_edges.resize(n);
  for (uint32_t k = 0; k < n; k++) {
    lfx::PgEdge & d = g->stage_edges[k];
    d.i = edges[k].i; d.j = edges[k].j; d.flags = edges[k].flags; d.loop = loop_of[k];
    std::memcpy(d.z, edges[k].z, sizeof(d.z));
    std::memcpy(d.omega, edges[k].information, sizeof(d.omega));
  }
  LFX_HIP(c, hipMemcpyAsync(g->edges.p + g->n_edges, g->stage_edges.data(), sizeof(lfx::PgEdge) * n, hipMemcpyHostToDevice, call.st));
  for (uint32_t k = 0; k < n; k++) {
    g->edge_i.push_back(edges[k].i); g->edge_j.push_back(edges[k].j); g->edge_loop.push_back(loop_of[k]);
    if (loop_of[k] == lfx::kPgNone) {g->chain_edge[edges[k].i] = g->n_edges + k; g->n_chain++;}
  }
  g->n_edges += n;
  g->n_loop += loops;
  g->topology_stale = true;
  g->linearised = false;
  g->marg_current = false;
  return call.finish();
}

int lfx_pose_graph_optimize(lfx_ctx * c, lfx_pose_graph * g, lfx_pose_graph_result * result, void * stream)
{
  if (!c || !g || !result) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_graph(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (g->n_edges == 0u && g->n_priors == 0u) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the pose graph has no edges");}
  Call k(c, stream);
  hipStream_t st = k.st;
  LFX_TRY(k.open());
  if (g->topology_stale) {LFX_TRY(upload_topology(k, g));}
  LFX_TRY(k.behind(g->tail));
  const lfx::PgArgs a = args_of(g);
  g->marg_current = false;
  const size_t pose_bytes = sizeof(double) * 12u * g->n_nodes;
  LFX_HIP(c, hipMemcpyAsync(g->backup.p, g->poses.p, pose_bytes, hipMemcpyDeviceToDevice, st));
  LFX_HIP(c, hipMemsetAsync(g->status.p, 0, sizeof(uint32_t), st));
  LFX_TRY(launch_linearize(c, a, 0u, false, st));
  const lfx::PgRecord * rec = reinterpret_cast<const lfx::PgRecord *>(g->h_record.p);
  uint32_t it = 0;
  bool converged = false, refused = false;
  while (it < g->cfg.max_iter) {
    it++;
    LFX_TRY(launch_step(c, a, st));
    LFX_TRY(launch_linearize(c, a, it, true, st));
    // the iteration's only wait: its record (chi^2 at the new poses, the largest step, the status word)
    LFX_TRY(read_block(c, g->h_record, g->record.p, sizeof(lfx::PgRecord) * ((size_t)it + 1u), st));
    if (rec[it].status != lfx::kPgOk) {refused = true; break;}
    if (rec[it].max_step < g->cfg.tolerance) {converged = true; break;}
    if (!(rec[it].max_step == rec[it].max_step)) {break;}          // (not a number: nothing more to learn)
  }
  *result = lfx_pose_graph_result{};
  result->n_chain = g->n_chain;
  result->n_loop = g->n_loop;
  result->chi2_initial = rec[0].chi2;
  const double first = rec[0].chi2, last = rec[it].chi2;
  const bool diverged = !refused && (!(last == last) || !(rec[it].max_step == rec[it].max_step) || last > first + 1e-12 * std::max(1.0, first));
  if (refused || diverged) {
    LFX_HIP(c, hipMemcpyAsync(g->poses.p, g->backup.p, pose_bytes, hipMemcpyDeviceToDevice, st));
    LFX_TRY(relinearize(c, g, a, st));
    LFX_TRY(read_block(c, g->h_record, g->record.p, sizeof(lfx::PgRecord), st));
    result->code = refused ? LFX_POSE_GRAPH_NOT_POSITIVE_DEFINITE : LFX_POSE_GRAPH_DIVERGED;
    result->iterations = refused ? (int32_t)it - 1 : (int32_t)it;
    result->chi2_final = first;
    result->max_step = refused ? 0.0 : rec[it].max_step;
    result->n_robust_downweighted = rec[0].n_down;
    g->prior_down = rec[0].n_down_prior; g->prior_chi2 = rec[0].chi2_prior;
  } else {
    result->code = converged ? LFX_POSE_GRAPH_CONVERGED : LFX_POSE_GRAPH_MAX_ITERATIONS;
    result->iterations = (int32_t)it;
    result->chi2_final = last;
    result->max_step = rec[it].max_step;
    result->n_robust_downweighted = rec[it].n_down;
    g->prior_down = rec[it].n_down_prior; g->prior_chi2 = rec[it].chi2_prior;
  }
  g->linearised = true;
  g->fixed_stale = false;
  return k.finish();
}

int lfx_pose_graph_poses(lfx_ctx * c, const lfx_pose_graph * g, uint32_t first, uint32_t count, double * poses_out, void * stream)
{
  if (!c || !g || (count && !poses_out)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_graph(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (first > g->n_nodes || count > g->n_nodes - first) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "nodes outside the pose graph");}
  if (count == 0) {return LFX_OK;}
  Call k(c, stream);
  return poses_get(k, g->tail, g->poses, first, count, poses_out);
}

int lfx_pose_graph_set_poses(lfx_ctx * c, lfx_pose_graph * g, uint32_t first, uint32_t count, const double * poses, void * stream)
{
  if (!c || !g || (count && !poses)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_graph(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (first > g->n_nodes || count > g->n_nodes - first) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "nodes outside the pose graph");}
  if (!finite_all(poses, 12u * (size_t)count)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "a pose that is not finite");}
  if (count == 0) {return LFX_OK;}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.after(g->tail));
  LFX_TRY(send_block(c, g->h_poses, g->poses.p + 12u * (size_t)first, poses, sizeof(double) * 12u * count, k.st));
  g->linearised = false;
  g->marg_current = false;
  return k.finish();
}

int lfx_pose_graph_view(lfx_ctx * c, const lfx_pose_graph * g, const double ** d_poses, uint32_t * n_nodes, void * stream)
{
  if (!c || !g || !d_poses || !n_nodes) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_graph(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.read(g->tail));
  *d_poses = g->poses.p;
  *n_nodes = g->n_nodes;
  return LFX_OK;
}

int lfx_pose_graph_edge_chi2(lfx_ctx * c, const lfx_pose_graph * g, uint32_t first, uint32_t count, double * rho, double * w, void * stream)
{
  if (!c || !g) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_graph(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (first > g->n_edges || count > g->n_edges - first) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "edges outside the pose graph");}
  if (!g->linearised) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the graph has changed since the last lfx_pose_graph_optimize");}
  if (count == 0) {return LFX_OK;}
  Call k(c, stream);
  hipStream_t st = k.st;
  LFX_TRY(k.open());
  LFX_TRY(k.wait(g->tail));              // (the staging vector is the graph's)
  g->stage_lin.resize((size_t)lfx::kPgLin * count);
  LFX_HIP(c, hipMemcpyAsync(g->stage_lin.data(), g->lin.p + (size_t)lfx::kPgLin * first, sizeof(double) * lfx::kPgLin * count, hipMemcpyDeviceToHost, st));
  LFX_HIP(c, hipStreamSynchronize(st));
  for (uint32_t e = 0; e < count; e++) {
    if (w) {w[e] = g->stage_lin[(size_t)lfx::kPgLin * e + 12u];}
    if (rho) {rho[e] = g->stage_lin[(size_t)lfx::kPgLin * e + 13u];}
  }
  return LFX_OK;
}

int lfx_pose_graph_reserve_priors(lfx_ctx * c, lfx_pose_graph * g, uint32_t max_priors)
{
  if (!c || !g) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_graph(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (max_priors == 0u) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "max_priors must be >= 1");}
  if (g->max_priors != 0u) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the pose graph's priors are reserved already");}
  LFX_HIP(c, hipSetDevice(c->device));
  const size_t P = max_priors, N = g->cfg.max_nodes;
  DevBuf<lfx::PgPrior> priors;
  DevBuf<double> plin;
  DevBuf<uint32_t> begin, inc;
  const uint64_t bytes = (uint64_t)P * sizeof(lfx::PgPrior) + (uint64_t)P * lfx::kPgPlin * sizeof(double) + (uint64_t)(N + 1u + P) * sizeof(uint32_t);
  if (priors.alloc(P) != hipSuccess || plin.alloc((size_t)lfx::kPgPlin * P) != hipSuccess || begin.alloc(N + 1u) != hipSuccess ||
    inc.alloc(P) != hipSuccess)
  {
    (void)hipGetLastError();
    return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the priors' " + std::to_string(bytes) + " bytes");     // (the four free themselves)
  }
  g->priors = std::move(priors); g->plin = std::move(plin); g->prior_begin = std::move(begin); g->prior_inc = std::move(inc);
  g->prior_node.reserve(P);
  g->max_priors = max_priors;
  g->device_bytes += bytes;
  return LFX_OK;
}

int lfx_pose_graph_add_priors(lfx_ctx * c, lfx_pose_graph * g, const lfx_pose_graph_prior * priors, uint32_t n, void * stream)
{
  if (!c || !g || (n && !priors)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_graph(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  for (uint32_t k = 0; k < n; k++) {                // every prior is checked before anything is touched
    const lfx_pose_graph_prior & p = priors[k];
    const std::string which = "prior " + std::to_string(k) + " of the call: ";
    if (p.node >= g->n_nodes) {return fail(c, LFX_ERR_INVALID_ARGUMENT, which + "a node that is not in the graph");}
    if (p.flags & ~(LFX_PRIOR_ROBUST | LFX_PRIOR_POSITION)) {return fail(c, LFX_ERR_INVALID_ARGUMENT, which + "unknown flags");}
    if (!finite_all(p.z, 12) || !finite_all(p.information, 36) || !finite_all(p.lever, 3)) {
      return fail(c, LFX_ERR_INVALID_ARGUMENT, which + "a value that is not finite");
    }
    double top = 0.0;
    for (int i = 0; i < 36; i++) {top = std::max(top, std::fabs(p.information[i]));}
    for (int r = 0; r < 6; r++) {
      for (int q = 0; q < r; q++) {
        if (std::fabs(p.information[6 * r + q] - p.information[6 * q + r]) > 1e-9 * top) {
          return fail(c, LFX_ERR_INVALID_ARGUMENT, which + "the information matrix is not symmetric");
        }
      }
    }
    if (p.flags & LFX_PRIOR_POSITION) {
      for (int i = 0; i < 36; i++) {
        if ((i / 6 < 3 || i % 6 < 3) && p.information[i] != 0.0) {
          return fail(c, LFX_ERR_INVALID_ARGUMENT, which + "a position prior with information outside its lower right 3 x 3 block");
        }
      }
    } else if (p.lever[0] != 0.0 || p.lever[1] != 0.0 || p.lever[2] != 0.0) {
      return fail(c, LFX_ERR_INVALID_ARGUMENT, which + "a pose prior with a lever");
    }
  }
  if (n > g->max_priors - g->n_priors) {
    return fail(c, LFX_ERR_CAPACITY, "the pose graph holds " + std::to_string(g->n_priors) + " of " + std::to_string(g->max_priors) +
             " priors (lfx_pose_graph_reserve_priors): no room for " + std::to_string(n) + " more");
  }
  if (n == 0) {return LFX_OK;}
  Call call(c, stream);
  LFX_TRY(call.open());
  LFX_TRY(call.after(g->tail));
  g->stage_priors.resize(n);
  for (uint32_t k = 0; k < n; k++) {
    lfx::PgPrior & d = g->stage_priors[k];
    d.node = priors[k].node; d.flags = priors[k].flags;
    std::memcpy(d.z, priors[k].z, sizeof(d.z));
    std::memcpy(d.omega, priors[k].information, sizeof(d.omega));
    std::memcpy(d.lever, priors[k].lever, sizeof(d.lever));
  }
  LFX_HIP(c, hipMemcpyAsync(g->priors.p + g->n_priors, g->stage_priors.data(), sizeof(lfx::PgPrior) * n, hipMemcpyHostToDevice, call.st));
  for (uint32_t k = 0; k < n; k++) {g->prior_node.push_back(priors[k].node);}
  g->n_priors += n;
  g->topology_stale = true;
  g->linearised = false;
  g->marg_current = false;
  return call.finish();
}

int lfx_pose_graph_release_first(lfx_ctx * c, lfx_pose_graph * g, int released, void * stream)
{
  if (!c || !g) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_graph(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  g->released = released != 0;
  g->marg_current = false;
  g->fixed_stale = true;
  if (g->n_nodes == 0u) {return LFX_OK;}            // (lfx_pose_graph_add_nodes writes node 0's flag)
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(k.after(g->tail));
  g->fixed[0] = (!g->released || g->first_fixed) ? 1 : 0;
  LFX_HIP(c, hipMemcpyAsync(g->d_fixed.p, g->fixed.data(), 1, hipMemcpyHostToDevice, k.st));
  return k.finish();
}

int lfx_pose_graph_prior_chi2(lfx_ctx * c, const lfx_pose_graph * g, uint32_t first, uint32_t count, double * rho, double * w, void * stream)
{
  if (!c || !g) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_graph(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (first > g->n_priors || count > g->n_priors - first) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "priors outside the pose graph");}
  if (!g->linearised) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the graph has changed since the last lfx_pose_graph_optimize");}
  if (count == 0) {return LFX_OK;}
  Call k(c, stream);
  hipStream_t st = k.st;
  LFX_TRY(k.open());
  LFX_TRY(k.wait(g->tail));              // (the staging vector is the graph's)
  g->stage_lin.resize((size_t)lfx::kPgPlin * count);
  LFX_HIP(c, hipMemcpyAsync(g->stage_lin.data(), g->plin.p + (size_t)lfx::kPgPlin * first, sizeof(double) * lfx::kPgPlin * count, hipMemcpyDeviceToHost, st));
  LFX_HIP(c, hipStreamSynchronize(st));
  for (uint32_t p = 0; p < count; p++) {
    if (w) {w[p] = g->stage_lin[(size_t)lfx::kPgPlin * p + 12u];}
    if (rho) {rho[p] = g->stage_lin[(size_t)lfx::kPgPlin * p + 13u];}
  }
  return LFX_OK;
}

int lfx_pose_graph_prior_info(const lfx_pose_graph * g, lfx_pose_graph_prior_info_t * info)
{
  if (!g || !info) {return LFX_ERR_INVALID_ARGUMENT;}
  info->n_priors = g->n_priors; info->max_priors = g->max_priors; info->n_downweighted = g->prior_down; info->reserved = 0u;
  info->chi2 = g->prior_chi2;
  return LFX_OK;
}

int lfx_pose_graph_reserve_marginals(lfx_ctx * c, lfx_pose_graph * g)
{
  if (!c || !g) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_graph(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (g->marg_reserved) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "the pose graph's covariances are reserved already");}
  LFX_HIP(c, hipSetDevice(c->device));
  const size_t N = g->cfg.max_nodes, K = lfx::kPgPairs;
  DevBuf<double> ginv, tblk, cov, cross;
  DevBuf<uint32_t> pairs, status;
  const uint64_t bytes = (uint64_t)(3u * 36u * N + 36u * K) * sizeof(double) + (uint64_t)(2u * K + 1u) * sizeof(uint32_t);
  if (ginv.alloc(36u * N) != hipSuccess || tblk.alloc(36u * N) != hipSuccess || cov.alloc(36u * N) != hipSuccess ||
    cross.alloc(36u * K) != hipSuccess || pairs.alloc(2u * K) != hipSuccess || status.alloc(1u) != hipSuccess)
  {
    (void)hipGetLastError();
    return fail(c, LFX_ERR_OUT_OF_MEMORY, "cannot allocate the covariances' " + std::to_string(bytes) + " bytes");     // (the six free themselves)
  }
  g->ginv = std::move(ginv); g->tblk = std::move(tblk); g->cov = std::move(cov); g->cross = std::move(cross);
  g->pairs = std::move(pairs); g->mstatus = std::move(status);
  g->marg_reserved = true;
  g->marg_current = false;
  g->device_bytes += bytes;
  return LFX_OK;
}

int lfx_pose_graph_marginals(lfx_ctx * c, lfx_pose_graph * g, uint32_t first, uint32_t count, double * cov_out, int32_t * code, void * stream)
{
  if (!c || !g || !code || (count && !cov_out)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_graph(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  LFX_TRY(check_marginals(c, g));
  if (first > g->n_nodes || count > g->n_nodes - first) {return fail(c, LFX_ERR_INVALID_ARGUMENT, "nodes outside the pose graph");}
  Call k(c, stream);
  LFX_TRY(k.open());
  LFX_TRY(ensure_marginals(k, g));
  *code = g->marg_code;
  if (g->marg_code != LFX_POSE_GRAPH_CONVERGED || count == 0u) {return LFX_OK;}
  LFX_HIP(c, hipMemcpyAsync(cov_out, g->cov.p + 36u * (size_t)first, sizeof(double) * 36u * count, hipMemcpyDeviceToHost, k.st));
  LFX_HIP(c, hipStreamSynchronize(k.st));
  return LFX_OK;
}

int lfx_pose_graph_joint_covariances(lfx_ctx * c, lfx_pose_graph * g, const uint32_t * pairs, uint32_t n, double * out, int32_t * code, void * stream)
{
  if (!c || !g || !code || (n && (!pairs || !out))) {return LFX_ERR_INVALID_ARGUMENT;}
  if (check_graph(c, g) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  LFX_TRY(check_marginals(c, g));
  for (uint32_t p = 0; p < n; p++) {                  // every pair is checked before anything is queued or written
    const uint32_t i = pairs[2u * p], j = pairs[2u * p + 1u];
    const std::string which = "pair " + std::to_string(p) + " of the call: ";
    if (i >= g->n_nodes || j >= g->n_nodes) {return fail(c, LFX_ERR_INVALID_ARGUMENT, which + "an id that is not a node of the graph");}
    if (i == j) {return fail(c, LFX_ERR_INVALID_ARGUMENT, which + "i == j");}
  }
  Call k(c, stream);
  hipStream_t st = k.st;
  LFX_TRY(k.open());
  LFX_TRY(ensure_marginals(k, g));
  *code = g->marg_code;
  if (g->marg_code != LFX_POSE_GRAPH_CONVERGED || n == 0u) {return LFX_OK;}
  LFX_TRY(k.wait(g->tail));                           // (the staging vectors below are the graph's)
  lfx::PgArgs a = args_of(g);
  a.status = g->mstatus.p;
  const lfx::PgMargArgs m = marg_args_of(g);
  g->stage_cov.resize((size_t)36 * g->n_nodes);
  LFX_HIP(c, hipMemcpyAsync(g->stage_cov.data(), g->cov.p, sizeof(double) * g->stage_cov.size(), hipMemcpyDeviceToHost, st));
  g->stage_pairs.resize(2u * (size_t)lfx::kPgPairs);
  g->stage_cross.resize(36u * (size_t)lfx::kPgPairs);
  for (uint32_t p0 = 0; p0 < n; p0 += lfx::kPgPairs) {
    const uint32_t np = std::min<uint32_t>(lfx::kPgPairs, n - p0);
    for (uint32_t p = 0; p < np; p++) {
      const uint32_t i = pairs[2u * (p0 + p)], j = pairs[2u * (p0 + p) + 1u];
      g->stage_pairs[2u * p] = std::min(i, j); g->stage_pairs[2u * p + 1u] = std::max(i, j);
    }
    LFX_HIP(c, hipMemcpyAsync(g->pairs.p, g->stage_pairs.data(), sizeof(uint32_t) * 2u * np, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(lfx::pose_graph_joint_kernel, dim3(np), dim3(lfx::kPgWave), 0, st, a, m, np);
    LFX_HIP(c, hipGetLastError());
    LFX_HIP(c, hipMemcpyAsync(g->stage_cross.data(), g->cross.p, sizeof(double) * 36u * np, hipMemcpyDeviceToHost, st));
    LFX_HIP(c, hipStreamSynchronize(st));
    for (uint32_t p = 0; p < np; p++) {
      const uint32_t i = pairs[2u * (p0 + p)], j = pairs[2u * (p0 + p) + 1u];
      const double * x = g->stage_cross.data() + 36u * (size_t)p;      // Sigma(min, max)
      const double * di = g->stage_cov.data() + 36u * (size_t)i, * dj = g->stage_cov.data() + 36u * (size_t)j;
      double * o = out + 144u * (size_t)(p0 + p);
      for (int r = 0; r < 6; r++) {
        for (int q = 0; q < 6; q++) {
          const double ij = i < j ? x[6 * r + q] : x[6 * q + r];       // Sigma_ij(r, q)
          o[12 * r + q] = di[6 * r + q];
          o[12 * r + 6 + q] = ij;
          o[12 * (6 + q) + r] = ij;
          o[12 * (6 + r) + 6 + q] = dj[6 * r + q];
        }
      }
    }
  }
  return LFX_OK;
}

#ifdef LFX_TEST_HOOKS
// Test infrastructure (the test-hooks build only): the graph linearised where it stands -- per edge r [E][6] (may be NULL),
// per node the gradient [N][6], chi^2 -- and lfx_pose_graph_edge_chi2 opened for those values.
int lfx_test_pose_graph_linearize(lfx_ctx * c, lfx_pose_graph * g, double * r_out, double * grad_out, double * chi2_out, void * stream)
{
  if (!c || !g || !grad_out || !chi2_out || g->n_edges == 0u) {return LFX_ERR_INVALID_ARGUMENT;}
  Call k(c, stream);
  hipStream_t st = k.st;
  LFX_TRY(k.open());
  if (g->topology_stale) {LFX_TRY(upload_topology(k, g));}
  LFX_TRY(k.behind(g->tail));
  const lfx::PgArgs a = args_of(g);
  LFX_TRY(relinearize(c, g, a, st));
  std::vector<double> lin((size_t)lfx::kPgLin * g->n_edges);
  LFX_HIP(c, hipMemcpyAsync(lin.data(), g->lin.p, sizeof(double) * lin.size(), hipMemcpyDeviceToHost, st));
  LFX_HIP(c, hipMemcpyAsync(grad_out, g->grad.p, sizeof(double) * 6u * g->n_nodes, hipMemcpyDeviceToHost, st));
  LFX_HIP(c, hipMemcpyAsync(g->h_record.p, g->record.p, sizeof(lfx::PgRecord), hipMemcpyDeviceToHost, st));
  LFX_HIP(c, hipStreamSynchronize(st));
  for (uint32_t e = 0; r_out && e < g->n_edges; e++) {std::memcpy(r_out + 6u * (size_t)e, lin.data() + (size_t)lfx::kPgLin * e, sizeof(double) * 6u);}
  *chi2_out = reinterpret_cast<const lfx::PgRecord *>(g->h_record.p)->chi2;
  g->linearised = true;
  g->marg_current = false;
  g->fixed_stale = false;
  return k.finish();
}

// ... and the same for a graph with priors (edges or none): per prior r [P][6] (may be NULL), per node the gradient of edges
// and priors [N][6], chi^2 of both; lfx_pose_graph_prior_chi2 and lfx_pose_graph_edge_chi2 opened for those values.
int lfx_test_pose_graph_prior_linearize(lfx_ctx * c, lfx_pose_graph * g, double * r_out, double * grad_out, double * chi2_out, void * stream)
{
  if (!c || !g || !grad_out || !chi2_out || g->n_priors == 0u) {return LFX_ERR_INVALID_ARGUMENT;}
  Call k(c, stream);
  hipStream_t st = k.st;
  LFX_TRY(k.open());
  if (g->topology_stale) {LFX_TRY(upload_topology(k, g));}
  LFX_TRY(k.behind(g->tail));
  const lfx::PgArgs a = args_of(g);
  LFX_TRY(relinearize(c, g, a, st));
  std::vector<double> lin((size_t)lfx::kPgPlin * g->n_priors);
  LFX_HIP(c, hipMemcpyAsync(lin.data(), g->plin.p, sizeof(double) * lin.size(), hipMemcpyDeviceToHost, st));
  LFX_HIP(c, hipMemcpyAsync(grad_out, g->grad.p, sizeof(double) * 6u * g->n_nodes, hipMemcpyDeviceToHost, st));
  LFX_HIP(c, hipMemcpyAsync(g->h_record.p, g->record.p, sizeof(lfx::PgRecord), hipMemcpyDeviceToHost, st));
  LFX_HIP(c, hipStreamSynchronize(st));
  for (uint32_t p = 0; r_out && p < g->n_priors; p++) {std::memcpy(r_out + 6u * (size_t)p, lin.data() + (size_t)lfx::kPgPlin * p, sizeof(double) * 6u);}
  *chi2_out = reinterpret_cast<const lfx::PgRecord *>(g->h_record.p)->chi2;
  g->linearised = true;
  g->marg_current = false;
  g->fixed_stale = false;
  return k.finish();
}
#endif

}  // extern "C"
