// graph_covariance.cpp -- how well an optimised pose graph knows its nodes: the two-lap circle of close_loop.cpp is built and
// optimised, then lfx::PoseGraph::Marginals gives every node's covariance and JointCovariances / RelativeCovariance the
// uncertainty of one node as seen from another, which is what a loop candidate is gated by.
//
//   graph_covariance [N [L]]
//     N     nodes (default 256), two laps of a circle of radius 20 m
//     L     loop closures (default 5), each from a node of the first lap to the node at the same place in the second
//   Printed: the trace of the position covariance at 16 nodes along the trajectory, without the closures (it grows along
//   the open chain) and with them (it collapses where the laps are tied); then one Mahalanobis gate between a node of the
//   first lap and the node at the same place in the second, a pair no closure names: the true revisit passes, a candidate
//   3 sigma off in every whitened coordinate does not.  tests/test_graph_covariance_cpp_gpu.py runs it and compares the
//   traces with the Python binding's.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "lfx.hpp"

namespace
{
struct Pose {double m[12];};

Pose planar(double yaw, double x, double y)
{
  const double c = std::cos(yaw), s = std::sin(yaw);
  return Pose{{c, -s, 0.0, x, s, c, 0.0, y, 0.0, 0.0, 1.0, 0.0}};
}

// a b, both [R | t]
Pose product(const Pose & a, const Pose & b)
{
  Pose out;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 4; c++) {
      out.m[4 * r + c] = (a.m[4 * r] * b.m[c] + a.m[4 * r + 1] * b.m[4 + c]) + a.m[4 * r + 2] * b.m[8 + c];
    }
    out.m[4 * r + 3] += a.m[4 * r + 3];
  }
  return out;
}

// uniform noise in [-1, 1) from a fixed sequence: the same graph on every run (close_loop.cpp's)
struct Noise
{
  std::uint64_t state = 0x2545F4914F6CDD1DULL;
  double operator()()
  {
    state = state * 6364136223846793005ULL + 1442695040888963407ULL;
    return static_cast<double>(state >> 11) / 4503599627370496.0 - 1.0;
  }
};

// the residual r = (phi, t_E) of an edge (i, j, Z) at the poses Ti, Tj (lfx.h, the pose graph section)
void residual(const Pose & Ti, const Pose & Tj, const Pose & Z, double r[6])
{
  Pose Zi, E;
  lfx_motion_between(Ti.m, Tj.m, Zi.m);               // T_i^-1 T_j
  lfx_motion_between(Z.m, Zi.m, E.m);                 // Z^-1 T_i^-1 T_j = [R_E | t_E]
  const double v[3] = {0.5 * (E.m[9] - E.m[6]), 0.5 * (E.m[2] - E.m[8]), 0.5 * (E.m[4] - E.m[1])};
  const double nv = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  const double theta = std::atan2(nv, 0.5 * (E.m[0] + E.m[5] + E.m[10] - 1.0));
  for (int k = 0; k < 3; k++) {
    r[k] = nv < 1e-10 ? v[k] : v[k] * theta / nv;
    r[3 + k] = E.m[4 * k + 3];
  }
}

// the lower Cholesky factor of a 6 x 6 covariance
void cholesky6(const std::vector<double> & a, double L[36])
{
  for (int i = 0; i < 36; i++) {L[i] = 0.0;}
  for (int j = 0; j < 6; j++) {
    double p = a[7 * j];
    for (int m = 0; m < j; m++) {p -= L[6 * j + m] * L[6 * j + m];}
    if (!(p > 0.0)) {throw std::runtime_error("a covariance that is not positive definite");}
    L[7 * j] = std::sqrt(p);
    for (int r = j + 1; r < 6; r++) {
      double v = a[6 * r + j];
      for (int m = 0; m < j; m++) {v -= L[6 * r + m] * L[6 * j + m];}
      L[6 * r + j] = v / L[7 * j];
    }
  }
}

// r^T (L L^T)^-1 r
double mahalanobis2(const double L[36], const double r[6])
{
  double w[6], sum = 0.0;
  for (int i = 0; i < 6; i++) {
    double v = r[i];
    for (int m = 0; m < i; m++) {v -= L[6 * i + m] * w[m];}
    w[i] = v / L[7 * i];
    sum += w[i] * w[i];
  }
  return sum;
}
}  // namespace

int main(int argc, char ** argv)
{
  try {
    const std::uint32_t n = argc > 1 ? static_cast<std::uint32_t>(std::stoul(argv[1])) : 256u;
    const std::uint32_t loops = argc > 2 ? static_cast<std::uint32_t>(std::stoul(argv[2])) : 5u;
    if (n < 32u || n % 2u || loops < 1u || loops > n / 4u) {throw std::runtime_error("N must be even and >= 32, 1 <= L <= N / 4");}
    const double radius = 20.0, sigma_rot = 0.002, sigma_t = 0.01, two_pi = 6.283185307179586;
    std::vector<Pose> truth(n);
    for (std::uint32_t k = 0; k < n; k++) {
      const double a = 2.0 * two_pi * k / n;
      truth[k] = planar(a + two_pi / 4.0, radius * std::cos(a), radius * std::sin(a));
    }
    Noise noise;
    auto measure = [&](std::uint32_t i, std::uint32_t j, std::uint32_t flags) {
        lfx_pose_graph_edge e{};
        e.i = i; e.j = j; e.flags = flags;
        Pose z;
        lfx_motion_between(truth[i].m, truth[j].m, z.m);
        Pose jitter = planar(sigma_rot * noise(), sigma_t * noise(), sigma_t * noise());
        jitter.m[11] = sigma_t * noise();
        z = product(z, jitter);
        for (int q = 0; q < 12; q++) {e.z[q] = z.m[q];}
        for (int q = 0; q < 6; q++) {e.information[7 * q] = 1.0 / ((q < 3 ? sigma_rot : sigma_t) * (q < 3 ? sigma_rot : sigma_t));}
        return e;
      };
    std::vector<lfx_pose_graph_edge> chain, closures;
    std::vector<double> chained(truth[0].m, truth[0].m + 12);
    Pose at = truth[0];
    for (std::uint32_t k = 0; k + 1u < n; k++) {
      chain.push_back(measure(k, k + 1u, 0u));
      Pose z;
      for (int q = 0; q < 12; q++) {z.m[q] = chain.back().z[q];}
      at = product(at, z);
      chained.insert(chained.end(), at.m, at.m + 12);
    }
    for (std::uint32_t l = 0; l < loops; l++) {
      const std::uint32_t i = static_cast<std::uint32_t>((l + 0.5) * (n / 2u) / loops) % (n / 2u);
      closures.push_back(measure(i, i + n / 2u, LFX_EDGE_ROBUST));
    }

    lfx::FeatureExtraction extraction(lfx::HyperParameters(), 0, 1024);
    lfx::PoseGraph graph(extraction, lfx::PoseGraph::DefaultConfig(n, n - 1u + loops));
    graph.ReserveMarginals();
    graph.AddNodes(chained);
    graph.AddEdges(chain);
    lfx_pose_graph_result r = graph.Optimize();
    const std::vector<double> open = graph.Marginals();
    graph.AddEdges(closures);
    r = graph.Optimize();
    const std::vector<double> closed = graph.Marginals();
    const std::vector<double> poses = graph.Poses();
    std::printf("pose graph: %u nodes, %u loop closures, code %d after %d iterations\n", n, loops, r.code, r.iterations);
    std::printf("trace of the position covariance (m^2), the open chain and the closed graph:\n");
    auto trace = [](const std::vector<double> & cov, std::uint32_t k) {return cov[36u * k + 21u] + cov[36u * k + 28u] + cov[36u * k + 35u];};
    for (std::uint32_t s = 0; s < 16u; s++) {
      const std::uint32_t k = s == 15u ? n - 1u : s * (n / 16u);
      std::printf("  node %5u  open %.6e  closed %.6e\n", k, trace(open, k), trace(closed, k));
    }

    // the gate: is node j where node i was?  A pair of the two laps that no closure names.
    std::uint32_t i = n / 4u + 1u;
    for (const lfx_pose_graph_edge & e : closures) {
      if (e.i == i) {i++;}
    }
    const std::uint32_t j = i + n / 2u;
    const std::vector<double> joint = graph.JointCovariances({i, j});
    Pose Ti, Tj;
    for (int q = 0; q < 12; q++) {Ti.m[q] = poses[12u * i + q]; Tj.m[q] = poses[12u * j + q];}
    const std::vector<double> rel = lfx::PoseGraph::RelativeCovariance(Ti.m, Tj.m, joint.data());
    double L[36], res[6];
    cholesky6(rel, L);
    const double gate = 16.81;                                  // chi^2, 6 degrees of freedom, 99 %
    Pose revisit;
    lfx_motion_between(truth[i].m, truth[j].m, revisit.m);      // what a perfect scan match would measure
    residual(Ti, Tj, revisit, res);
    const double d_true = mahalanobis2(L, res);
    // a candidate whose residual lies 3 sigma further off in every whitened coordinate: r + 3 L (1 .. 1)^T
    for (int a = 0; a < 6; a++) {
      for (int b = 0; b <= a; b++) {res[a] += 3.0 * L[6 * a + b];}
    }
    const double d_off = mahalanobis2(L, res);
    std::printf("gate between nodes %u and %u (chi2 %.2f): sigma of the relative position %.4f %.4f %.4f m\n", i, j, gate,
      std::sqrt(rel[21]), std::sqrt(rel[28]), std::sqrt(rel[35]));
    std::printf("  the true revisit: d2 = %.3f, %s\n", d_true, d_true <= gate ? "accepted" : "rejected");
    std::printf("  a candidate 3 sigma off: d2 = %.3f, %s\n", d_off, d_off <= gate ? "accepted" : "rejected");
    return (r.code == LFX_POSE_GRAPH_CONVERGED && d_true <= gate && d_off > gate) ? 0 : 3;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "graph_covariance: %s\n", e.what());
    return 1;
  }
}
