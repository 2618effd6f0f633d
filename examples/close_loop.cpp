// close_loop.cpp -- loop closing without scans: a sensor drives two laps of a circle; its odometry steps carry noise, so the
// chained poses drift; a few loop closures tie the second lap to the first; lfx::PoseGraph optimises the poses on the device.
// Every pose here comes from pose arithmetic (lfx_motion_between and a product), none from a scan; close_loop_scans.cpp is
// the same loop from scans, its closures found and verified by lfx::LoopCloser.
//
//   close_loop [N [L [OUT]]]
//     N     nodes (default 256), two laps of a circle of radius 20 m
//     L     loop closures (default 5), each from a node of the first lap to the node at the same place in the second
//     OUT   N and E (2 x uint32), the chained poses (N x 12 doubles), the edges (E x lfx_pose_graph_edge), the optimised
//           poses (N x 12 doubles)
//   The worst position error against the true circle is printed before and after.  tests/test_pose_graph_cpp_gpu.py runs
//   the same graph through the Python binding and compares.
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

// uniform noise in [-1, 1) from a fixed sequence: the same graph on every run
struct Noise
{
  std::uint64_t state = 0x2545F4914F6CDD1DULL;
  double operator()()
  {
    state = state * 6364136223846793005ULL + 1442695040888963407ULL;
    return static_cast<double>(state >> 11) / 4503599627370496.0 - 1.0;
  }
};

double worst_error(const std::vector<double> & poses, const std::vector<Pose> & truth)
{
  double worst = 0.0;
  for (std::size_t k = 0; k < truth.size(); k++) {
    const double dx = poses[12 * k + 3] - truth[k].m[3], dy = poses[12 * k + 7] - truth[k].m[7], dz = poses[12 * k + 11] - truth[k].m[11];
    worst = std::fmax(worst, std::sqrt(dx * dx + dy * dy + dz * dz));
  }
  return worst;
}
}  // namespace

int main(int argc, char ** argv)
{
  try {
    const std::uint32_t n = argc > 1 ? static_cast<std::uint32_t>(std::stoul(argv[1])) : 256u;
    const std::uint32_t loops = argc > 2 ? static_cast<std::uint32_t>(std::stoul(argv[2])) : 5u;
    if (n < 8u || n % 2u || loops > n / 2u) {throw std::runtime_error("N must be even and >= 8, L <= N / 2");}
    const double radius = 20.0, sigma_rot = 0.002, sigma_t = 0.01, two_pi = 6.283185307179586;
    std::vector<Pose> truth(n);
    for (std::uint32_t k = 0; k < n; k++) {
      const double a = 2.0 * two_pi * k / n;
      truth[k] = planar(a + two_pi / 4.0, radius * std::cos(a), radius * std::sin(a));
    }
    Noise noise;
    // a measurement of pose_i^-1 pose_j with noise, its information diag(1 / sigma^2)
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
    std::vector<lfx_pose_graph_edge> edges;
    std::vector<double> chained(truth[0].m, truth[0].m + 12);
    Pose at = truth[0];
    for (std::uint32_t k = 0; k + 1u < n; k++) {             // the odometry: every step measured, the poses chained from it
      edges.push_back(measure(k, k + 1u, 0u));
      Pose z;
      for (int q = 0; q < 12; q++) {z.m[q] = edges.back().z[q];}
      at = product(at, z);
      chained.insert(chained.end(), at.m, at.m + 12);
    }
    for (std::uint32_t l = 0; l < loops; l++) {               // the closures: place recognition would name these pairs
      const std::uint32_t i = static_cast<std::uint32_t>((l + 0.5) * (n / 2u) / loops) % (n / 2u);
      edges.push_back(measure(i, i + n / 2u, LFX_EDGE_ROBUST));
    }

    lfx::FeatureExtraction extraction(lfx::HyperParameters(), 0, 1024);
    lfx::PoseGraph graph(extraction, lfx::PoseGraph::DefaultConfig(n, static_cast<std::uint32_t>(edges.size())));
    graph.AddNodes(chained);
    graph.AddEdges(edges);
    const lfx_pose_graph_result r = graph.Optimize();
    const std::vector<double> optimised = graph.Poses();
    const lfx_pose_graph_info_t info = graph.Info();
    std::printf("pose graph: %u nodes, %u chain and %u loop edges, %llu bytes on the device\n", info.n_nodes, info.n_chain, info.n_loop,
      static_cast<unsigned long long>(info.device_bytes));
    std::printf("optimised: code %d after %d iterations, chi2 %.6e -> %.6e, last step %.3e\n", r.code, r.iterations, r.chi2_initial, r.chi2_final,
      r.max_step);
    std::printf("worst position error: %.6f m before, %.6f m after\n", worst_error(chained, truth), worst_error(optimised, truth));
    if (argc > 3) {
      std::FILE * out = std::fopen(argv[3], "wb");
      if (!out) {throw std::runtime_error("cannot open the output file");}
      const std::uint32_t head[2] = {n, static_cast<std::uint32_t>(edges.size())};
      std::fwrite(head, sizeof(std::uint32_t), 2, out);
      std::fwrite(chained.data(), sizeof(double), chained.size(), out);
      std::fwrite(edges.data(), sizeof(lfx_pose_graph_edge), edges.size(), out);
      std::fwrite(optimised.data(), sizeof(double), optimised.size(), out);
      std::fclose(out);
    }
    return r.code == LFX_POSE_GRAPH_CONVERGED ? 0 : 3;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "close_loop: %s\n", e.what());
    return 1;
  }
}
