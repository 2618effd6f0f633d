// anchor_loop.cpp -- drift bounded by absolute fixes instead of loop closures: the drifted two-lap circle of close_loop.cpp
// with its closures left out and its first pose turned by a heading error, which no relative measurement can see.  Every 16th
// node gets a noisy position fix of an antenna that sits off the sensor (a lever arm), as a GNSS receiver would give; the
// first node is released, so the fixes can turn and shift the trajectory as a whole; lfx::PoseGraph optimises on the device.
//
//   anchor_loop [N [OUT]]
//     N     nodes (default 256, a multiple of 16), two laps of a circle of radius 20 m
//     OUT   N and P (2 x uint32), the chained poses (N x 12 doubles), the edges ((N - 1) x lfx_pose_graph_edge), the priors
//           (P x lfx_pose_graph_prior), the optimised poses (N x 12 doubles)
//   The worst position error against the true circle and the heading error at node 0 are printed before and after.
//   tests/test_pose_graph_prior_cpp_gpu.py runs the same graph through the Python binding and compares.
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

// the yaw of node 0 against the truth's, in (-pi, pi]
double heading_error(const std::vector<double> & poses, const Pose & truth)
{
  const double d = std::atan2(poses[4], poses[0]) - std::atan2(truth.m[4], truth.m[0]);
  return std::atan2(std::sin(d), std::cos(d));
}
}  // namespace

int main(int argc, char ** argv)
{
  try {
    const std::uint32_t n = argc > 1 ? static_cast<std::uint32_t>(std::stoul(argv[1])) : 256u;
    if (n < 32u || n % 16u) {throw std::runtime_error("N must be a multiple of 16 and >= 32");}
    const double radius = 20.0, sigma_rot = 0.002, sigma_t = 0.01, sigma_fix = 0.05, first_heading_error = 0.03, two_pi = 6.283185307179586;
    const double lever[3] = {0.8, -0.2, 1.5};
    std::vector<Pose> truth(n);
    for (std::uint32_t k = 0; k < n; k++) {
      const double a = 2.0 * two_pi * k / n;
      truth[k] = planar(a + two_pi / 4.0, radius * std::cos(a), radius * std::sin(a));
    }
    Noise noise;
    std::vector<lfx_pose_graph_edge> edges;
    // the odometry: every step measured with noise, the poses chained from it -- from a first pose whose heading is off
    Pose at = planar(two_pi / 4.0 + first_heading_error, radius, 0.0);
    std::vector<double> chained(at.m, at.m + 12);
    for (std::uint32_t k = 0; k + 1u < n; k++) {
      lfx_pose_graph_edge e{};
      e.i = k; e.j = k + 1u;
      Pose z;
      lfx_motion_between(truth[k].m, truth[k + 1u].m, z.m);
      Pose jitter = planar(sigma_rot * noise(), sigma_t * noise(), sigma_t * noise());
      jitter.m[11] = sigma_t * noise();
      z = product(z, jitter);
      for (int q = 0; q < 12; q++) {e.z[q] = z.m[q];}
      for (int q = 0; q < 6; q++) {e.information[7 * q] = 1.0 / ((q < 3 ? sigma_rot : sigma_t) * (q < 3 ? sigma_rot : sigma_t));}
      edges.push_back(e);
      at = product(at, z);
      chained.insert(chained.end(), at.m, at.m + 12);
    }
    // the fixes: the antenna's true place t + R l with noise, on every 16th node
    std::vector<lfx_pose_graph_prior> priors;
    for (std::uint32_t k = 0; k < n; k += 16u) {
      lfx_pose_graph_prior p{};
      p.node = k;
      p.flags = LFX_PRIOR_POSITION | LFX_PRIOR_ROBUST;
      for (int r = 0; r < 3; r++) {
        const double * row = truth[k].m + 4 * r;
        p.z[4 * r + 3] = (row[3] + ((row[0] * lever[0] + row[1] * lever[1]) + row[2] * lever[2])) + sigma_fix * noise();
        p.information[7 * (3 + r)] = 1.0 / (sigma_fix * sigma_fix);
        p.lever[r] = lever[r];
      }
      priors.push_back(p);
    }

    lfx::FeatureExtraction extraction(lfx::HyperParameters(), 0, 1024);
    lfx_pose_graph_config config = lfx::PoseGraph::DefaultConfig(n, static_cast<std::uint32_t>(edges.size()));
    config.max_iter = 20u;
    lfx::PoseGraph graph(extraction, config);
    graph.AddNodes(chained);
    graph.AddEdges(edges);
    graph.ReservePriors(static_cast<std::uint32_t>(priors.size()));
    graph.AddPriors(priors);
    graph.ReleaseFirst();
    const lfx_pose_graph_result r = graph.Optimize();
    const std::vector<double> optimised = graph.Poses();
    const lfx_pose_graph_info_t info = graph.Info();
    const lfx_pose_graph_prior_info_t pinfo = graph.PriorInfo();
    std::printf("pose graph: %u nodes, %u chain and %u loop edges, %u priors, %llu bytes on the device\n", info.n_nodes, info.n_chain, info.n_loop,
      pinfo.n_priors, static_cast<unsigned long long>(info.device_bytes));
    std::printf("optimised: code %d after %d iterations, chi2 %.6e -> %.6e (the priors' share %.6e), last step %.3e\n", r.code, r.iterations,
      r.chi2_initial, r.chi2_final, pinfo.chi2, r.max_step);
    std::printf("worst position error: %.6f m before, %.6f m after\n", worst_error(chained, truth), worst_error(optimised, truth));
    std::printf("heading error at node 0: %.6f rad before, %.6f rad after\n", heading_error(chained, truth[0]), heading_error(optimised, truth[0]));
    if (argc > 2) {
      std::FILE * out = std::fopen(argv[2], "wb");
      if (!out) {throw std::runtime_error("cannot open the output file");}
      const std::uint32_t head[2] = {n, static_cast<std::uint32_t>(priors.size())};
      std::fwrite(head, sizeof(std::uint32_t), 2, out);
      std::fwrite(chained.data(), sizeof(double), chained.size(), out);
      std::fwrite(edges.data(), sizeof(lfx_pose_graph_edge), edges.size(), out);
      std::fwrite(priors.data(), sizeof(lfx_pose_graph_prior), priors.size(), out);
      std::fwrite(optimised.data(), sizeof(double), optimised.size(), out);
      std::fclose(out);
    }
    return r.code == LFX_POSE_GRAPH_CONVERGED ? 0 : 3;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "anchor_loop: %s\n", e.what());
    return 1;
  }
}
