// repose_map.cpp -- a map that follows its pose graph: the drifted two-lap circle of close_loop.cpp, with a small synthetic
// cloud per keyframe.  The clouds go into an lfx::Keyframes store in the SENSOR frame, the chained poses into the store and
// into an lfx::PoseGraph.  The world map is built from the store at the chained poses and measured against the map at the
// true poses; the graph is optimised, the store follows it (device to device), and the map is built and measured again.
// Then a submap is cut around the lap-closing keyframe from the keyframes of the first lap only, and that keyframe's own cloud
// is localised against it: the measurement a loop closer would turn into the next loop edge.
//
//   repose_map [N [L [DIR]]]
//     N     keyframes (default 256), two laps of a circle of radius 20 m -- the graph is close_loop's for the same N and L
//     L     loop closures (default 5)
//     DIR   where DIR/edge.pcd and DIR/surface.pcd of the corrected map are written (lfx_keyframes_save)
//   The scene (world frame): a ring road between two 48-sided walls of radius 14 m and 26 m, a ground grid under it, and
//   poles at radius 17 m and 23 m; a keyframe holds what lies within 8 m of its true position, in its own frame.  The poles
//   are its edge cloud, ground and walls its surface cloud.  tests/test_keyframes_cpp_gpu.py reads the printed figures.
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

// uniform noise in [-1, 1) from a fixed sequence: the same graph on every run (close_loop's)
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

struct Scene {std::vector<double> edge, surface;};    // world points, 3 doubles each

Scene make_scene()
{
  Scene s;
  const double two_pi = 6.283185307179586;
  for (int side = 0; side < 48; side++) {
    const double a0 = two_pi * side / 48.0, a1 = two_pi * (side + 1) / 48.0;
    for (double r : {17.0, 23.0}) {                           // a pole at every corner
      for (int h = 0; h <= 30; h++) {s.edge.insert(s.edge.end(), {r * std::cos(a0), r * std::sin(a0), -1.5 + 0.1 * h});}
    }
    for (double r : {14.0, 26.0}) {                           // a wall panel from corner to corner
      const double x0 = r * std::cos(a0), y0 = r * std::sin(a0), x1 = r * std::cos(a1), y1 = r * std::sin(a1);
      const int steps = static_cast<int>(std::hypot(x1 - x0, y1 - y0) / 0.25);
      for (int i = 0; i < steps; i++) {
        for (int h = 0; h <= 10; h++) {
          s.surface.insert(s.surface.end(), {x0 + (x1 - x0) * i / steps, y0 + (y1 - y0) * i / steps, -1.5 + 0.3 * h});
        }
      }
    }
  }
  for (int ia = 0; ia < 240; ia++) {                          // the ground under the road
    for (int ir = 0; ir <= 22; ir++) {
      const double a = two_pi * ia / 240.0, r = 14.5 + 0.5 * ir;
      s.surface.insert(s.surface.end(), {r * std::cos(a), r * std::sin(a), -1.8});
    }
  }
  return s;
}

// what of `world` lies within `range` of the pose's position, in the pose's frame: records of 4 floats
std::vector<float> observe(const std::vector<double> & world, const Pose & pose, double range)
{
  std::vector<float> out;
  for (std::size_t i = 0; i < world.size(); i += 3) {
    const double d[3] = {world[i] - pose.m[3], world[i + 1] - pose.m[7], world[i + 2] - pose.m[11]};
    if (d[0] * d[0] + d[1] * d[1] > range * range) {continue;}
    for (int c = 0; c < 3; c++) {out.push_back(static_cast<float>((pose.m[c] * d[0] + pose.m[4 + c] * d[1]) + pose.m[8 + c] * d[2]));}
    out.push_back(0.0f);
  }
  return out;
}

// worst and mean distance between the records of two clouds of the same layout
void point_error(const float * a, const float * b, std::uint64_t n, double & worst, double & sum)
{
  for (std::uint64_t i = 0; i < n; i++) {
    const double dx = static_cast<double>(a[4 * i]) - b[4 * i], dy = static_cast<double>(a[4 * i + 1]) - b[4 * i + 1],
      dz = static_cast<double>(a[4 * i + 2]) - b[4 * i + 2];
    const double d = std::sqrt(dx * dx + dy * dy + dz * dz);
    worst = std::fmax(worst, d);
    sum += d;
  }
}
}  // namespace

int main(int argc, char ** argv)
{
  try {
    const std::uint32_t n = argc > 1 ? static_cast<std::uint32_t>(std::stoul(argv[1])) : 256u;
    const std::uint32_t loops = argc > 2 ? static_cast<std::uint32_t>(std::stoul(argv[2])) : 5u;
    if (n < 64u || n % 2u || loops > n / 2u) {throw std::runtime_error("N must be even and >= 64, L <= N / 2");}
    const double radius = 20.0, sigma_rot = 0.002, sigma_t = 0.01, two_pi = 6.283185307179586;
    std::vector<Pose> truth(n);
    for (std::uint32_t k = 0; k < n; k++) {
      const double a = 2.0 * two_pi * k / n;
      truth[k] = planar(a + two_pi / 4.0, radius * std::cos(a), radius * std::sin(a));
    }
    Noise noise;
    // close_loop's graph, measurement for measurement
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
    std::vector<double> chained(truth[0].m, truth[0].m + 12), true_poses;
    Pose at = truth[0];
    for (std::uint32_t k = 0; k + 1u < n; k++) {
      edges.push_back(measure(k, k + 1u, 0u));
      Pose z;
      for (int q = 0; q < 12; q++) {z.m[q] = edges.back().z[q];}
      at = product(at, z);
      chained.insert(chained.end(), at.m, at.m + 12);
    }
    for (std::uint32_t l = 0; l < loops; l++) {
      const std::uint32_t i = static_cast<std::uint32_t>((l + 0.5) * (n / 2u) / loops) % (n / 2u);
      edges.push_back(measure(i, i + n / 2u, LFX_EDGE_ROBUST));
    }
    for (const Pose & p : truth) {true_poses.insert(true_poses.end(), p.m, p.m + 12);}

    // every keyframe's clouds, as the sensor at the TRUE pose sees the scene
    const Scene scene = make_scene();
    std::vector<std::vector<float>> edge_clouds(n), surface_clouds(n);
    std::uint64_t total[2] = {0, 0};
    for (std::uint32_t k = 0; k < n; k++) {
      edge_clouds[k] = observe(scene.edge, truth[k], 8.0);
      surface_clouds[k] = observe(scene.surface, truth[k], 8.0);
      total[0] += edge_clouds[k].size() / 4u;
      total[1] += surface_clouds[k].size() / 4u;
    }

    lfx::FeatureExtraction extraction(lfx::HyperParameters(), 0, 1024);
    lfx::PoseGraph graph(extraction, lfx::PoseGraph::DefaultConfig(n, static_cast<std::uint32_t>(edges.size())));
    lfx::Keyframes keyframes(extraction, n, total[0], total[1]);
    graph.AddNodes(chained);
    graph.AddEdges(edges);
    for (std::uint32_t k = 0; k < n; k++) {                  // keyframe k is node k
      if (keyframes.AddHost(edge_clouds[k], surface_clouds[k], chained.data() + 12u * k) != k) {throw std::runtime_error("keyframe ids out of step");}
    }
    const lfx_keyframes_info_t info = keyframes.Info();
    std::printf("keyframe store: %u keyframes, %llu edge and %llu surface records, %llu bytes on the device\n", info.n_keyframes,
      static_cast<unsigned long long>(info.n_points[0]), static_cast<unsigned long long>(info.n_points[1]),
      static_cast<unsigned long long>(info.device_bytes));

    // the maps: pinned blocks the device writes and the host reads once the stream has passed the build (Poses waits for it)
    const lfx::Keyframes::Kind kinds[2] = {lfx::Keyframes::kEdge, lfx::Keyframes::kSurface};
    float * want[2], * got[2];
    for (int q = 0; q < 2; q++) {want[q] = extraction.PinnedFloats(4u * total[q]); got[q] = extraction.PinnedFloats(4u * total[q]);}
    auto build = [&](float * const out[2]) {
        for (int q = 0; q < 2; q++) {
          if (keyframes.Build(kinds[q], 0, n, out[q], total[q]) != total[q]) {throw std::runtime_error("a build of another size");}
        }
        keyframes.Poses(0, 1);
      };
    auto measure_map = [&](const char * when) {
        build(got);
        double worst = 0.0, sum = 0.0;
        for (int q = 0; q < 2; q++) {point_error(got[q], want[q], total[q], worst, sum);}
        std::printf("map point error %s: worst %.6f m, mean %.6f m\n", when, worst, sum / static_cast<double>(total[0] + total[1]));
      };
    keyframes.SetPoses(0, true_poses);
    build(want);
    keyframes.SetPoses(0, chained);
    measure_map("before");

    const lfx_pose_graph_result r = graph.Optimize();
    keyframes.Follow(graph);
    const std::vector<double> optimised = keyframes.Poses(0, n);
    std::printf("optimised: code %d after %d iterations, chi2 %.6e -> %.6e, last step %.3e\n", r.code, r.iterations, r.chi2_initial, r.chi2_final,
      r.max_step);
    std::printf("worst position error: %.6f m before, %.6f m after\n", worst_error(chained, truth), worst_error(optimised, truth));
    measure_map("after");

    // the loop closer's measurement: the last keyframe against the map of the first lap around it
    const std::uint32_t last = n - 1u, twin = n / 2u - 1u;
    const double * here = optimised.data() + 12u * last;
    const double center[3] = {here[3], here[7], here[11]};
    lfx_keyframes_submap_result cut[2];
    for (int q = 0; q < 2; q++) {cut[q] = keyframes.Submap(kinds[q], center, 5.0, 0, n / 2u, got[q], total[q]);}
    keyframes.Poses(0, 1);
    std::printf("submap around keyframe %u: keyframes %u .. %u, %llu edge and %llu surface records\n", last, cut[0].first_id, cut[0].last_id,
      static_cast<unsigned long long>(cut[0].n_points), static_cast<unsigned long long>(cut[1].n_points));
    if (cut[0].n_points == 0u || cut[1].n_points == 0u) {throw std::runtime_error("the submap is empty");}
    lfx_map * maps[2] = {nullptr, nullptr};
    for (int q = 0; q < 2; q++) {
      const int rc = lfx_map_create_host(extraction.handle(), got[q], static_cast<std::uint32_t>(cut[q].n_points), 1.0f, &maps[q], nullptr);
      if (rc != LFX_OK) {throw lfx::Error(rc, lfx_last_error(extraction.handle()));}
    }
    lfx_align_result aligned{};
    const int rc = lfx_localize_host(extraction.handle(), maps[0], maps[1], 15, 40, 1.0f, edge_clouds[last].data(),
      static_cast<std::uint32_t>(edge_clouds[last].size() / 4u), surface_clouds[last].data(), static_cast<std::uint32_t>(surface_clouds[last].size() / 4u),
      here, &aligned, nullptr);
    lfx_map_destroy(maps[0]);
    lfx_map_destroy(maps[1]);
    if (rc != LFX_OK) {throw lfx::Error(rc, lfx_last_error(extraction.handle()));}
    // keyframes `last` and `twin` stand at the same place: aligned against the first lap's map, `last` lands where that map
    // has `twin`
    const double * there = optimised.data() + 12u * twin;
    const double before = std::sqrt(std::pow(here[3] - there[3], 2) + std::pow(here[7] - there[7], 2) + std::pow(here[11] - there[11], 2));
    const double after = std::sqrt(std::pow(aligned.pose[3] - there[3], 2) + std::pow(aligned.pose[7] - there[7], 2) + std::pow(aligned.pose[11] - there[11], 2));
    std::printf("localised keyframe %u against it: code %d (%s) after %d iterations, %.6f m from keyframe %u before, %.6f m after\n", last, aligned.code,
      lfx_align_message(aligned.code), aligned.iteration, before, twin, after);
    if (argc > 3) {
      const std::pair<bool, bool> written = keyframes.Save(argv[3]);
      std::printf("saved: edge.pcd %d, surface.pcd %d\n", written.first ? 1 : 0, written.second ? 1 : 0);
    }
    return r.code == LFX_POSE_GRAPH_CONVERGED && LFX_ALIGN_SUCCESS(aligned.code) ? 0 : 3;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "repose_map: %s\n", e.what());
    return 1;
  }
}
