// close_loop_scans.cpp -- loop closing from scans, without ROS: every scan is a keyframe; its feature clouds go into an
// lfx::Keyframes store at its odometry pose, its scan-context descriptor into an lfx::PlaceDb and its pose into an
// lfx::PoseGraph with the odometry step that led to it (keyframe id == place entry == graph node id).  lfx::LoopCloser then
// finds the revisits among the keyframes, aligns each against a submap around the place it names, adds the accepted
// closures to the graph, optimises it and makes the store follow -- the glue examples/close_loop.cpp leaves out.
//
//   close_loop_scans SCANS N RINGS COLS POSES EDGES MIN_GAP SEARCH_RADIUS MAX_DISTANCE HALF_WINDOW SUBMAP_RADIUS OUT
//     SCANS     N scans of RINGS x COLS raw 32-byte PointXYZIR records, back to back
//     POSES     N x 12 doubles: the odometry (chained) pose [R | t] of every scan
//     EDGES     N - 1 lfx_pose_graph_edge records: the odometry steps
//     MIN_GAP .. SUBMAP_RADIUS   the lfx_loop_closer_config fields of those names (the rest stay at their defaults)
//     OUT       n_detected, n_verified, n_accepted (3 x uint32), followed, the graph's code (2 x int32), the graph's poses after
//               the update and the store's (N x 12 doubles each), then per keyframe MIN_GAP .. N - 1 its closure:
//               query, candidate (uint32), accepted, reason (int32), the aligned pose (12 doubles)
//   tests/test_loop_closer_cpp_gpu.py runs the same drive through the Python binding and compares.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "lfx.hpp"

namespace
{
template<typename T>
std::vector<T> slurp(const char * path)
{
  std::FILE * f = std::fopen(path, "rb");
  if (!f) {throw std::runtime_error(std::string("cannot open ") + path);}
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<T> v(static_cast<std::size_t>(bytes) / sizeof(T));
  if (!v.empty() && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) {std::fclose(f); throw std::runtime_error("short read");}
  std::fclose(f);
  return v;
}
}  // namespace

int main(int argc, char ** argv)
{
  try {
    if (argc < 13) {
      std::fprintf(stderr, "usage: close_loop_scans SCANS N RINGS COLS POSES EDGES MIN_GAP SEARCH_RADIUS MAX_DISTANCE HALF_WINDOW SUBMAP_RADIUS OUT\n");
      return 2;
    }
    const std::vector<lfx::PointXYZIR> scans = slurp<lfx::PointXYZIR>(argv[1]);
    const std::uint32_t n = static_cast<std::uint32_t>(std::stoul(argv[2]));
    const std::uint32_t rings = static_cast<std::uint32_t>(std::stoul(argv[3])), cols = static_cast<std::uint32_t>(std::stoul(argv[4]));
    const std::vector<double> poses = slurp<double>(argv[5]);
    const std::vector<lfx_pose_graph_edge> steps = slurp<lfx_pose_graph_edge>(argv[6]);
    const std::size_t per_scan = static_cast<std::size_t>(rings) * cols;
    if (n < 2u || scans.size() != per_scan * n || poses.size() != 12u * static_cast<std::size_t>(n) || steps.size() + 1u != n) {
      throw std::runtime_error("the files do not hold N scans of RINGS x COLS, N poses and N - 1 edges");
    }
    lfx::FeatureExtraction extraction(lfx::HyperParameters(), 0, static_cast<std::uint32_t>(per_scan), cols, rings, 0);
    const lfx_scan_context_config sc = lfx::FeatureExtraction::DefaultScanContextConfig();
    lfx::PlaceDb places(extraction, sc, n);
    lfx::Keyframes keyframes(extraction, n, per_scan * n, per_scan * n);
    lfx::PoseGraph graph(extraction, lfx::PoseGraph::DefaultConfig(n, 2u * n));
    float * descriptor = extraction.PinnedFloats(static_cast<std::size_t>(sc.n_rings) * sc.n_sectors);
    // the drive: keyframe k, place entry k and node k are the same scan
    for (std::uint32_t k = 0; k < n; k++) {
      extraction.ExtractFeaturesView(scans.data() + per_scan * k, per_scan);
      extraction.ScanContext(sc, 1, descriptor);
      places.Add(descriptor, 1);
      keyframes.Add(std::vector<double>(poses.begin() + 12 * k, poses.begin() + 12 * (k + 1)));
      extraction.BatchStatus();          // (all are queued: the next scan replaces the records and the descriptor they read)
    }
    graph.AddNodes(poses);
    graph.AddEdges(steps);

    const std::uint32_t min_gap = static_cast<std::uint32_t>(std::stoul(argv[7]));
    const std::uint32_t half_window = static_cast<std::uint32_t>(std::stoul(argv[10]));
    // a submap holds at most the window's keyframes
    const std::uint64_t capacity = per_scan * (2u * static_cast<std::uint64_t>(half_window) + 1u);
    lfx_loop_closer_config config = lfx::LoopCloser::DefaultConfig(capacity, capacity);
    config.min_gap = min_gap;
    config.search_radius = std::stod(argv[8]);
    config.max_distance = std::stod(argv[9]);
    config.submap_half_window = half_window;
    config.submap_radius = std::stod(argv[11]);
    lfx::LoopCloser closer(extraction, config, keyframes, places, graph);
    if (min_gap >= n) {throw std::runtime_error("MIN_GAP leaves no keyframe a candidate");}
    std::vector<lfx_loop_closure> closures;
    const lfx_loop_closer_result r = closer.Update(min_gap, n - min_gap, closures);
    std::printf("loop closer: %u of %u keyframes have a candidate, %u verified, %u accepted; %llu bytes on the device\n", r.n_detected, n - min_gap,
      r.n_verified, r.n_accepted, static_cast<unsigned long long>(closer.Info().device_bytes));
    for (const lfx_loop_closure & c : closures) {
      if (c.candidate == UINT32_MAX) {std::printf("keyframe %u: no candidate\n", c.query); continue;}
      std::printf("keyframe %u revisits %u (distance %.4f, yaw %.1f deg): %s, reason %d, rms edge %.4f surface %.4f\n", c.query, c.candidate,
        c.match.distance, c.match.yaw * 180.0 / M_PI, c.accepted ? "accepted" : "rejected", c.reason, c.report.rms_edge, c.report.rms_surface);
    }
    if (r.n_accepted) {
      std::printf("optimised: code %d after %d iterations, chi2 %.6e -> %.6e; the store %s\n", r.graph.code, r.graph.iterations, r.graph.chi2_initial,
        r.graph.chi2_final, r.followed ? "followed" : "stayed");
    }
    const std::vector<double> after = graph.Poses(), stored = keyframes.Poses(0, n);
    std::FILE * out = std::fopen(argv[12], "wb");
    if (!out) {throw std::runtime_error("cannot open the output file");}
    const std::uint32_t head[3] = {r.n_detected, r.n_verified, r.n_accepted};
    const std::int32_t tail[2] = {r.followed, r.graph.code};
    std::fwrite(head, sizeof(std::uint32_t), 3, out);
    std::fwrite(tail, sizeof(std::int32_t), 2, out);
    std::fwrite(after.data(), sizeof(double), after.size(), out);
    std::fwrite(stored.data(), sizeof(double), stored.size(), out);
    for (const lfx_loop_closure & c : closures) {
      std::fwrite(&c.query, sizeof(std::uint32_t), 1, out);
      std::fwrite(&c.candidate, sizeof(std::uint32_t), 1, out);
      std::fwrite(&c.accepted, sizeof(std::int32_t), 1, out);
      std::fwrite(&c.reason, sizeof(std::int32_t), 1, out);
      std::fwrite(c.result.pose, sizeof(double), 12, out);
    }
    std::fclose(out);
    return 0;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "close_loop_scans: %s\n", e.what());
    return 1;
  }
}
