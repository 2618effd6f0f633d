// filter_map.cpp -- the last step of the pipeline: keyframes read from a directory go into an lfx::Keyframes store in the
// SENSOR frame with their poses, lfx::Visibility flags what moved while the map was recorded (into the store's own flags),
// lfx::Keyframes::SaveFiltered writes the map of each kind without those records and thinned to one centroid per voxel
// (lfx::VoxelFilter straight from the store: no world cloud in between), and an lfx::Localizer is built from the two files and
// localises one keyframe's clouds against them.
//
//   filter_map IN OUT [EDGE_LEAF SURFACE_LEAF MIN_POINTS [ROWS COLUMNS ELEV_MIN ELEV_STEP GUARD]]
//     IN     IN/poses.txt: one keyframe per line, 12 numbers, [R | t] row-major; IN/edge_K.pcd and IN/surface_K.pcd, K = 0, 1,
//            ..: keyframe K's clouds in its own frame (a missing file is an empty cloud)
//     OUT    where OUT/edge.pcd and OUT/surface.pcd of the filtered map are written
//     EDGE_LEAF SURFACE_LEAF MIN_POINTS   0.2 0.4 1 (LIO-SAM's and LeGO-LOAM's leaves)
//     ROWS .. GUARD   the range images of the votes (lfx_visibility_config); the defaults otherwise, none of them measured
//   tests/test_voxel_filter_cpp_gpu.py reads the printed figures and the two files.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "lfx.hpp"

namespace
{
// the records of a PCD file, 4 floats each (x, y, z, 1); none if the file is not there
std::vector<float> read_cloud(const std::string & path)
{
  if (!std::ifstream(path).good()) {return {};}
  return lfx::ReadPcd(path, false);
}
}  // namespace

int main(int argc, char ** argv)
{
  try {
    if (argc != 3 && argc != 6 && argc != 11) {
      std::fprintf(stderr, "usage: filter_map IN OUT [EDGE_LEAF SURFACE_LEAF MIN_POINTS [ROWS COLUMNS ELEV_MIN ELEV_STEP GUARD]]\n");
      return 2;
    }
    const std::string in(argv[1]), out(argv[2]);
    const float edge_leaf = argc >= 6 ? std::strtof(argv[3], nullptr) : 0.2f, surface_leaf = argc >= 6 ? std::strtof(argv[4], nullptr) : 0.4f;
    const std::uint32_t min_points = argc >= 6 ? static_cast<std::uint32_t>(std::stoul(argv[5])) : 1u;
    lfx_visibility_config config = lfx::Visibility::DefaultConfig();
    if (argc == 11) {
      config.n_rows = static_cast<std::uint32_t>(std::stoul(argv[6]));
      config.n_columns = static_cast<std::uint32_t>(std::stoul(argv[7]));
      config.elev_min = std::strtof(argv[8], nullptr);
      config.elev_step = std::strtof(argv[9], nullptr);
      config.guard = static_cast<std::uint32_t>(std::stoul(argv[10]));
    }
    std::vector<double> poses;
    {
      std::ifstream f(in + "/poses.txt");
      if (!f.good()) {throw std::runtime_error("cannot read " + in + "/poses.txt");}
      std::string line;
      while (std::getline(f, line)) {
        std::istringstream s(line);
        double v;
        std::size_t got = 0;
        while (s >> v) {poses.push_back(v); got++;}
        if (got != 0u && got != 12u) {throw std::runtime_error("poses.txt: a line without 12 numbers");}
      }
    }
    const std::uint32_t n = static_cast<std::uint32_t>(poses.size() / 12u);
    if (n == 0u) {throw std::runtime_error("no keyframe");}
    std::vector<std::vector<float>> clouds[2];
    std::uint64_t total[2] = {0, 0};
    for (std::uint32_t k = 0; k < n; k++) {
      clouds[0].push_back(read_cloud(in + "/edge_" + std::to_string(k) + ".pcd"));
      clouds[1].push_back(read_cloud(in + "/surface_" + std::to_string(k) + ".pcd"));
      for (int q = 0; q < 2; q++) {total[q] += clouds[q].back().size() / 4u;}
    }

    lfx::FeatureExtraction extraction(lfx::HyperParameters(), 0, 1024);
    lfx::Keyframes keyframes(extraction, n, total[0] ? total[0] : 1u, total[1] ? total[1] : 1u);
    for (std::uint32_t k = 0; k < n; k++) {
      if (keyframes.AddHost(clouds[0][k], clouds[1][k], poses.data() + 12u * k) != k) {throw std::runtime_error("keyframe ids out of step");}
    }
    std::printf("keyframe store: %u keyframes, %llu edge and %llu surface records\n", n, static_cast<unsigned long long>(total[0]),
      static_cast<unsigned long long>(total[1]));

    // the votes, straight into the flags the store keeps
    keyframes.ReserveFlags();
    const std::pair<std::uint8_t *, std::uint8_t *> d_flags = keyframes.Flags();
    std::uint8_t * const flags[2] = {d_flags.first, d_flags.second};
    std::uint32_t * const no_votes[2] = {nullptr, nullptr};
    lfx::Visibility visibility(extraction, config, n, n);
    const lfx_visibility_result r = visibility.Run(keyframes, 0, n, no_votes, flags);
    std::printf("visibility: %llu edge and %llu surface records dynamic\n", static_cast<unsigned long long>(r.n_dynamic[0]),
      static_cast<unsigned long long>(r.n_dynamic[1]));

    // a table of about twice the voxels expected: here no more voxels than records, so the next power of two above twice those
    const std::uint64_t most = total[0] > total[1] ? total[0] : total[1];
    std::uint32_t log2_slots = 4;
    while (log2_slots < 30u && (std::uint64_t(1) << log2_slots) < 2u * most) {log2_slots++;}
    lfx::VoxelFilter filter(extraction, log2_slots, most ? most : 1u);
    const std::pair<bool, bool> written = keyframes.SaveFiltered(filter, out, edge_leaf, surface_leaf, min_points, true);
    std::printf("filtered map: edge.pcd %s, surface.pcd %s\n", written.first ? "written" : "not written", written.second ? "written" : "not written");

    // the same through the filter's own calls: what the files hold, counted
    const lfx::Keyframes::Kind kinds[2] = {lfx::Keyframes::kEdge, lfx::Keyframes::kSurface};
    const float leaf[2] = {edge_leaf, surface_leaf};
    for (int q = 0; q < 2; q++) {
      filter.Reset(leaf[q]);
      filter.AddKeyframes(keyframes, kinds[q], 0, n, true);
      float * d_map = extraction.PinnedFloats(4u * total[q] + 4u);
      const lfx_voxel_filter_result e = filter.Emit(min_points, d_map, total[q]);
      std::printf("%s: %llu records, %llu accumulated, %llu voxels, %llu written (leaf %g, load %.3f)\n", q ? "surface" : "edge",
        static_cast<unsigned long long>(e.n_records), static_cast<unsigned long long>(e.n_accumulated), static_cast<unsigned long long>(e.n_voxels),
        static_cast<unsigned long long>(e.n_written), static_cast<double>(leaf[q]), static_cast<double>(e.n_voxels) / static_cast<double>(filter.Info().slots));
    }

    if (written.first && written.second) {
      lfx::Localizer localizer(extraction, out + "/edge.pcd", out + "/surface.pcd");
      const std::uint32_t k = n / 2u;
      localizer.Init(poses.data() + 12u * k);
      const bool ok = localizer.Update(clouds[0][k].data(), static_cast<std::uint32_t>(clouds[0][k].size() / 4u), clouds[1][k].data(),
        static_cast<std::uint32_t>(clouds[1][k].size() / 4u));
      const double * p = localizer.Get(), * p0 = poses.data() + 12u * k;
      const double d = std::sqrt((p[3] - p0[3]) * (p[3] - p0[3]) + (p[7] - p0[7]) * (p[7] - p0[7]) + (p[11] - p0[11]) * (p[11] - p0[11]));
      std::printf("localised keyframe %u against the filtered map: %s, code %d, %.4f m from its pose\n", k, ok ? "success" : "no success",
        static_cast<int>(localizer.Result().code), d);
    }
    return 0;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "filter_map: %s\n", e.what());
    return 1;
  }
}
