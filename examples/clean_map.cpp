// clean_map.cpp -- a map without what moved while it was recorded: keyframes read from a directory go into an
// lfx::Keyframes store in the SENSOR frame with their poses, lfx::Visibility lets every keyframe vote on the records of the
// keyframes near it, and the map of each kind is built without the records the votes flag DYNAMIC
// (lfx::Keyframes::BuildMasked) and written through lfx_pcd_write.
//
//   clean_map IN OUT [ROWS COLUMNS ELEV_MIN ELEV_STEP GUARD]
//     IN     IN/poses.txt: one keyframe per line, 12 numbers, [R | t] row-major; IN/edge_K.pcd and IN/surface_K.pcd, K = 0, 1,
//            ..: keyframe K's clouds in its own frame (a missing file is an empty cloud)
//     OUT    where OUT/edge.pcd and OUT/surface.pcd of the cleaned map are written
//     ROWS .. GUARD   the range images (lfx_visibility_config: n_rows, n_columns, elev_min, elev_step, guard); the defaults
//            otherwise.  None of the defaults is measured on real data.
//   tests/test_visibility_cpp_gpu.py reads the printed figures and the two files.
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
  char msg[512];
  std::uint64_t n = 0, bad = 0;
  int rc = lfx_pcd_read(path.c_str(), nullptr, 0, 0, &n, &bad, msg, sizeof(msg));
  if (rc != LFX_OK) {throw lfx::Error(rc, msg);}
  std::vector<float> out(4u * static_cast<std::size_t>(n));
  if (n > 0u) {
    rc = lfx_pcd_read(path.c_str(), out.data(), n, 0, &n, &bad, msg, sizeof(msg));
    if (rc != LFX_OK) {throw lfx::Error(rc, msg);}
  }
  return out;
}
}  // namespace

int main(int argc, char ** argv)
{
  try {
    if (argc != 3 && argc != 8) {
      std::fprintf(stderr, "usage: clean_map IN OUT [ROWS COLUMNS ELEV_MIN ELEV_STEP GUARD]\n");
      return 2;
    }
    const std::string in(argv[1]), out(argv[2]);
    lfx_visibility_config config = lfx::Visibility::DefaultConfig();
    if (argc == 8) {
      config.n_rows = static_cast<std::uint32_t>(std::stoul(argv[3]));
      config.n_columns = static_cast<std::uint32_t>(std::stoul(argv[4]));
      config.elev_min = std::strtof(argv[5], nullptr);
      config.elev_step = std::strtof(argv[6], nullptr);
      config.guard = static_cast<std::uint32_t>(std::stoul(argv[7]));
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

    // the flags: one byte per record of the store, in pinned blocks the device writes and reads (as the maps below)
    std::uint8_t * flags[2];
    float * map[2];
    for (int q = 0; q < 2; q++) {
      flags[q] = reinterpret_cast<std::uint8_t *>(extraction.PinnedFloats(total[q] / 4u + 1u));
      map[q] = extraction.PinnedFloats(4u * total[q] + 4u);
    }
    std::uint32_t * const no_votes[2] = {nullptr, nullptr};
    lfx::Visibility visibility(extraction, config, n, n);
    const lfx_visibility_result r = visibility.Run(keyframes, 0, n, no_votes, flags);
    std::printf("visibility: %llu pairs in %u chunk(s), images %llu of %llu cells occupied\n", static_cast<unsigned long long>(r.n_pairs),
      r.n_viewer_chunks, static_cast<unsigned long long>(r.occupied_cells), static_cast<unsigned long long>(r.total_cells));
    std::printf("edge: %llu records, %llu voted on, %llu dynamic\n", static_cast<unsigned long long>(r.n_records[0]),
      static_cast<unsigned long long>(r.n_voted[0]), static_cast<unsigned long long>(r.n_dynamic[0]));
    std::printf("surface: %llu records, %llu voted on, %llu dynamic\n", static_cast<unsigned long long>(r.n_records[1]),
      static_cast<unsigned long long>(r.n_voted[1]), static_cast<unsigned long long>(r.n_dynamic[1]));

    const lfx::Keyframes::Kind kinds[2] = {lfx::Keyframes::kEdge, lfx::Keyframes::kSurface};
    std::uint64_t kept[2];
    for (int q = 0; q < 2; q++) {kept[q] = keyframes.BuildMasked(kinds[q], 0, n, flags[q], map[q], total[q]);}
    keyframes.Poses(0, 1);                                   // (waits for the stream: the maps are written)
    for (int q = 0; q < 2; q++) {
      if (kept[q] + r.n_dynamic[q] != total[q]) {throw std::runtime_error("the masked build kept another number of records than the votes left");}
      char msg[512];
      const std::string path = out + (q ? "/surface.pcd" : "/edge.pcd");
      const int rc = lfx_pcd_write(path.c_str(), map[q], kept[q], msg, sizeof(msg));
      if (rc != LFX_OK) {throw lfx::Error(rc, msg);}
    }
    std::printf("clean map: %llu of %llu edge and %llu of %llu surface records kept\n", static_cast<unsigned long long>(kept[0]),
      static_cast<unsigned long long>(total[0]), static_cast<unsigned long long>(kept[1]), static_cast<unsigned long long>(total[1]));
    return 0;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "clean_map: %s\n", e.what());
    return 1;
  }
}
