// clean_closer.cpp -- the local map a loop closer verifies against, without what moved while it was recorded: keyframes
// read from a directory go into an lfx::Keyframes store in the SENSOR frame with their poses, the store reserves its own
// flags (lfx::Keyframes::ReserveFlags), lfx::Visibility votes straight into them, and lfx::Keyframes::SubmapMasked writes the
// keyframes around one keyframe without the records the votes flag DYNAMIC.  (lfx::LoopCloser::SetMasked makes a closer do
// the same in its verification.)
//
//   clean_closer IN CENTER RADIUS [ROWS COLUMNS ELEV_MIN ELEV_STEP GUARD]
//     IN      IN/poses.txt, IN/edge_K.pcd, IN/surface_K.pcd as examples/clean_map.cpp reads them
//     CENTER  the keyframe whose translation is the submap's centre; RADIUS in metres
//     ROWS .. GUARD   the range images (lfx_visibility_config); the defaults otherwise.  None is measured on real data.
//   Printed per kind: the result record and the FNV-1a checksum (64 bits) of the submap's bytes.
//   tests/test_clean_closer_cpp_gpu.py reads the printed figures.
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

std::uint64_t fnv1a(const void * data, std::size_t bytes)
{
  const unsigned char * p = static_cast<const unsigned char *>(data);
  std::uint64_t h = 14695981039346656037ull;
  for (std::size_t i = 0; i < bytes; i++) {h = (h ^ p[i]) * 1099511628211ull;}
  return h;
}
}  // namespace

int main(int argc, char ** argv)
{
  try {
    if (argc != 4 && argc != 9) {
      std::fprintf(stderr, "usage: clean_closer IN CENTER RADIUS [ROWS COLUMNS ELEV_MIN ELEV_STEP GUARD]\n");
      return 2;
    }
    const std::string in(argv[1]);
    const std::uint32_t center_id = static_cast<std::uint32_t>(std::stoul(argv[2]));
    const double radius = std::strtod(argv[3], nullptr);
    lfx_visibility_config config = lfx::Visibility::DefaultConfig();
    if (argc == 9) {
      config.n_rows = static_cast<std::uint32_t>(std::stoul(argv[4]));
      config.n_columns = static_cast<std::uint32_t>(std::stoul(argv[5]));
      config.elev_min = std::strtof(argv[6], nullptr);
      config.elev_step = std::strtof(argv[7], nullptr);
      config.guard = static_cast<std::uint32_t>(std::stoul(argv[8]));
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
    if (center_id >= n) {throw std::runtime_error("CENTER is not a keyframe");}
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
    // the store's own flags; the votes go straight into them
    keyframes.ReserveFlags();
    const std::pair<std::uint8_t *, std::uint8_t *> d = keyframes.Flags();
    std::uint8_t * const flags[2] = {d.first, d.second};
    std::uint32_t * const no_votes[2] = {nullptr, nullptr};
    lfx::Visibility visibility(extraction, config, n, n);
    const lfx_visibility_result r = visibility.Run(keyframes, 0, n, no_votes, flags);
    const lfx_keyframes_flags_info_t fi = keyframes.FlagsInfo();
    if (fi.n_flagged[0] != r.n_dynamic[0] || fi.n_flagged[1] != r.n_dynamic[1]) {throw std::runtime_error("the store counts other flags than the votes set");}
    std::printf("flags: %llu of %llu edge and %llu of %llu surface records\n", static_cast<unsigned long long>(fi.n_flagged[0]),
      static_cast<unsigned long long>(total[0]), static_cast<unsigned long long>(fi.n_flagged[1]), static_cast<unsigned long long>(total[1]));

    const double center[3] = {poses[12u * center_id + 3u], poses[12u * center_id + 7u], poses[12u * center_id + 11u]};
    const lfx::Keyframes::Kind kinds[2] = {lfx::Keyframes::kEdge, lfx::Keyframes::kSurface};
    for (int q = 0; q < 2; q++) {
      float * map = extraction.PinnedFloats(4u * total[q] + 4u);
      const lfx_keyframes_submap_result s = keyframes.SubmapMasked(kinds[q], center, radius, 0, n, map, total[q]);
      keyframes.Poses(0, 1);                                 // (waits for the stream: the submap is written)
      std::printf("%s: selected %u written %u points %llu first %u last %u truncated %d checksum %016llx\n", q ? "surface" : "edge", s.n_selected,
        s.n_written_keyframes, static_cast<unsigned long long>(s.n_points), s.first_id, s.last_id, s.truncated,
        static_cast<unsigned long long>(fnv1a(map, 16u * static_cast<std::size_t>(s.n_points))));
    }
    return 0;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "clean_closer: %s\n", e.what());
    return 1;
  }
}
