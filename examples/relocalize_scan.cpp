// relocalize_scan.cpp -- "where am I in this map?" without ROS: the keyframes of a map are extracted and indexed by their
// scan-context descriptors (lfx::FeatureExtraction::ScanContext, lfx::PlaceDb), a scan taken somewhere in that map is
// recognised, and lfx::Localizer refines the pose the index proposes.
//
//   relocalize_scan KEYFRAMES N_KEYFRAMES SCAN RINGS COLS OUT
//     KEYFRAMES   N_KEYFRAMES scans of RINGS x COLS raw 32-byte PointXYZIR records, back to back
//     SCAN        one such scan: the revisit
//     OUT         the match (uint32 entry, uint32 shift, double distance, double yaw), then the localisation from the
//                 proposed pose: 12 doubles pose [R | t], error, error_scale (doubles), iteration, code (int32)
//   Every keyframe's map is its own two feature clouds in its own frame, so the pose that comes out is the revisit's pose
//   in the frame of the keyframe it was recognised as: the proposal is Rz(yaw) with no translation.
//   tests/test_relocalize_cpp_gpu.py compares with the Python binding.
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

struct Keyframe { std::vector<float> edge, surface; };
}  // namespace

int main(int argc, char ** argv)
{
  try {
    if (argc < 7) {
      std::fprintf(stderr, "usage: relocalize_scan KEYFRAMES N_KEYFRAMES SCAN RINGS COLS OUT\n");
      return 2;
    }
    const std::vector<lfx::PointXYZIR> keyframes = slurp<lfx::PointXYZIR>(argv[1]), scan = slurp<lfx::PointXYZIR>(argv[3]);
    const std::uint32_t n_key = static_cast<std::uint32_t>(std::stoul(argv[2]));
    const std::uint32_t rings = static_cast<std::uint32_t>(std::stoul(argv[4])), cols = static_cast<std::uint32_t>(std::stoul(argv[5]));
    const std::size_t per_scan = static_cast<std::size_t>(rings) * cols;
    if (n_key == 0 || keyframes.size() != per_scan * n_key || scan.size() != per_scan) {throw std::runtime_error("the files do not hold RINGS x COLS scans");}
    lfx::FeatureExtraction extraction(lfx::HyperParameters(), 0, static_cast<std::uint32_t>(per_scan), cols, rings, 0);
    const lfx_scan_context_config config = lfx::FeatureExtraction::DefaultScanContextConfig();
    lfx::PlaceDb places(extraction, config, n_key);
    // one descriptor in memory that the device writes and the index reads
    float * descriptor = extraction.PinnedFloats(static_cast<std::size_t>(config.n_rings) * config.n_sectors);
    // the map: every keyframe's features, and its descriptor in the index (entry k = keyframe k)
    std::vector<Keyframe> map(n_key);
    for (std::uint32_t k = 0; k < n_key; k++) {
      const lfx_scan_result view = extraction.ExtractFeaturesView(keyframes.data() + per_scan * k, per_scan);
      map[k].edge.assign(view.edge_points, view.edge_points + 4 * static_cast<std::size_t>(view.n_edge));
      map[k].surface.assign(view.surface_points, view.surface_points + 4 * static_cast<std::size_t>(view.n_surface));
      extraction.ScanContext(config, 1, descriptor);
      places.Add(descriptor, 1);
      extraction.BatchStatus();          // (both are queued: the next scan replaces the records and the descriptor they read)
    }
    // the revisit: features, descriptor, the best entry and the yaw it proposes
    extraction.ExtractFeaturesView(scan.data(), scan.size());
    extraction.ScanContext(config, 1, descriptor);
    const lfx_place_match match = places.Query(descriptor, 1, 1)[0];
    std::printf("recognised keyframe %u of %u: shift %u, distance %.6f, yaw %.3f deg\n", match.entry, places.Size(), match.shift, match.distance,
      match.yaw * 180.0 / M_PI);
    // the pose from the proposal, against that keyframe's own clouds (the revisit's clouds are still on the device)
    lfx::Localizer localizer(extraction, map[match.entry].edge, map[match.entry].surface, 20, 1.0f);
    const double c = std::cos(match.yaw), s = std::sin(match.yaw);
    const double proposal[12] = {c, -s, 0, 0, s, c, 0, 0, 0, 0, 1, 0};
    localizer.Init(proposal);
    const bool ok = localizer.Update();
    const lfx_align_result & r = localizer.Result();
    std::printf("update %s: iteration %d, %s\n", ok ? "succeeded" : "failed", r.iteration, lfx_align_message(r.code));
    std::printf("pose in the keyframe's frame: t = %.4f %.4f %.4f, yaw %.3f deg\n", r.pose[3], r.pose[7], r.pose[11],
      std::atan2(r.pose[4], r.pose[0]) * 180.0 / M_PI);
    std::FILE * out = std::fopen(argv[6], "wb");
    if (!out) {throw std::runtime_error("cannot open the output file");}
    std::fwrite(&match.entry, sizeof(std::uint32_t), 1, out);
    std::fwrite(&match.shift, sizeof(std::uint32_t), 1, out);
    std::fwrite(&match.distance, sizeof(double), 1, out);
    std::fwrite(&match.yaw, sizeof(double), 1, out);
    std::fwrite(r.pose, sizeof(double), 12, out);
    std::fwrite(&r.error, sizeof(double), 1, out);
    std::fwrite(&r.error_scale, sizeof(double), 1, out);
    std::fwrite(&r.iteration, sizeof(std::int32_t), 1, out);
    std::fwrite(&r.code, sizeof(std::int32_t), 1, out);
    std::fclose(out);
    return 0;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "relocalize_scan: %s\n", e.what());
    return 1;
  }
}
