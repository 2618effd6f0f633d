// segment_scan.cpp -- LeGO-LOAM's front end without ROS: every scan is extracted, segmented into ground, clusters and
// clutter (lfx::FeatureExtraction::Segment), its feature clouds are packed through the default class masks -- edges from
// clusters, surfaces from the ground and from clusters (PackFeaturesSegmented) -- and lfx::Odometry aligns the filtered
// clouds against the last scans (lfx_odometry_update).
//
//   segment_scan SCANS RINGS COLS N OUT
//     SCANS   N scans of RINGS x COLS raw 32-byte PointXYZIR records (point_type.hpp:62-86), back to back
//     OUT     per scan: the records by class (4 x uint32: none, ground, segment, clutter), the edge and surface features kept
//             (2 x uint32), then 12 doubles pose [R | t], error, error_scale (doubles), iteration, code, aligned (int32)
//   The counts per class and the pose are printed.  tests/test_segment_cpp_gpu.py compares them with the Python binding.
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "lfx.hpp"

namespace
{
std::vector<lfx::PointXYZIR> slurp(const char * path)
{
  std::FILE * f = std::fopen(path, "rb");
  if (!f) {throw std::runtime_error(std::string("cannot open ") + path);}
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<lfx::PointXYZIR> v(static_cast<std::size_t>(bytes) / sizeof(lfx::PointXYZIR));
  if (!v.empty() && std::fread(v.data(), sizeof(lfx::PointXYZIR), v.size(), f) != v.size()) {std::fclose(f); throw std::runtime_error("short read");}
  std::fclose(f);
  return v;
}
}  // namespace

int main(int argc, char ** argv)
{
  try {
    if (argc < 6) {
      std::fprintf(stderr, "usage: segment_scan SCANS RINGS COLS N OUT\n");
      return 2;
    }
    const std::vector<lfx::PointXYZIR> scans = slurp(argv[1]);
    const std::uint32_t rings = static_cast<std::uint32_t>(std::stoul(argv[2])), cols = static_cast<std::uint32_t>(std::stoul(argv[3]));
    const std::uint32_t n = static_cast<std::uint32_t>(std::stoul(argv[4])), per = rings * cols;
    if (scans.size() != static_cast<std::size_t>(n) * per) {throw std::runtime_error("SCANS does not hold N scans of RINGS x COLS points");}
    lfx::FeatureExtraction extraction(lfx::HyperParameters(), 0, per, cols, rings, 0);
    lfx::Odometry odometry(extraction);
    lfx_segment_config config = lfx::FeatureExtraction::DefaultSegmentConfig();
    config.n_rows = rings;
    config.n_columns = cols;
    config.ground_last_row = rings / 2u - 1u;            // the lower half of the beams can see the road
    // one scan's classes, filtered clouds and tables in pinned memory: the device writes it, the host reads it once the
    // stream has passed (BatchStatus), and the odometry's kernels read the clouds from there
    std::uint8_t * classes = reinterpret_cast<std::uint8_t *>(extraction.PinnedFloats((per + 3u) / 4u));
    float * edge = extraction.PinnedFloats(4u * static_cast<std::size_t>(per));
    float * surface = extraction.PinnedFloats(4u * static_cast<std::size_t>(per));
    std::uint32_t * offsets = reinterpret_cast<std::uint32_t *>(extraction.PinnedFloats(4));      // [2][1 + 1]
    std::FILE * out = std::fopen(argv[5], "wb");
    if (!out) {throw std::runtime_error("cannot open the output file");}
    for (std::uint32_t k = 0; k < n; k++) {
      extraction.ExtractFeaturesView(scans.data() + static_cast<std::size_t>(k) * per, per);
      extraction.Segment(config, 1, classes);
      extraction.PackFeaturesSegmented(classes, edge, surface, offsets, per);
      extraction.BatchStatus();          // (all three are queued; the host reads the classes and the table below)
      std::uint32_t by_class[4] = {0u, 0u, 0u, 0u};
      for (std::uint32_t i = 0; i < per; i++) {by_class[classes[i] & 3u]++;}
      const std::uint32_t kept[2] = {offsets[1], offsets[3]};
      const lfx_odometry_result r = odometry.UpdateDevice(edge, kept[0], surface, kept[1]);
      std::fwrite(by_class, sizeof(std::uint32_t), 4, out);
      std::fwrite(kept, sizeof(std::uint32_t), 2, out);
      std::fwrite(r.align.pose, sizeof(double), 12, out);
      std::fwrite(&r.align.error, sizeof(double), 1, out);
      std::fwrite(&r.align.error_scale, sizeof(double), 1, out);
      std::fwrite(&r.align.iteration, sizeof(std::int32_t), 1, out);
      std::fwrite(&r.align.code, sizeof(std::int32_t), 1, out);
      const std::int32_t aligned = r.aligned;
      std::fwrite(&aligned, sizeof(std::int32_t), 1, out);
      const std::vector<double> p = odometry.CurrentPose();
      std::printf("scan %u: none %u, ground %u, segment %u, clutter %u; %u edge and %u surface features kept; t = (%.4f, %.4f, %.4f)\n", k,
        by_class[0], by_class[1], by_class[2], by_class[3], kept[0], kept[1], p[3], p[7], p[11]);
    }
    std::fclose(out);
    std::printf("segmented odometry: %u scans\n", n);
    return 0;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "segment_scan: %s\n", e.what());
    return 1;
  }
}
