// odometry_scans.cpp -- odometry without ROS: lfx::Odometry (the reference's Odometry over EdgeSurfaceMap,
// localization/include/lidar_feature_localization/odometry.hpp:43-71) fed scan by scan.
//
//   odometry_scans SCANS RINGS COLS N OUT
//     SCANS   N scans of RINGS x COLS raw 32-byte PointXYZIR records (point_type.hpp:62-86), back to back
//     OUT     per scan two records of 12 doubles pose [R | t], error, error_scale (doubles), iteration, code, aligned
//             (int32): first the odometry fed with the extraction's own device clouds (Update()), then a second odometry
//             fed with the clouds as a separate subscriber would receive them (Update(edge, surface))
//   tests/test_odometry_cpp_gpu.py compares both with the library's Python binding.
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

void put(std::FILE * f, const lfx_odometry_result & r)
{
  std::fwrite(r.align.pose, sizeof(double), 12, f);
  std::fwrite(&r.align.error, sizeof(double), 1, f);
  std::fwrite(&r.align.error_scale, sizeof(double), 1, f);
  std::fwrite(&r.align.iteration, sizeof(std::int32_t), 1, f);
  std::fwrite(&r.align.code, sizeof(std::int32_t), 1, f);
  std::fwrite(&r.aligned, sizeof(std::int32_t), 1, f);
}
}  // namespace

int main(int argc, char ** argv)
{
  try {
    if (argc < 6) {
      std::fprintf(stderr, "usage: odometry_scans SCANS RINGS COLS N OUT\n");
      return 2;
    }
    const std::vector<lfx::PointXYZIR> scans = slurp(argv[1]);
    const std::uint32_t rings = static_cast<std::uint32_t>(std::stoul(argv[2])), cols = static_cast<std::uint32_t>(std::stoul(argv[3]));
    const std::uint32_t n = static_cast<std::uint32_t>(std::stoul(argv[4])), per = rings * cols;
    if (scans.size() != static_cast<std::size_t>(n) * per) {throw std::runtime_error("SCANS does not hold N scans of RINGS x COLS points");}
    lfx::FeatureExtraction extraction(lfx::HyperParameters(), 0, per, cols, rings, 0);
    lfx::Odometry on_device(extraction), from_host(extraction);
    std::FILE * out = std::fopen(argv[5], "wb");
    if (!out) {throw std::runtime_error("cannot open the output file");}
    for (std::uint32_t k = 0; k < n; k++) {
      // the node's order of things: features of the scan, then the pose from them
      const lfx_scan_result view = extraction.ExtractFeaturesView(scans.data() + static_cast<std::size_t>(k) * per, per);
      const lfx_odometry_result r = on_device.Update().at(0);
      put(out, r);
      std::vector<float> edge(view.edge_points, view.edge_points + 4 * static_cast<std::size_t>(view.n_edge));
      std::vector<float> surface(view.surface_points, view.surface_points + 4 * static_cast<std::size_t>(view.n_surface));
      put(out, from_host.Update(edge.data(), view.n_edge, surface.data(), view.n_surface));
    }
    std::fclose(out);
    const std::vector<double> pose = on_device.CurrentPose();
    std::printf("odometry: %u scans, last pose t = (%.4f, %.4f, %.4f)\n", n, pose[3], pose[7], pose[11]);
    return 0;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "odometry_scans: %s\n", e.what());
    return 1;
  }
}
