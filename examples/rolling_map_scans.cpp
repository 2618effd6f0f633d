// rolling_map_scans.cpp -- a SLAM front end without ROS: lfx::Odometry (scan to the last 7 scans) chained into
// lfx::RollingMap (scan to the rolling voxel map), scan by scan.  The odometry's pose of a scan goes in as the mapping
// stage's odometry pose; the map corrects it against everything its window still holds.
//
//   rolling_map_scans SCANS RINGS COLS N OUT
//     SCANS   N scans of RINGS x COLS raw 32-byte PointXYZIR records (point_type.hpp:62-86), back to back
//     OUT     per scan two records of 12 doubles pose [R | t], error, error_scale (doubles), iteration, code, aligned
//             (int32): first the odometry's, then the rolling map's
//   Both trajectories are printed.  tests/test_rolling_map_cpp_gpu.py compares them with the library's Python binding.
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

void put(std::FILE * f, const lfx_align_result & r, std::int32_t aligned)
{
  std::fwrite(r.pose, sizeof(double), 12, f);
  std::fwrite(&r.error, sizeof(double), 1, f);
  std::fwrite(&r.error_scale, sizeof(double), 1, f);
  std::fwrite(&r.iteration, sizeof(std::int32_t), 1, f);
  std::fwrite(&r.code, sizeof(std::int32_t), 1, f);
  std::fwrite(&aligned, sizeof(std::int32_t), 1, f);
}
}  // namespace

int main(int argc, char ** argv)
{
  try {
    if (argc < 6) {
      std::fprintf(stderr, "usage: rolling_map_scans SCANS RINGS COLS N OUT\n");
      return 2;
    }
    const std::vector<lfx::PointXYZIR> scans = slurp(argv[1]);
    const std::uint32_t rings = static_cast<std::uint32_t>(std::stoul(argv[2])), cols = static_cast<std::uint32_t>(std::stoul(argv[3]));
    const std::uint32_t n = static_cast<std::uint32_t>(std::stoul(argv[4])), per = rings * cols;
    if (scans.size() != static_cast<std::size_t>(n) * per) {throw std::runtime_error("SCANS does not hold N scans of RINGS x COLS points");}
    lfx::FeatureExtraction extraction(lfx::HyperParameters(), 0, per, cols, rings, 0);
    lfx::Odometry odometry(extraction);
    lfx::RollingMap map(extraction);
    std::FILE * out = std::fopen(argv[5], "wb");
    if (!out) {throw std::runtime_error("cannot open the output file");}
    for (std::uint32_t k = 0; k < n; k++) {
      extraction.ExtractFeaturesView(scans.data() + static_cast<std::size_t>(k) * per, per);
      const lfx_odometry_result o = odometry.Update().at(0);
      const std::vector<double> odometry_pose(o.align.pose, o.align.pose + 12);
      const lfx_rolling_map_result m = map.Update(odometry_pose).at(0);
      put(out, o.align, o.aligned);
      put(out, m.align, m.aligned);
      // a scan the map could not place keeps its initial pose (lfx_rolling_map_pose), not the failed alignment's
      const std::vector<double> p = map.CurrentPose();
      std::printf("scan %u: odometry t = (%.4f, %.4f, %.4f)  map t = (%.4f, %.4f, %.4f)%s\n", k, o.align.pose[3], o.align.pose[7],
        o.align.pose[11], p[3], p[7], p[11], m.recentered ? "  [recentred]" : "");
    }
    std::fclose(out);
    const lfx_rolling_map_view_t v = map.View();
    std::printf("rolling map: %u scans, %llu edge and %llu surface voxels live\n", n, static_cast<unsigned long long>(v.n_live[0]),
      static_cast<unsigned long long>(v.n_live[1]));
    return 0;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "rolling_map_scans: %s\n", e.what());
    return 1;
  }
}
