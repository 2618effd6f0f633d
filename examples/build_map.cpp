// build_map.cpp -- drive -> map -> file -> localize without ROS: the scans through the extraction and lfx::Odometry, the
// odometry poses into two lfx::Mappers (the reference's mapping node, mapping/src/mapping.cpp, once for the edge clouds
// and once for the surface clouds), both maps saved as PCD files, then lfx::Localizer built from those files as the
// localization node builds it (localization/app/localization.cpp:54,78-85) and every scan localized from its odometry pose.
//
//   build_map SCANS RINGS COLS N DIR OUT
//     SCANS   N scans of RINGS x COLS raw 32-byte PointXYZIR records (point_type.hpp:62-86), back to back
//     DIR     where DIR/edge.pcd and DIR/surface.pcd are written
//     OUT     per scan: the odometry pose and the localized pose (12 doubles each, [R | t]), the localization's error
//             (double), iteration, code, and the edge and surface mappers' outcomes (int32 each)
//   tests/test_mapping_cpp_gpu.py compares files and poses with the library's Python binding.
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
    if (argc < 7) {
      std::fprintf(stderr, "usage: build_map SCANS RINGS COLS N DIR OUT\n");
      return 2;
    }
    const std::vector<lfx::PointXYZIR> scans = slurp(argv[1]);
    const std::uint32_t rings = static_cast<std::uint32_t>(std::stoul(argv[2])), cols = static_cast<std::uint32_t>(std::stoul(argv[3]));
    const std::uint32_t n = static_cast<std::uint32_t>(std::stoul(argv[4])), per = rings * cols;
    const std::string dir = argv[5];
    if (scans.size() != static_cast<std::size_t>(n) * per) {throw std::runtime_error("SCANS does not hold N scans of RINGS x COLS points");}
    lfx::FeatureExtraction extraction(lfx::HyperParameters(), 0, per, cols, rings, 0);
    lfx::Odometry odometry(extraction);
    lfx::Mapper edge_map(extraction), surface_map(extraction);
    std::vector<std::vector<double>> poses(n);
    std::vector<std::uint8_t> edge_outcome(n), surface_outcome(n);
    for (std::uint32_t k = 0; k < n; k++) {
      extraction.ExtractFeaturesView(scans.data() + static_cast<std::size_t>(k) * per, per);
      const lfx_odometry_result & r = odometry.Update().at(0);
      poses[k].assign(r.align.pose, r.align.pose + 12);
      // the mapping node's Callback, once per map, with the scan's clouds still on the device
      edge_outcome[k] = edge_map.Add(lfx::Mapper::kEdge, poses[k]).at(0);
      surface_outcome[k] = surface_map.Add(lfx::Mapper::kSurface, poses[k]).at(0);
    }
    const std::string edge_path = dir + "/edge.pcd", surface_path = dir + "/surface.pcd";
    if (!edge_map.Save(edge_path) || !surface_map.Save(surface_path)) {throw std::runtime_error("a map is empty");}
    const lfx_mapper_store_view ev = edge_map.View(), sv = surface_map.View();
    lfx::Localizer localizer(extraction, edge_path, surface_path, 40);    // localization.cpp:54: max_iter 40
    std::FILE * out = std::fopen(argv[6], "wb");
    if (!out) {throw std::runtime_error("cannot open the output file");}
    std::uint32_t succeeded = 0;
    for (std::uint32_t k = 0; k < n; k++) {
      extraction.ExtractFeaturesView(scans.data() + static_cast<std::size_t>(k) * per, per);
      localizer.Init(poses[k].data());
      succeeded += localizer.Update() ? 1u : 0u;
      const lfx_align_result & r = localizer.Result();
      const std::int32_t tail[4] = {r.iteration, r.code, edge_outcome[k], surface_outcome[k]};
      std::fwrite(poses[k].data(), sizeof(double), 12, out);
      std::fwrite(r.pose, sizeof(double), 12, out);
      std::fwrite(&r.error, sizeof(double), 1, out);
      std::fwrite(tail, sizeof(std::int32_t), 4, out);
    }
    std::fclose(out);
    std::printf("build_map: %u scans, %llu + %llu map points from %llu + %llu keyframes, %u localized\n", n,
      static_cast<unsigned long long>(ev.n_points), static_cast<unsigned long long>(sv.n_points),
      static_cast<unsigned long long>(ev.n_added), static_cast<unsigned long long>(sv.n_added), succeeded);
    return 0;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "build_map: %s\n", e.what());
    return 1;
  }
}
