// occupancy_map.cpp -- the map a navigation stack consumes, without ROS: every scan is extracted and reduced to a virtual 2-D
// scan kept on the device with its pose (lfx::OccupancyGrid::Add), the grid is rendered by ray casting and saved as the
// map.pgm / map.yaml pair map_server reads; then the poses move -- what a pose graph does after a loop closure -- and the
// grid is rendered again from the kept beams, no scan being read again, and saved a second time.
//
//   occupancy_map SCANS RINGS COLS N POSES MOVED OUT BEAMS WIDTH HEIGHT RESOLUTION ORIGIN_X ORIGIN_Y
//     SCANS   N scans of RINGS x COLS raw 32-byte PointXYZIR records (point_type.hpp:62-86), back to back
//     POSES   one scan per line, 12 numbers, [R | t] row-major: the poses the scans are added with
//     MOVED   the same, the poses after the correction
//     OUT     OUT/first/map.pgm, map.yaml: the grid at POSES; OUT/second/...: at MOVED
//     BEAMS .. ORIGIN_Y   lfx_occupancy_config's n_beams, width, height, resolution, origin_x, origin_y
//   The counters of both renders are printed.  tests/test_occupancy_cpp_gpu.py reads them and the four files.
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <sstream>
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

std::vector<double> read_poses(const std::string & path, std::uint32_t n)
{
  std::ifstream f(path);
  if (!f.good()) {throw std::runtime_error("cannot read " + path);}
  std::vector<double> poses;
  double v;
  while (f >> v) {poses.push_back(v);}
  if (poses.size() != 12u * static_cast<std::size_t>(n)) {throw std::runtime_error(path + " does not hold 12 numbers per scan");}
  return poses;
}

void report(const char * what, const lfx_occupancy_counters_t & r)
{
  std::printf("%s: %llu hit beams, %llu clear beams, %llu skipped, %llu occupied votes, %llu free votes, %llu outside their window\n", what,
    static_cast<unsigned long long>(r.n_hit_beams), static_cast<unsigned long long>(r.n_clear_beams), static_cast<unsigned long long>(r.n_skipped_beams),
    static_cast<unsigned long long>(r.n_occupied_votes), static_cast<unsigned long long>(r.n_free_votes), static_cast<unsigned long long>(r.n_window_miss));
}
}  // namespace

int main(int argc, char ** argv)
{
  try {
    if (argc != 14) {
      std::fprintf(stderr, "usage: occupancy_map SCANS RINGS COLS N POSES MOVED OUT BEAMS WIDTH HEIGHT RESOLUTION ORIGIN_X ORIGIN_Y\n");
      return 2;
    }
    const std::vector<lfx::PointXYZIR> scans = slurp(argv[1]);
    const std::uint32_t rings = static_cast<std::uint32_t>(std::stoul(argv[2])), cols = static_cast<std::uint32_t>(std::stoul(argv[3]));
    const std::uint32_t n = static_cast<std::uint32_t>(std::stoul(argv[4])), per = rings * cols;
    if (n == 0u || scans.size() != static_cast<std::size_t>(n) * per) {throw std::runtime_error("SCANS does not hold N scans of RINGS x COLS points");}
    const std::vector<double> poses = read_poses(argv[5], n), moved = read_poses(argv[6], n);
    const std::string out(argv[7]);
    lfx_occupancy_config config = lfx::OccupancyGrid::DefaultConfig();
    config.max_scans = n;
    config.n_beams = static_cast<std::uint32_t>(std::stoul(argv[8]));
    config.width = static_cast<std::uint32_t>(std::stoul(argv[9]));
    config.height = static_cast<std::uint32_t>(std::stoul(argv[10]));
    config.resolution = std::strtof(argv[11], nullptr);
    config.origin_x = std::strtod(argv[12], nullptr);
    config.origin_y = std::strtod(argv[13], nullptr);

    lfx::FeatureExtraction extraction(lfx::HyperParameters(), 0, per, cols, rings, 0);
    lfx::OccupancyGrid grid(extraction, config);
    for (std::uint32_t k = 0; k < n; k++) {
      extraction.ExtractFeaturesView(scans.data() + static_cast<std::size_t>(k) * per, per);
      const std::vector<double> pose(poses.begin() + 12u * k, poses.begin() + 12u * (k + 1u));
      if (grid.Add(pose) != k) {throw std::runtime_error("scan ids out of step");}
      extraction.BatchStatus();          // (the add reads the scan's records on the device: it has passed before the next scan overwrites them)
    }
    std::printf("occupancy grid: %u scans of %u beams, %u x %u cells of %g m, windows of %u cells\n", grid.Info().n_scans, config.n_beams, config.width,
      config.height, static_cast<double>(config.resolution), grid.Info().window);

    std::filesystem::create_directories(out + "/first");
    std::filesystem::create_directories(out + "/second");
    grid.RenderAll();
    report("first render", grid.Counters());
    grid.Save(out + "/first");

    // the correction: the poses move, the beams stay
    grid.SetPoses(0, moved);
    grid.RenderAll();
    report("second render", grid.Counters());
    grid.Save(out + "/second");
    return 0;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "occupancy_map: %s\n", e.what());
    return 1;
  }
}
