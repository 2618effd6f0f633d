// costmap.cpp -- from scans to what a grid planner searches, without ROS: every scan is extracted and reduced to a virtual 2-D
// scan kept on the device (lfx::OccupancyGrid::Add), the grid is rendered, its distance field is taken from the counts in
// place (lfx::DistanceField::FromOccupancy) and turned into nav2's inflated costmap; then the poses move -- what a pose graph
// does after a loop closure -- the grid is rendered again from the kept beams and one more FromOccupancy refreshes the costmap.
//
//   costmap SCANS RINGS COLS N POSES MOVED OUT BEAMS WIDTH HEIGHT RESOLUTION ORIGIN_X ORIGIN_Y MAX_CELLS
//     SCANS .. ORIGIN_Y   as examples/occupancy_map.cpp
//     MAX_CELLS           lfx_distance_config's max_cells (0: uncapped)
//     OUT     OUT/first/grid.bin: the emitted int8 grid, row 0 the lowest y; OUT/first/costmap.pgm: P5, maxval 255, the top row
//             the highest y, the cost of every cell as its grey value; OUT/second/...: at MOVED
//   The stats of both transforms are printed.  tests/test_distance_cpp_gpu.py reads them and the four files.
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <fstream>
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

void write_all(const std::string & path, const std::string & head, const std::uint8_t * rows, std::uint32_t w, std::uint32_t h, bool top_first)
{
  std::FILE * f = std::fopen(path.c_str(), "wb");
  if (!f) {throw std::runtime_error("cannot write " + path);}
  bool ok = head.empty() || std::fwrite(head.data(), 1, head.size(), f) == head.size();
  for (std::uint32_t k = 0; ok && k < h; k++) {
    const std::uint32_t y = top_first ? h - 1u - k : k;
    ok = std::fwrite(rows + static_cast<std::size_t>(y) * w, 1, w, f) == w;
  }
  ok = (std::fclose(f) == 0) && ok;
  if (!ok) {throw std::runtime_error("cannot write " + path);}
}
}  // namespace

int main(int argc, char ** argv)
{
  try {
    if (argc != 15) {
      std::fprintf(stderr, "usage: costmap SCANS RINGS COLS N POSES MOVED OUT BEAMS WIDTH HEIGHT RESOLUTION ORIGIN_X ORIGIN_Y MAX_CELLS\n");
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
    lfx_distance_config transform = lfx::DistanceField::DefaultConfig();
    transform.max_cells = static_cast<std::uint32_t>(std::stoul(argv[14]));

    lfx::FeatureExtraction extraction(lfx::HyperParameters(), 0, per, cols, rings, 0);
    lfx::OccupancyGrid grid(extraction, config);
    lfx::DistanceField field(extraction, config.width, config.height);
    for (std::uint32_t k = 0; k < n; k++) {
      extraction.ExtractFeaturesView(scans.data() + static_cast<std::size_t>(k) * per, per);
      const std::vector<double> pose(poses.begin() + 12u * k, poses.begin() + 12u * (k + 1u));
      if (grid.Add(pose) != k) {throw std::runtime_error("scan ids out of step");}
      extraction.BatchStatus();          // (the add reads the scan's records on the device: it has passed before the next scan overwrites them)
    }
    // one pinned block: the emitted grid, then the costs (a float holds four cells of either)
    const std::size_t cells = static_cast<std::size_t>(config.width) * config.height, quarter = (cells + 3u) / 4u;
    float * block = extraction.PinnedFloats(2u * quarter);
    std::int8_t * cells_out = reinterpret_cast<std::int8_t *>(block);
    std::uint8_t * cost_out = reinterpret_cast<std::uint8_t *>(block + quarter);
    const std::string head = "P5\n" + std::to_string(config.width) + " " + std::to_string(config.height) + "\n255\n";

    for (int pass = 0; pass < 2; pass++) {
      const std::string dir = out + (pass == 0 ? "/first" : "/second");
      std::filesystem::create_directories(dir);
      if (pass == 1) {grid.SetPoses(0, moved);}           // the correction: the poses move, the beams stay
      grid.RenderAll();
      field.FromOccupancy(grid, transform);
      field.Costmap(config.resolution, cost_out);
      grid.Emit(cells_out);
      const lfx_distance_stats_t s = field.Stats();       // (synchronous: the two outputs above have landed behind it)
      std::printf("%s transform: %llu obstacle cells, %llu unknown cells, %llu far cells, max d2 %llu\n", pass == 0 ? "first" : "second",
        static_cast<unsigned long long>(s.n_obstacle), static_cast<unsigned long long>(s.n_unknown), static_cast<unsigned long long>(s.n_far),
        static_cast<unsigned long long>(s.max_d2));
      write_all(dir + "/grid.bin", "", reinterpret_cast<const std::uint8_t *>(cells_out), config.width, config.height, false);
      write_all(dir + "/costmap.pgm", head, cost_out, config.width, config.height, true);
    }
    return 0;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "costmap: %s\n", e.what());
    return 1;
  }
}
