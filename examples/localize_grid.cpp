// localize_grid.cpp -- "where am I in this occupancy grid?" without ROS: the scans of a map are extracted, reduced to virtual
// 2-D scans and rendered into a grid (lfx::OccupancyGrid), the grid's distance field becomes a score field
// (lfx::DistanceField, lfx::GridMatcher::SetField), and a scan taken in that map is searched for from a centre that is a few
// cells and heading steps wrong (lfx::GridMatcher::Search).  The pose found, lifted to 3-D (lfx::GridMatcher::Pose3), is the
// initial pose lfx::Localizer refines against the map's feature clouds.
//
//   localize_grid SCANS RINGS COLS N POSES QUERY BEAMS WIDTH HEIGHT RESOLUTION ORIGIN_X ORIGIN_Y DX DY DT THETA_STEP OUT
//     SCANS .. ORIGIN_Y   as examples/occupancy_map.cpp
//     QUERY               the scan of SCANS that is searched for: its own pose in POSES is the truth
//     DX DY DT            how far the search's centre is off: cells, cells, heading steps of THETA_STEP radians
//     OUT                 uint32 {score, index, inside, n_points}, then 3 doubles centre, 3 doubles the pose found, 12 doubles
//                         its lift, 12 doubles the refined pose, int32 the alignment's code
//   The live scan goes through a second grid of 1 x 1 cells that only reduces scans to beams: Truncate(0), Add, SetScans.
//   tests/test_grid_match_cpp_gpu.py compares with the Python binding and the restatement.
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

// a scan's feature records (4 floats each) moved into the map's frame and appended
void append_world(std::vector<float> & map, const float * points, std::uint32_t n, const double * pose)
{
  for (std::uint32_t i = 0; i < n; i++) {
    const double x = points[4u * i], y = points[4u * i + 1u], z = points[4u * i + 2u];
    for (int r = 0; r < 3; r++) {map.push_back(static_cast<float>(pose[4 * r] * x + pose[4 * r + 1] * y + pose[4 * r + 2] * z + pose[4 * r + 3]));}
    map.push_back(0.0f);
  }
}
}  // namespace

int main(int argc, char ** argv)
{
  try {
    if (argc != 18) {
      std::fprintf(stderr, "usage: localize_grid SCANS RINGS COLS N POSES QUERY BEAMS WIDTH HEIGHT RESOLUTION ORIGIN_X ORIGIN_Y DX DY DT THETA_STEP OUT\n");
      return 2;
    }
    const std::vector<lfx::PointXYZIR> scans = slurp(argv[1]);
    const std::uint32_t rings = static_cast<std::uint32_t>(std::stoul(argv[2])), cols = static_cast<std::uint32_t>(std::stoul(argv[3]));
    const std::uint32_t n = static_cast<std::uint32_t>(std::stoul(argv[4])), per = rings * cols;
    if (n == 0u || scans.size() != static_cast<std::size_t>(n) * per) {throw std::runtime_error("SCANS does not hold N scans of RINGS x COLS points");}
    const std::vector<double> poses = read_poses(argv[5], n);
    const std::uint32_t query = static_cast<std::uint32_t>(std::stoul(argv[6]));
    if (query >= n) {throw std::runtime_error("QUERY is no scan of SCANS");}
    lfx_occupancy_config config = lfx::OccupancyGrid::DefaultConfig();
    config.max_scans = n;
    config.n_beams = static_cast<std::uint32_t>(std::stoul(argv[7]));
    config.width = static_cast<std::uint32_t>(std::stoul(argv[8]));
    config.height = static_cast<std::uint32_t>(std::stoul(argv[9]));
    config.resolution = std::strtof(argv[10], nullptr);
    config.origin_x = std::strtod(argv[11], nullptr);
    config.origin_y = std::strtod(argv[12], nullptr);
    const int off_x = std::atoi(argv[13]), off_y = std::atoi(argv[14]), off_t = std::atoi(argv[15]);
    const double theta_step = std::strtod(argv[16], nullptr);

    // the map: the grid's scans, and the feature clouds the 3-D alignment runs against
    lfx::FeatureExtraction extraction(lfx::HyperParameters(), 0, per, cols, rings, 0);
    lfx::OccupancyGrid grid(extraction, config);
    std::vector<float> edge_map, surface_map;
    for (std::uint32_t k = 0; k < n; k++) {
      const lfx_scan_result view = extraction.ExtractFeaturesView(scans.data() + static_cast<std::size_t>(k) * per, per);
      append_world(edge_map, view.edge_points, view.n_edge, poses.data() + 12u * k);
      append_world(surface_map, view.surface_points, view.n_surface, poses.data() + 12u * k);
      const std::vector<double> pose(poses.begin() + 12u * k, poses.begin() + 12u * (k + 1u));
      if (grid.Add(pose) != k) {throw std::runtime_error("scan ids out of step");}
      extraction.BatchStatus();          // (the add reads the scan's records on the device: it has passed before the next scan overwrites them)
    }
    grid.RenderAll();
    lfx::DistanceField field(extraction, config.width, config.height);
    field.FromOccupancy(grid);
    lfx_grid_match_config match = lfx::GridMatcher::DefaultConfig();
    match.width = config.width; match.height = config.height;
    match.resolution = config.resolution;
    match.origin_x = config.origin_x; match.origin_y = config.origin_y;
    match.max_scans = 1;
    match.max_beams = config.n_beams;
    lfx::GridMatcher matcher(extraction, match);
    matcher.SetField(field);

    // the live scan, reduced by a grid of one cell that holds no map: its level is the rotation an IMU would give, here the
    // true one, and no translation
    lfx_occupancy_config reduce = config;
    reduce.max_scans = 1; reduce.width = 1; reduce.height = 1;
    lfx::OccupancyGrid reducer(extraction, reduce);
    const double * truth = poses.data() + 12u * query;
    std::vector<double> level_pose(truth, truth + 12);
    level_pose[3] = level_pose[7] = level_pose[11] = 0.0;
    extraction.ExtractFeaturesView(scans.data() + static_cast<std::size_t>(query) * per, per);
    reducer.Truncate(0);
    reducer.Add(level_pose);
    matcher.SetScans(reducer, 0, 1);

    // the search, from a centre that is off; a level that is a pure yaw would make the truth's heading 0 -- the level above
    // holds the truth's whole rotation, so the heading searched for is 0
    lfx_grid_match_search_config search = lfx::GridMatcher::DefaultSearchConfig();
    search.half_x = static_cast<std::uint32_t>(std::abs(off_x)) + 2u;
    search.half_y = static_cast<std::uint32_t>(std::abs(off_y)) + 2u;
    search.half_theta = static_cast<std::uint32_t>(std::abs(off_t)) + 1u;
    search.theta_step = theta_step;
    const std::array<double, 3> centre = {truth[3] + off_x * static_cast<double>(config.resolution), truth[7] + off_y * static_cast<double>(config.resolution),
      off_t * theta_step};
    std::uint32_t * best = reinterpret_cast<std::uint32_t *>(extraction.PinnedFloats(4));
    matcher.Search(0, std::vector<double>(centre.begin(), centre.end()), search, best);
    extraction.BatchStatus();
    const std::array<double, 3> found = lfx::GridMatcher::Candidate(search, config.resolution, centre, best[1]);
    std::printf("searched from (%.3f, %.3f, %.4f rad): score %u of %u points (%u inside), candidate %u\n", centre[0], centre[1], centre[2], best[0],
      best[3], best[2], best[1]);
    std::printf("pose found: x %.3f y %.3f yaw %.4f rad; truth: x %.3f y %.3f\n", found[0], found[1], found[2], truth[3], truth[7]);
    double level[9];
    for (int r = 0; r < 3; r++) {
      for (int k = 0; k < 3; k++) {level[3 * r + k] = truth[4 * r + k];}
    }
    const std::array<double, 12> initial = lfx::GridMatcher::Pose3(found, level, truth[11]);

    // the 3-D alignment from that pose (the live scan's clouds are still on the device)
    lfx::Localizer localizer(extraction, edge_map, surface_map, 20, 1.0f);
    localizer.Init(initial.data());
    const bool ok = localizer.Update();
    const lfx_align_result & r = localizer.Result();
    std::printf("update %s: iteration %d, %s; refined t = %.4f %.4f %.4f\n", ok ? "succeeded" : "failed", r.iteration, lfx_align_message(r.code), r.pose[3],
      r.pose[7], r.pose[11]);
    std::FILE * out = std::fopen(argv[17], "wb");
    if (!out) {throw std::runtime_error("cannot open the output file");}
    std::fwrite(best, sizeof(std::uint32_t), 4, out);
    std::fwrite(centre.data(), sizeof(double), 3, out);
    std::fwrite(found.data(), sizeof(double), 3, out);
    std::fwrite(initial.data(), sizeof(double), 12, out);
    std::fwrite(r.pose, sizeof(double), 12, out);
    std::fwrite(&r.code, sizeof(std::int32_t), 1, out);
    std::fclose(out);
    return 0;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "localize_grid: %s\n", e.what());
    return 1;
  }
}
