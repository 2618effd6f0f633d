// deskew_trajectory.cpp -- de-skewing with an IMU, without ROS: every sweep's feature clouds corrected along the sensor's
// poses within the sweep (lfx::FeatureExtraction::DeskewTrajectory: include/lfx.h, the de-skew section), the poses
// integrated from gyro samples (lfx::Trajectory::FromGyro).
//
//   deskew_trajectory SCANS RINGS COLS N [YAW] [SPEED]
//     SCANS   N sweeps of RINGS x COLS raw 32-byte PointXYZIR records (point_type.hpp:62-86) in firing order, back to back
//     YAW     the turn over one sweep in radians at its middle (0.06); the gyro's z rate runs from half of it to one and a half
//     SPEED   metres per sweep along the sensor's x at the start (1.5)
//   The 21 gyro samples of a sweep sit at the fractions j / 20 of it (index times); the records are brought to the sweep's
//   end.  Per sweep the feature counts and a checksum (the sum of the de-skewed records' floats read as 32-bit words) are
//   printed.  tests/test_trajectory_cpp_gpu.py compares them with the Python binding.
#include <cstdio>
#include <cstring>
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

std::uint64_t words(const float * records, std::uint32_t n)
{
  std::uint64_t sum = 0;
  for (std::size_t i = 0; i < 4 * static_cast<std::size_t>(n); i++) {
    std::uint32_t u;
    std::memcpy(&u, records + i, sizeof(u));
    sum += u;
  }
  return sum;
}
}  // namespace

int main(int argc, char ** argv)
{
  try {
    if (argc < 5) {
      std::fprintf(stderr, "usage: deskew_trajectory SCANS RINGS COLS N [YAW] [SPEED]\n");
      return 2;
    }
    const std::vector<lfx::PointXYZIR> scans = slurp(argv[1]);
    const std::uint32_t rings = static_cast<std::uint32_t>(std::stoul(argv[2])), cols = static_cast<std::uint32_t>(std::stoul(argv[3]));
    const std::uint32_t n = static_cast<std::uint32_t>(std::stoul(argv[4])), per = rings * cols;
    const double yaw = argc > 5 ? std::stod(argv[5]) : 0.06, speed = argc > 6 ? std::stod(argv[6]) : 1.5;
    if (scans.size() != static_cast<std::size_t>(n) * per) {throw std::runtime_error("SCANS does not hold N scans of RINGS x COLS points");}
    // what an IMU driver hands over for one sweep: 21 samples, a little roll and pitch beside the yaw
    std::vector<double> times, rates;
    for (int j = 0; j <= 20; j++) {
      const double t = j / 20.0;
      times.push_back(t);
      rates.push_back(0.02 * t);
      rates.push_back(-0.01);
      rates.push_back(yaw * (0.5 + t));
    }
    const double velocity[3] = {speed, 0.0, 0.0};
    const lfx::Trajectory trajectory = lfx::Trajectory::FromGyro(times, rates, 1.0, nullptr, velocity);
    lfx::FeatureExtraction extraction(lfx::HyperParameters(), 0, per, cols, rings, 0);
    const lfx_time_field time = lfx::TimeField::FromIndex();      // the records arrive in firing order
    std::printf("scan   edge surface   checksum\n");
    for (std::uint32_t k = 0; k < n; k++) {
      extraction.ExtractFeaturesView(scans.data() + static_cast<std::size_t>(k) * per, per);
      extraction.DeskewTrajectory(time, {trajectory});            // in place: what is read afterwards is de-skewed
      lfx_scan_result r{};
      if (lfx_download_scan(extraction.handle(), 0, nullptr, &r) != LFX_OK) {throw std::runtime_error(lfx_last_error(extraction.handle()));}
      std::printf("%4u   %4u %7u   %llu\n", k, r.n_edge, r.n_surface,
        static_cast<unsigned long long>(words(r.edge_points, r.n_edge) + words(r.surface_points, r.n_surface)));
    }
    std::printf("deskew_trajectory: %u scans\n", n);
    return 0;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "deskew_trajectory: %s\n", e.what());
    return 1;
  }
}
