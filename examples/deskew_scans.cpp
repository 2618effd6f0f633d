// deskew_scans.cpp -- odometry on a moving platform without ROS: the same sweeps through lfx::Odometry twice, as they come
// (Update()) and with every scan corrected for the sensor's motion during its sweep by the odometry's own constant-velocity
// prediction (UpdateBatchDeskewed(): include/lfx.h, the de-skew section).
//
//   deskew_scans SCANS RINGS COLS N OUT [SWEEP_RATIO]
//     SCANS        N sweeps of RINGS x COLS raw 32-byte PointXYZIR records (point_type.hpp:62-86) in firing order, back to back
//     OUT          per scan two records of 12 doubles pose [R | t], error, error_scale (doubles), iteration, code, aligned
//                  (int32): first the plain odometry, then the de-skewing one
//     SWEEP_RATIO  sweep time over scan period (1.0)
//   Both trajectories are printed, one line per scan.  tests/test_deskew_cpp_gpu.py compares them with the Python binding.
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
      std::fprintf(stderr, "usage: deskew_scans SCANS RINGS COLS N OUT [SWEEP_RATIO]\n");
      return 2;
    }
    const std::vector<lfx::PointXYZIR> scans = slurp(argv[1]);
    const std::uint32_t rings = static_cast<std::uint32_t>(std::stoul(argv[2])), cols = static_cast<std::uint32_t>(std::stoul(argv[3]));
    const std::uint32_t n = static_cast<std::uint32_t>(std::stoul(argv[4])), per = rings * cols;
    const double ratio = argc > 6 ? std::stod(argv[6]) : 1.0;
    if (scans.size() != static_cast<std::size_t>(n) * per) {throw std::runtime_error("SCANS does not hold N scans of RINGS x COLS points");}
    lfx::FeatureExtraction extraction(lfx::HyperParameters(), 0, per, cols, rings, 0);
    lfx::Odometry plain(extraction), deskewed(extraction);
    const lfx_time_field time = lfx::TimeField::FromIndex();      // the records arrive in firing order
    std::FILE * out = std::fopen(argv[5], "wb");
    if (!out) {throw std::runtime_error("cannot open the output file");}
    std::printf("scan   plain x y z                      de-skewed x y z\n");
    for (std::uint32_t k = 0; k < n; k++) {
      extraction.ExtractFeaturesView(scans.data() + static_cast<std::size_t>(k) * per, per);
      const lfx_odometry_result a = plain.Update().at(0);
      const lfx_odometry_result b = deskewed.UpdateBatchDeskewed(time, {}, ratio).at(0);   // (the batch's own clouds stay raw)
      put(out, a);
      put(out, b);
      std::printf("%4u   %9.4f %9.4f %9.4f   %9.4f %9.4f %9.4f\n", k, a.align.pose[3], a.align.pose[7], a.align.pose[11],
        b.align.pose[3], b.align.pose[7], b.align.pose[11]);
    }
    std::fclose(out);
    std::printf("deskew: %u scans\n", n);
    return 0;
  } catch (const std::exception & e) {
    std::fprintf(stderr, "deskew_scans: %s\n", e.what());
    return 1;
  }
}
