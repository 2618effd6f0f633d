// lfx_gridmatchmap.cpp -- the host side of the grid-match section (include/lfx.h) that needs no device: the default configs,
// the score table (the only source of the likelihood's decay -- the device is handed these bytes), the search's sizes and
// rotations (the only source of the cosines and sines), and a candidate's pose in 2-D and 3-D.  Host only, no HIP header:
// tests/test_grid_match_expect.py builds this file alone under sanitizers.
#include "../../include/lfx.h"

#include <cmath>

namespace
{
bool table_config_ok(const lfx_grid_match_table_config & c, float resolution)
{
  if (!std::isfinite(resolution) || !(resolution > 0.0f)) {return false;}
  if (!std::isfinite(c.sigma) || !(c.sigma > 0.0f)) {return false;}
  if (!std::isfinite(c.max_distance) || !(c.max_distance >= 0.0f)) {return false;}
  return c.peak >= 1u && c.peak <= 65535u && c.reserved == 0u;
}

bool rotations_ok(double yaw0, uint32_t half_theta, double theta_step)
{
  if (!std::isfinite(yaw0) || half_theta > LFX_GRID_MATCH_MAX_HALF_THETA) {return false;}
  return half_theta == 0u || (std::isfinite(theta_step) && theta_step > 0.0);
}

double angle_of(double yaw0, uint32_t half_theta, double theta_step, uint32_t j)
{
  // (with half_theta == 0 the step is not inspected and takes no part: the one heading is yaw0 itself)
  if (half_theta == 0u) {return yaw0;}
  return yaw0 + (double)((int32_t)j - (int32_t)half_theta) * theta_step;
}
}  // namespace

extern "C" {

void lfx_grid_match_default_config(lfx_grid_match_config * config)
{
  if (!config) {return;}
  *config = lfx_grid_match_config{};
  config->max_scans = 64;
  config->max_beams = 1800;
  config->max_half_x = 50;
  config->max_half_y = 50;
  config->max_half_theta = 30;
}

void lfx_grid_match_table_default_config(lfx_grid_match_table_config * config)
{
  if (!config) {return;}
  *config = lfx_grid_match_table_config{};
  config->sigma = 0.2f;
  config->max_distance = 2.0f;
  config->peak = 1000u;
}

void lfx_grid_match_search_default_config(lfx_grid_match_search_config * config)
{
  if (!config) {return;}
  *config = lfx_grid_match_search_config{};
  config->half_x = 10;
  config->half_y = 10;
  config->step_cells = 1;
}

int lfx_grid_match_table_size(const lfx_grid_match_table_config * config, float resolution, uint32_t * n)
{
  if (!config || !n) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!table_config_ok(*config, resolution)) {return LFX_ERR_INVALID_ARGUMENT;}
  const double cells = std::ceil((double)config->max_distance / (double)resolution);
  if (!(cells <= (double)LFX_GRID_MATCH_MAX_CELLS)) {return LFX_ERR_INVALID_ARGUMENT;}
  const uint32_t rs = (uint32_t)cells;
  *n = rs * rs + 1u;
  return LFX_OK;
}

int lfx_grid_match_table(const lfx_grid_match_table_config * config, float resolution, uint16_t * lut, uint32_t n)
{
  uint32_t want = 0;
  if (!lut) {return LFX_ERR_INVALID_ARGUMENT;}
  if (lfx_grid_match_table_size(config, resolution, &want) != LFX_OK || n != want) {return LFX_ERR_INVALID_ARGUMENT;}
  const double res = (double)resolution, sigma = (double)config->sigma, reach = (double)config->max_distance, peak = (double)config->peak;
  const double denom = (2.0 * sigma) * sigma;
  for (uint32_t k = 0; k < n; k++) {
    const double d = std::sqrt((double)k) * res;
    if (d > reach) {
      lut[k] = 0;
    } else {
      lut[k] = (uint16_t)std::rint(peak * std::exp(-(d * d) / denom));       // (at most peak <= 65535)
    }
  }
  return LFX_OK;
}

int lfx_grid_match_search_size(const lfx_grid_match_search_config * search, uint32_t dims[3])
{
  if (!search || !dims) {return LFX_ERR_INVALID_ARGUMENT;}
  if (search->half_x > LFX_GRID_MATCH_MAX_HALF || search->half_y > LFX_GRID_MATCH_MAX_HALF) {return LFX_ERR_INVALID_ARGUMENT;}
  if (search->step_cells < 1u || search->step_cells > 16u) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!rotations_ok(0.0, search->half_theta, search->theta_step)) {return LFX_ERR_INVALID_ARGUMENT;}
  dims[0] = 2u * search->half_x + 1u;
  dims[1] = 2u * search->half_y + 1u;
  dims[2] = 2u * search->half_theta + 1u;
  return LFX_OK;
}

int lfx_grid_match_rotations(double yaw0, uint32_t half_theta, double theta_step, double * cs)
{
  if (!cs || !rotations_ok(yaw0, half_theta, theta_step)) {return LFX_ERR_INVALID_ARGUMENT;}
  const uint32_t T = 2u * half_theta + 1u;
  for (uint32_t j = 0; j < T; j++) {
    const double a = angle_of(yaw0, half_theta, theta_step, j);
    cs[2u * j] = std::cos(a);
    cs[2u * j + 1u] = std::sin(a);
  }
  return LFX_OK;
}

int lfx_grid_match_candidate(const lfx_grid_match_search_config * search, float resolution, const double centre[3], uint32_t index, double pose2[3])
{
  uint32_t dims[3];
  if (!centre || !pose2) {return LFX_ERR_INVALID_ARGUMENT;}
  if (lfx_grid_match_search_size(search, dims) != LFX_OK) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!std::isfinite(resolution) || !std::isfinite(centre[0]) || !std::isfinite(centre[1]) || !std::isfinite(centre[2])) {return LFX_ERR_INVALID_ARGUMENT;}
  if ((uint64_t)index >= (uint64_t)dims[0] * dims[1] * dims[2]) {return LFX_ERR_INVALID_ARGUMENT;}
  const uint32_t ix = index % dims[0], iy = (index / dims[0]) % dims[1], j = index / (dims[0] * dims[1]);
  const int32_t kx = ((int32_t)ix - (int32_t)search->half_x) * (int32_t)search->step_cells;
  const int32_t ky = ((int32_t)iy - (int32_t)search->half_y) * (int32_t)search->step_cells;
  pose2[0] = centre[0] + (double)kx * (double)resolution;
  pose2[1] = centre[1] + (double)ky * (double)resolution;
  pose2[2] = angle_of(centre[2], search->half_theta, search->theta_step, j);
  return LFX_OK;
}

int lfx_grid_match_pose3(const double pose2[3], const double * level, double z, double pose[12])
{
  if (!pose2 || !pose) {return LFX_ERR_INVALID_ARGUMENT;}
  static const double identity[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  const double * l = level ? level : identity;
  const double c = std::cos(pose2[2]), s = std::sin(pose2[2]);
  const double rz[9] = {c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0};
  for (int r = 0; r < 3; r++) {
    for (int k = 0; k < 3; k++) {
      pose[4 * r + k] = (rz[3 * r] * l[k] + rz[3 * r + 1] * l[3 + k]) + rz[3 * r + 2] * l[6 + k];
    }
  }
  pose[3] = pose2[0];
  pose[7] = pose2[1];
  pose[11] = z;
  return LFX_OK;
}

}  // extern "C"
