// lfx_distmap.cpp -- the host side of the distance section (include/lfx.h) that needs no device: the two default configs and
// the cost table, the only source of the inflation decay -- the device is handed these bytes.  Host only, no HIP header:
// tests/test_distance_expect.py builds this file alone under sanitizers.
#include "../../include/lfx.h"

#include <cmath>

namespace
{
bool cost_config_ok(const lfx_distance_cost_config & c, float resolution)
{
  if (!std::isfinite(resolution) || !(resolution > 0.0f)) {return false;}
  if (!std::isfinite(c.inscribed_radius) || !(c.inscribed_radius >= 0.0f)) {return false;}
  if (!std::isfinite(c.inflation_radius) || !(c.inflation_radius >= c.inscribed_radius)) {return false;}
  if (!std::isfinite(c.cost_scaling_factor) || !(c.cost_scaling_factor >= 0.0f)) {return false;}
  return c.track_unknown <= 1u;
}
}  // namespace

extern "C" {

void lfx_distance_default_config(lfx_distance_config * config)
{
  if (!config) {return;}
  *config = lfx_distance_config{};
  config->occupied_percent = 65;
}

void lfx_distance_cost_default_config(lfx_distance_cost_config * config)
{
  if (!config) {return;}
  *config = lfx_distance_cost_config{};
  config->inscribed_radius = 0.22f;
  config->inflation_radius = 0.55f;
  config->cost_scaling_factor = 10.0f;
  config->track_unknown = 1u;
}

int lfx_distance_cost_table_size(const lfx_distance_cost_config * config, float resolution, uint32_t * n)
{
  if (!config || !n) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!cost_config_ok(*config, resolution)) {return LFX_ERR_INVALID_ARGUMENT;}
  const double cells = std::ceil((double)config->inflation_radius / (double)resolution);
  if (!(cells <= (double)LFX_DISTANCE_MAX_COST_CELLS)) {return LFX_ERR_INVALID_ARGUMENT;}
  const uint32_t rc = (uint32_t)cells;
  *n = rc * rc + 1u;
  return LFX_OK;
}

int lfx_distance_cost_table(const lfx_distance_cost_config * config, float resolution, uint8_t * lut, uint32_t n)
{
  uint32_t want = 0;
  if (!lut) {return LFX_ERR_INVALID_ARGUMENT;}
  if (lfx_distance_cost_table_size(config, resolution, &want) != LFX_OK || n != want) {return LFX_ERR_INVALID_ARGUMENT;}
  const double res = (double)resolution, inscribed = (double)config->inscribed_radius, inflation = (double)config->inflation_radius;
  const double scaling = (double)config->cost_scaling_factor;
  lut[0] = 254;
  for (uint32_t k = 1; k < n; k++) {
    const double d = std::sqrt((double)k) * res;
    if (d <= inscribed) {
      lut[k] = 253;
    } else if (d > inflation) {
      lut[k] = 0;
    } else {
      lut[k] = (uint8_t)(252.0 * std::exp(-scaling * (d - inscribed)));     // (nav2's expression; at most 252.0, truncated)
    }
  }
  return LFX_OK;
}

}  // extern "C"
