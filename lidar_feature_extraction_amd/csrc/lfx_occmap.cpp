// lfx_occmap.cpp -- lfx_occupancy_write_map (include/lfx.h, the occupancy section): an int8 occupancy grid as the map.pgm /
// map.yaml pair map_server reads.  Host only, no HIP header: tests/test_occupancy_files.py builds this file alone under
// sanitizers.
#include "../../include/lfx.h"

#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

extern "C" int lfx_occupancy_write_map(const char * dirname, const int8_t * grid, uint32_t w, uint32_t h, float resolution, double origin_x,
  double origin_y, int occupied_percent, int free_percent)
{
  if (!dirname || !grid) {return LFX_ERR_INVALID_ARGUMENT;}
  if (w < 1u || w > LFX_OCCUPANCY_MAX_SIDE || h < 1u || h > LFX_OCCUPANCY_MAX_SIDE) {return LFX_ERR_INVALID_ARGUMENT;}
  if (!std::isfinite(resolution) || !(resolution > 0.0f) || !std::isfinite(origin_x) || !std::isfinite(origin_y)) {return LFX_ERR_INVALID_ARGUMENT;}
  if (free_percent < 0 || !(free_percent < occupied_percent) || occupied_percent > 100) {return LFX_ERR_INVALID_ARGUMENT;}
  const std::string dir(dirname);
  const std::string sep = (!dir.empty() && dir.back() == '/') ? "" : "/";

  // map.pgm: P5, maxval 255, the top row the highest y
  std::FILE * f = std::fopen((dir + sep + "map.pgm").c_str(), "wb");
  if (!f) {return LFX_ERR_FILE;}
  bool ok = std::fprintf(f, "P5\n%u %u\n255\n", w, h) > 0;
  std::vector<unsigned char> row(w);
  for (uint32_t y = h; ok && y-- > 0u; ) {
    const int8_t * src = grid + (size_t)y * w;
    for (uint32_t x = 0; x < w; x++) {
      const int v = src[x];
      row[x] = v == -1 ? 205 : (v >= occupied_percent ? 0 : (v <= free_percent ? 254 : 205));
    }
    ok = std::fwrite(row.data(), 1, w, f) == w;
  }
  ok = (std::fclose(f) == 0) && ok;
  if (!ok) {return LFX_ERR_FILE;}

  f = std::fopen((dir + sep + "map.yaml").c_str(), "wb");
  if (!f) {return LFX_ERR_FILE;}
  ok = std::fprintf(f, "image: map.pgm\nresolution: %.17g\norigin: [%.17g, %.17g, 0.0]\nnegate: 0\noccupied_thresh: %.17g\nfree_thresh: %.17g\n",
      (double)resolution, origin_x, origin_y, (double)occupied_percent / 100.0, (double)free_percent / 100.0) > 0;
  ok = (std::fclose(f) == 0) && ok;
  return ok ? LFX_OK : LFX_ERR_FILE;
}
