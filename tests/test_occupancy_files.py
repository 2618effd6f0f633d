"""The host-only side of the occupancy grid through the built library, no device: lfx_occupancy_write_map against the
restatement's bytes (tests/occupancy_restatement.py), the emit's look-up table and the column tables against theirs, what the
three refuse -- and lfx_occmap.cpp built alone with a small main of its own under -fsanitize=address,undefined and run as a
program, the way tests/test_map_files.py treats lfx_pcd.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from lidar_feature_extraction_amd import binding as B
from lidar_feature_extraction_amd import occupancy_emit_table, occupancy_tables, segment_tables, write_occupancy_map
from tests import occupancy_restatement as O
from tests.test_occupancy_expect import GRID_2X4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_feature_extraction_amd", "csrc")


def _files(d):
    return open(os.path.join(d, "map.pgm"), "rb").read(), open(os.path.join(d, "map.yaml"), "rb").read()


def test_write_map_is_the_restatements_bytes(tmp_path):
    rng = np.random.default_rng(11)
    cases = [(GRID_2X4, 0.5, (-12.25, 3.0), 65, 25), (rng.integers(-1, 101, (37, 53)).astype(np.int8), 0.1, (1e6 / 3, -7.7), 65, 25),
             (rng.integers(-128, 128, (5, 1)).astype(np.int8), 0.05, (0.0, 0.0), 100, 0), (np.full((1, 9), 50, np.int8), 2.0, (-1.0, 1.0), 51, 50)]
    for k, (grid, res, origin, occ, free) in enumerate(cases):
        d = tmp_path / str(k)
        d.mkdir()
        write_occupancy_map(d, grid, res, origin, occ, free)
        pgm, yaml = _files(d)
        assert pgm == O.pgm_bytes(grid, occ, free), k
        assert yaml == O.yaml_bytes(res, origin[0], origin[1], occ, free), k
    # a trailing slash, and the hand case's bytes
    write_occupancy_map(str(tmp_path / "0") + "/", GRID_2X4, 0.5, (-12.25, 3.0))
    assert _files(tmp_path / "0")[0] == b"P5\n4 2\n255\n" + bytes([205, 0, 0, 205, 205, 254, 254, 205])


def test_write_map_refuses(tmp_path):
    L = B.load()
    g = np.zeros((2, 2), np.int8)
    d = os.fsencode(str(tmp_path))
    call = lambda dirname=d, grid=g.ctypes.data, w=2, h=2, res=0.5, ox=0.0, oy=0.0, occ=65, free=25: L.lfx_occupancy_write_map(
        dirname, C.c_void_p(grid), w, h, res, ox, oy, occ, free)
    assert call() == 0
    for kw in (dict(dirname=None), dict(grid=None), dict(w=0), dict(h=0), dict(w=16385), dict(h=16385), dict(res=0.0), dict(res=-1.0),
               dict(res=float("nan")), dict(res=float("inf")), dict(ox=float("nan")), dict(oy=float("inf")), dict(occ=101), dict(free=-1),
               dict(occ=25, free=25), dict(occ=20, free=30)):
        assert call(**kw) == B.ERR_INVALID_ARGUMENT, kw
    assert call(dirname=os.fsencode(str(tmp_path / "no" / "such" / "dir"))) == B.ERR_FILE


def test_emit_table_is_the_restatements():
    for fields in ({}, dict(l_min=-2048, l_max=2048), dict(l_min=-1, l_max=0), dict(l_min=100000, l_max=100001), dict(l_min=-200000, l_max=-199000)):
        cfg = O.emit_config(**fields)
        got = occupancy_emit_table(cfg)
        assert got.dtype == np.int8 and got.tobytes() == O.emit_table(cfg).tobytes(), fields
    lut = occupancy_emit_table()
    assert (lut[0], lut[200], lut[-1]) == (12, 50, 97) and (np.diff(lut.astype(int)) >= 0).all()
    for fields in (dict(w_hit=0), dict(w_hit=1001), dict(w_miss=0), dict(w_miss=1001), dict(l_min=0, l_max=0), dict(l_min=5, l_max=4),
                   dict(l_min=-2048, l_max=2049), dict(l_min=-(1 << 31), l_max=(1 << 31) - 1), dict(min_observations=0), dict(reserved=1)):
        with pytest.raises(B.LfxError) as e:
            occupancy_emit_table(O.emit_config(**fields))
        assert e.value.code == B.ERR_INVALID_ARGUMENT, fields


GOOD = dict(n_beams=16, max_scans=4, width=8, height=8, resolution=0.5, origin_x=0.0, origin_y=0.0)


def config_refusals():
    """every field of lfx_occupancy_config outside its range, one at a time"""
    nan, inf = float("nan"), float("inf")
    return [dict(n_beams=2), dict(n_beams=17), dict(n_beams=4098), dict(max_scans=0), dict(max_scans=(1 << 24) + 1), dict(width=0), dict(width=16385),
            dict(height=0), dict(height=16385), dict(resolution=0.0), dict(resolution=-0.5), dict(resolution=nan), dict(resolution=inf),
            dict(origin_x=nan), dict(origin_y=inf), dict(min_range=0.0), dict(min_range=nan), dict(min_range=100.0), dict(max_range=65537.0),
            dict(max_range=inf), dict(z_min=nan), dict(z_max=inf), dict(z_min=1.0, z_max=0.5), dict(chunk_scans=0), dict(chunk_scans=1025),
            dict(resolution=0.001, max_range=40.0)]


def test_column_tables_are_the_segmentations():
    for W in (4, 16, 1800, 4096):
        cs, sn = occupancy_tables(dict(GOOD, n_beams=W))
        scs, ssn, _ = segment_tables(dict(n_columns=W))
        assert cs.tobytes() == scs.tobytes() and sn.tobytes() == ssn.tobytes()
    occupancy_tables(dict(GOOD, resolution=0.001, max_range=32.0))         # (ceil(32000.0000...) cells: just inside)
    for fields in config_refusals():
        with pytest.raises(B.LfxError) as e:
            occupancy_tables(dict(GOOD, **fields))
        assert e.value.code == B.ERR_INVALID_ARGUMENT, fields


DRIVER = r"""
#include "lfx.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
static int same(const std::string & path, const std::vector<unsigned char> & want)
{
  std::FILE * f = std::fopen(path.c_str(), "rb");
  if (!f) {return 0;}
  std::vector<unsigned char> got(want.size() + 16);
  const size_t n = std::fread(got.data(), 1, got.size(), f);
  std::fclose(f);
  return n == want.size() && std::memcmp(got.data(), want.data(), n) == 0;
}
int main(int argc, char ** argv)
{
  if (argc != 2) {return 2;}
  const std::string dir(argv[1]);
  int bad = 0;
  // the smallest and a wide grid, every int8 value, thresholds at their ends
  for (uint32_t w : {1u, 3u, 257u}) {
    for (uint32_t h : {1u, 2u, 129u}) {
      std::vector<int8_t> grid((size_t)w * h);
      for (size_t i = 0; i < grid.size(); i++) {grid[i] = (int8_t)(unsigned char)(i * 7u + w);}
      for (int occ : {1, 65, 100}) {
        const int rc = lfx_occupancy_write_map(dir.c_str(), grid.data(), w, h, 0.05f, -1.5, 2.5, occ, occ - 1);
        std::vector<unsigned char> want;
        char head[64];
        const int hn = std::snprintf(head, sizeof(head), "P5\n%u %u\n255\n", w, h);
        want.assign(head, head + hn);
        for (uint32_t y = h; y-- > 0u; ) {
          for (uint32_t x = 0; x < w; x++) {
            const int v = grid[(size_t)y * w + x];
            want.push_back(v == -1 ? 205 : (v >= occ ? 0 : (v <= occ - 1 ? 254 : 205)));
          }
        }
        const int ok = rc == 0 && same(dir + "/map.pgm", want);
        std::printf("case %u x %u occ %d: %d %d\n", w, h, occ, rc, ok);
        bad += ok ? 0 : 1;
      }
    }
  }
  const int8_t one = 0;
  const double nan = std::nan("");
  bad += lfx_occupancy_write_map(nullptr, &one, 1, 1, 1.0f, 0, 0, 65, 25) == -1 ? 0 : 1;
  bad += lfx_occupancy_write_map(dir.c_str(), nullptr, 1, 1, 1.0f, 0, 0, 65, 25) == -1 ? 0 : 1;
  bad += lfx_occupancy_write_map(dir.c_str(), &one, 0, 1, 1.0f, 0, 0, 65, 25) == -1 ? 0 : 1;
  bad += lfx_occupancy_write_map(dir.c_str(), &one, 1, 16385, 1.0f, 0, 0, 65, 25) == -1 ? 0 : 1;
  bad += lfx_occupancy_write_map(dir.c_str(), &one, 1, 1, 0.0f, 0, 0, 65, 25) == -1 ? 0 : 1;
  bad += lfx_occupancy_write_map(dir.c_str(), &one, 1, 1, 1.0f, nan, 0, 65, 25) == -1 ? 0 : 1;
  bad += lfx_occupancy_write_map(dir.c_str(), &one, 1, 1, 1.0f, 0, 0, 25, 25) == -1 ? 0 : 1;
  bad += lfx_occupancy_write_map((dir + "/no/such/dir").c_str(), &one, 1, 1, 1.0f, 0, 0, 65, 25) == -9 ? 0 : 1;
  bad += lfx_occupancy_write_map((dir + "/").c_str(), &one, 1, 1, 1.0f, 0, 0, 65, 25) == 0 ? 0 : 1;
  std::printf("bad %d\n", bad);
  return bad ? 3 : 0;
}
"""


def test_writer_under_sanitizers(tmp_path):
    """lfx_occmap.cpp built alone with a small driver under -fsanitize=address,undefined: grids of several shapes with every
    int8 value, the refusals and an unwritable directory -- the files are what the driver expects and no sanitizer reports.
    The sanitizer runtimes are linked into the executable, so the driver runs in the environment as it is."""
    drv = tmp_path / "driver.cpp"
    drv.write_text(DRIVER)
    exe = tmp_path / "occmap_asan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), os.path.join(CSRC, "lfx_occmap.cpp"), str(drv), "-o", str(exe)])
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(exe), str(out_dir)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=300)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "runtime error" not in out and "Sanitizer" not in out, out[-4000:]
    assert out.count("case ") == 27 and "bad 0" in out
