"""The grid-match section without a device: the restatement (tests/grid_match_restatement.py) held to a triple-loop brute
force and to values written out by hand on a 5 x 4 field, and the library's host side held to it -- lfx_grid_match_table byte
for byte, the rotations against math.cos / math.sin, candidate and pose3, what the host calls refuse -- the conditions the GPU
cases rely on, checked on the restatement, and lfx_gridmatchmap.cpp built alone with a small main of its own under
-fsanitize=address,undefined and run as a program (nothing is loaded into Python under a sanitizer), the way
tests/test_distance_expect.py treats lfx_distmap.cpp."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from lidar_feature_extraction_amd import binding as B
from lidar_feature_extraction_amd import (grid_match_candidate, grid_match_pose3, grid_match_rotations, grid_match_search_config, grid_match_search_size,
                                          grid_match_table, grid_match_table_config)
from tests import distance_restatement as D
from tests import grid_match_cases as GC
from tests import grid_match_restatement as G
from tests import occupancy_cases as OC
from tests import occupancy_restatement as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_feature_extraction_amd", "csrc")


# --- the restatement against itself ------------------------------------------------------------------------------------------------
def test_hand_values():
    S, geom, pts = GC.HAND_S, GC.HAND_GEOM, GC.HAND_POINTS
    # the points' cells at the origin are (0, 0), (1, 0), (0, 2)
    sc, ins = G.score(S, pts, [[0, 0, 1, 0], [1, 1, 1, 0], [-1, -1, 1, 0], [0, 0, 0, 1], [3, 0, 0, 1], [3.5, 0, 1, 0], [float("nan"), 0, 1, 0],
                               [float("inf"), 0, 1, 0], [2.0 ** 30, 0, 1, 0]], geom)
    assert sc.tolist() == [0 + 1 + 20, 11 + 12 + 31, 0, 0, 2 + 12 + 0, 4 + 24, 0, 0, 0]
    assert ins.tolist() == [3, 3, 0, 0, 3, 2, 0, 0, 0]
    cfg = G.search_config(half_x=1, half_y=1)
    best, sl, vol = G.search(S, [pts], [[0.0, 0.0, 0.0]], cfg, geom)
    assert vol[0, 0].tolist() == [[0, 10, 11], [0, 0 + 1 + 20, 1 + 2 + 21], [10, 10 + 11 + 30, 11 + 12 + 31]]
    assert best[0].tolist() == [54, 8, 3, 3] and sl[0].tolist() == [[54, 8]]
    # three headings a quarter turn apart around -pi/2: the last one is exactly 0, the middle one turns every point to a negative y
    cfg = G.search_config(half_x=3, half_y=0, half_theta=1, theta_step=math.pi / 2, step_cells=1)
    best, sl, vol = G.search(S, [pts], [[0.0, 0.0, -math.pi / 2]], cfg, geom)
    assert G.angle(-math.pi / 2, 1, math.pi / 2, 2) == 0.0
    assert vol[0, 2, 0].tolist() == [0, 0, 0, 21, 1 + 2 + 21, 2 + 3 + 22, 3 + 4 + 23] and not vol[0, 1].any()
    assert best[0].tolist() == [30, 2 * 7 + 6, 3, 3] and sl[0, 1].tolist() == [0, 7]


def test_the_restatement_is_the_brute_force():
    rng = np.random.default_rng(7)
    for k, (w, h, hx, hy, ht, step) in enumerate([(5, 4, 1, 1, 0, 1), (17, 9, 3, 2, 1, 1), (9, 17, 2, 3, 1, 3), (12, 12, 6, 6, 0, 2), (6, 6, 0, 0, 2, 1)]):
        S = GC.random_field(h, w, seed=k)
        geom = G.geometry(w, h, 0.5, -1.25, 0.75)
        pts = np.stack([rng.uniform(-3, 6, 23), rng.uniform(-3, 6, 23)], axis=1)
        pts[3] = (float("inf"), 1.0)
        pts[4] = (1.0e12, 0.0)                                 # (beyond 2^30 cells: outside by the size rule, for every shift)
        cfg = GC.window(hx, hy, ht, step, theta_step=0.21)
        centre = [w * 0.25 - 1.25, h * 0.25 + 0.75, 0.4]
        best, sl, vol = G.search(S, [pts], [centre], cfg, geom)
        bvol, bbest = G.brute_search(S, pts, centre, cfg, geom)
        assert vol[0].tolist() == bvol, k
        assert (int(best[0, 0]), int(best[0, 1])) == bbest, k
        Nx, Ny, T = G.search_size(cfg)
        for j in range(T):
            flat = vol[0, j].reshape(-1)
            assert sl[0, j].tolist() == [flat.max(), j * Ny * Nx + int(np.flatnonzero(flat == flat.max())[0])]
        # the centre candidate of every heading is `score` at the centre under that heading
        cs = G.rotations(centre[2], cfg["half_theta"], cfg["theta_step"])
        sc, _ = G.score(S, pts, [[centre[0], centre[1], c, s] for c, s in cs], geom)
        assert sc.tolist() == vol[0, :, cfg["half_y"], cfg["half_x"]].tolist()
        # ... and the best's `inside` is `score`'s at a step of 1 cell only up to rounding: counted here from the base cells
        assert best[0, 3] == len(pts) and best[0, 2] <= len(pts) - 2


def test_equal_maxima_go_to_the_lowest_index():
    S = np.zeros((9, 9), np.uint16)
    S[2, 2] = S[2, 6] = S[6, 2] = S[6, 6] = 7
    geom = G.geometry(9, 9, 1.0)
    best, sl, vol = G.search(S, [np.array([[4.5, 4.5]])], [[0.0, 0.0, 0.0]], G.search_config(half_x=3, half_y=3), geom)
    assert (vol[0, 0] == 7).sum() == 4 and best[0].tolist() == [7, (1 * 7) + 1, 1, 1]
    empty = G.search(S, [np.zeros((0, 2))], [[0.0, 0.0, 0.0]], G.search_config(half_x=3, half_y=3), geom)[0]
    assert empty[0].tolist() == [0, 0, 0, 0]


def test_field_and_points():
    lut = np.array([9, 8, 7, 6, 5], np.uint16)                # Rs = 2
    d2 = np.array([[0, 4, 5, G.FAR], [1, 2, 3, 4]], np.uint32)
    assert G.field(d2, lut).tolist() == [[9, 5, 0, 0], [8, 7, 6, 5]] and G.field(d2, lut).dtype == np.uint16
    assert G.field(d2, lut[:1]).tolist() == [[9, 0, 0, 0], [0, 0, 0, 0]]
    xyz = np.array([[[1, 2, 3], [4, 5, 6], [7, 8, 9], [np.inf, 0, 0]]], np.float32)
    kind = np.array([[GC.HIT, GC.CLEAR, GC.HIT, GC.HIT]], np.uint32)
    assert G.points(xyz, kind)[0].tolist() == [[1, 2], [7, 8]]                   # (inf * 0 is no number: left out)
    lv = np.array([[[0, -1, 0], [1, 0, 0.5], [0, 0, 1]]])
    assert G.points(xyz[:, :3], kind[:, :3], lv)[0].tolist() == [[-2, 1 + 1.5], [-8, 7 + 4.5]]


# --- the library's host side ---------------------------------------------------------------------------------------------------------
TABLES = [dict(), dict(sigma=0.05), dict(sigma=1.0, max_distance=3.0), dict(max_distance=0.0), dict(peak=1), dict(peak=65535),
          dict(sigma=0.5, max_distance=1.0, peak=65535), dict(sigma=0.013, max_distance=0.7, peak=40000)]


def test_table_byte_for_byte():
    for res in (0.05, 0.1, 0.25):
        for fields in TABLES + [dict(max_distance=64 * float(np.float32(res)))]:
            cfg = G.table_config(**fields)
            want = G.table(cfg, res)
            got = grid_match_table(fields, res)
            GC.same_bytes(got, want, (res, fields))
            rs = G.table_cells(cfg, res)
            assert len(got) == rs * rs + 1 and got[0] == cfg["peak"]
            if rs:
                assert (np.diff(got.astype(np.int64)) <= 0).all()
    assert len(grid_match_table(dict(max_distance=0.0), 0.1)) == 1                                   # Rs = 0
    assert len(grid_match_table(dict(max_distance=6.4), 0.1)) == 64 * 64 + 1                         # Rs = 64
    assert grid_match_table(dict(peak=65535), 0.1)[0] == 65535 and grid_match_table(dict(peak=1), 0.1).max() == 1
    # numpy and libm agree on these configs: the restatement's exponentials through numpy give the same bytes
    for res in (0.05, 0.1, 0.25):
        for fields in TABLES:
            cfg = G.table_config(**fields)
            k = np.arange(G.table_cells(cfg, res) ** 2 + 1, dtype=np.float64)
            d = np.sqrt(k) * float(np.float32(res))
            v = np.rint(float(cfg["peak"]) * np.exp(-(d * d) / ((2.0 * cfg["sigma"]) * cfg["sigma"])))
            GC.same_bytes(np.where(d > cfg["max_distance"], 0, v).astype(np.uint16), G.table(cfg, res), ("numpy", res, fields))


def test_rotations_candidate_and_pose3():
    for yaw0, half, step in ((0.0, 0, 0.0), (0.0, 3, 0.01), (1.3, 30, 0.00872), (-2.9, 180, 0.0174), (0.4, 0, float("nan"))):
        got = grid_match_rotations(yaw0, half, step)
        want = G.rotations(yaw0, half, step)
        GC.same_bytes(got, want, (yaw0, half, step))
        assert got.shape == (2 * half + 1, 2)
    assert grid_match_rotations(0.0, 5, 0.02)[5].tolist() == [1.0, 0.0]
    rng = np.random.default_rng(3)
    for hx, hy, ht, step in GC.WINDOWS:
        cfg = GC.window(hx, hy, ht, step)
        Nx, Ny, T = G.search_size(cfg)
        assert grid_match_search_size(cfg) == (Nx, Ny, T)
        centre = rng.uniform(-50, 50, 3)
        for index in {0, Nx * Ny * T - 1, int(rng.integers(0, Nx * Ny * T))}:
            for res in (0.05, 0.1, 0.25):
                GC.same_bytes(grid_match_candidate(cfg, res, centre, index), G.candidate(cfg, res, centre, index), (cfg, index, res))
        with pytest.raises(B.LfxError):
            grid_match_candidate(cfg, 0.1, centre, Nx * Ny * T)
    for pose2 in ([0.0, 0.0, 0.0], [3.5, -2.25, 0.7], [1e3, 2e3, -3.1]):
        for level in (None, OC.tilted_poses(1, seed=8)[0][:, :3]):
            GC.same_bytes(grid_match_pose3(pose2, level, 0.37), G.pose3(pose2, level, 0.37), (pose2, level is None))
    assert grid_match_pose3([1.0, 2.0, 0.0]).tolist() == [[1, 0, 0, 1], [0, 1, 0, 2], [0, 0, 1, 0]]


def test_what_the_host_calls_refuse():
    L = B.load()
    n, lut = C.c_uint32(7), (C.c_uint16 * 4200)()
    ok = grid_match_table_config()
    assert L.lfx_grid_match_table_size(C.byref(ok), 0.1, C.byref(n)) == 0 and n.value == 401
    for fields in (dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(max_distance=-0.1),
                   dict(max_distance=float("nan")), dict(max_distance=6.5), dict(max_distance=3.0e38), dict(peak=0), dict(peak=65536), dict(reserved=1)):
        bad = grid_match_table_config(fields)
        assert L.lfx_grid_match_table_size(C.byref(bad), 0.1, C.byref(n)) == -1, fields
        assert L.lfx_grid_match_table(C.byref(bad), 0.1, lut, 401) == -1, fields
    for res in (0.0, -0.1, float("nan"), float("inf")):
        assert L.lfx_grid_match_table_size(C.byref(ok), res, C.byref(n)) == -1
    assert L.lfx_grid_match_table_size(None, 0.1, C.byref(n)) == -1 and L.lfx_grid_match_table_size(C.byref(ok), 0.1, None) == -1
    assert L.lfx_grid_match_table(C.byref(ok), 0.1, None, 401) == -1 and L.lfx_grid_match_table(C.byref(ok), 0.1, lut, 400) == -1
    assert n.value == 401
    dims = (C.c_uint32 * 3)()
    for fields in (dict(half_x=257), dict(half_y=257), dict(step_cells=0), dict(step_cells=17), dict(half_theta=181), dict(half_theta=1, theta_step=0.0),
                   dict(half_theta=1, theta_step=-0.1), dict(half_theta=1, theta_step=float("nan")), dict(half_theta=1, theta_step=float("inf"))):
        bad = grid_match_search_config(fields)
        assert L.lfx_grid_match_search_size(C.byref(bad), dims) == -1, fields
    good = grid_match_search_config(half_x=256, half_y=256, half_theta=180, step_cells=16, theta_step=0.01)
    assert L.lfx_grid_match_search_size(C.byref(good), dims) == 0 and list(dims) == [513, 513, 361]
    assert L.lfx_grid_match_search_size(None, dims) == -1 and L.lfx_grid_match_search_size(C.byref(good), None) == -1
    cs = np.zeros((361, 2))
    p = C.c_void_p(cs.ctypes.data)
    assert L.lfx_grid_match_rotations(0.0, 181, 0.01, p) == -1 and L.lfx_grid_match_rotations(float("nan"), 1, 0.01, p) == -1
    assert L.lfx_grid_match_rotations(0.0, 1, 0.0, p) == -1 and L.lfx_grid_match_rotations(0.0, 1, 0.01, None) == -1
    assert not cs.any()
    c3, out = np.zeros(3), np.zeros(3)
    pc, po = C.c_void_p(c3.ctypes.data), C.c_void_p(out.ctypes.data)
    assert L.lfx_grid_match_candidate(C.byref(good), 0.1, pc, 0, po) == 0
    assert L.lfx_grid_match_candidate(C.byref(good), 0.1, None, 0, po) == -1 and L.lfx_grid_match_candidate(C.byref(good), 0.1, pc, 0, None) == -1
    assert L.lfx_grid_match_candidate(None, 0.1, pc, 0, po) == -1 and L.lfx_grid_match_candidate(C.byref(good), float("nan"), pc, 0, po) == -1
    assert L.lfx_grid_match_candidate(C.byref(good), 0.1, pc, 513 * 513 * 361, po) == -1
    c3[1] = float("inf")
    assert L.lfx_grid_match_candidate(C.byref(good), 0.1, pc, 0, po) == -1
    p12 = np.zeros(12)
    assert L.lfx_grid_match_pose3(None, None, 0.0, C.c_void_p(p12.ctypes.data)) == -1 and L.lfx_grid_match_pose3(po, None, 0.0, None) == -1


# --- what the GPU cases rely on ------------------------------------------------------------------------------------------------------
def e2e_on_the_restatement():
    """(S, the scans' points, the poses, the table) of the end-to-end scene, all from the restatements"""
    cfg = GC.e2e_config()
    clouds, poses = GC.e2e_scans()
    ref = O.Grid(cfg)
    ref.add_scans(clouds, poses)
    ref.render()
    grid = ref.emit()
    d2 = D.d2_separable(grid, D.config())
    lut = G.table(G.table_config(), cfg.resolution)
    xyz, kind = ref.beams()
    return G.field(d2, lut), G.points(xyz, kind, poses[:, :, :3]), poses, lut, (xyz, kind)


def test_the_conditions_of_the_gpu_cases():
    cfg = GC.e2e_config()
    geom = G.geometry(cfg.width, cfg.height, cfg.resolution, cfg.origin_x, cfg.origin_y)
    S, pts, poses, lut, _ = e2e_on_the_restatement()
    assert [len(p) for p in pts] == [GC.E2E_BEAMS] * len(pts) and lut[0] == 1000
    # a scan scored at its own stored pose: every point on an obstacle cell
    for k, p in enumerate(pts):
        sc, ins = G.score(S, p, [[poses[k][0, 3], poses[k][1, 3], 1.0, 0.0]], geom)
        assert sc[0] == len(p) * int(lut[0]) and ins[0] == len(p), k
    # the search from the wrong centre
    window = G.search_config(**GC.E2E_WINDOW)
    centre = GC.e2e_centre(poses)
    best, sl, vol = G.search(S, [pts[GC.E2E_QUERY]], [centre], window, geom)
    true = GC.e2e_true_index()
    n = len(pts[GC.E2E_QUERY])
    assert vol[0].reshape(-1)[true] == n * int(lut[0])
    assert best[0, 0] == n * int(lut[0]) == vol[0].max() and best[0, 1] <= true and best[0, 2] == n
    assert (vol[0] < vol[0].max()).sum() > vol[0].size // 2
    found = G.candidate(window, cfg.resolution, centre, true)
    assert found.tolist() == [poses[GC.E2E_QUERY][0, 3], poses[GC.E2E_QUERY][1, 3], 0.0]


# --- lfx_gridmatchmap.cpp alone, under sanitizers ------------------------------------------------------------------------------------
DRIVER = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <memory>
#include <vector>
#include "lfx.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

int main()
{
  const float nan = std::numeric_limits<float>::quiet_NaN();
  lfx_grid_match_table_config k;
  lfx_grid_match_table_default_config(&k);
  lfx_grid_match_table_default_config(nullptr);
  lfx_grid_match_default_config(nullptr);
  lfx_grid_match_search_default_config(nullptr);
  EXPECT(k.sigma == 0.2f && k.max_distance == 2.0f && k.peak == 1000u && k.reserved == 0u);
  // tables of every size, each in a block of exactly its size: a write past the end is the sanitizer's
  const float resolutions[] = {0.05f, 0.1f, 0.25f, 1.0f};
  for (float res : resolutions) {
    for (int cells = 0; cells <= 64; cells++) {
      lfx_grid_match_table_config c = k;
      c.max_distance = (float)cells * res;
      std::uint32_t n = 0;
      if (lfx_grid_match_table_size(&c, res, &n) != LFX_OK) {continue;}      // (a product that rounds above 64 cells)
      std::unique_ptr<std::uint16_t[]> lut(new std::uint16_t[n]);
      EXPECT(lfx_grid_match_table(&c, res, lut.get(), n) == LFX_OK);
      EXPECT(lut[0] == 1000);
      EXPECT(lfx_grid_match_table(&c, res, lut.get(), n + 1u) == LFX_ERR_INVALID_ARGUMENT);
    }
  }
  std::uint32_t n = 0;
  std::uint16_t one = 0;
  lfx_grid_match_table_config c = k;
  c.max_distance = 0.0f;
  EXPECT(lfx_grid_match_table_size(&c, 0.1f, &n) == LFX_OK && n == 1u && lfx_grid_match_table(&c, 0.1f, &one, 1u) == LFX_OK && one == 1000);
  c.max_distance = 3.0e38f;                     // (a quotient far beyond uint32: refused, not converted)
  EXPECT(lfx_grid_match_table_size(&c, 1.0e-38f, &n) == LFX_ERR_INVALID_ARGUMENT);
  EXPECT(lfx_grid_match_table(&c, 1.0e-38f, &one, 1u) == LFX_ERR_INVALID_ARGUMENT);
  c = k; c.sigma = nan;
  EXPECT(lfx_grid_match_table_size(&c, 0.1f, &n) == LFX_ERR_INVALID_ARGUMENT);
  c = k; c.sigma = 1.0e-30f; c.peak = 65535u;   // (the exponent overflows to -inf: the table is the peak, then zeros)
  EXPECT(lfx_grid_match_table_size(&c, 0.1f, &n) == LFX_OK && n == 401u);
  std::vector<std::uint16_t> lut(n);
  EXPECT(lfx_grid_match_table(&c, 0.1f, lut.data(), n) == LFX_OK && lut[0] == 65535 && lut[1] == 0 && lut[400] == 0);
  EXPECT(lfx_grid_match_table_size(&k, nan, &n) == LFX_ERR_INVALID_ARGUMENT && lfx_grid_match_table_size(nullptr, 0.1f, &n) == LFX_ERR_INVALID_ARGUMENT);
  // the rotations, in a block of exactly their size
  for (std::uint32_t half : {0u, 1u, 30u, 180u}) {
    std::unique_ptr<double[]> cs(new double[2u * (2u * half + 1u)]);
    EXPECT(lfx_grid_match_rotations(0.0, half, 0.01, cs.get()) == LFX_OK);
    EXPECT(cs[2u * half] == 1.0 && cs[2u * half + 1u] == 0.0);
  }
  double two[2];
  EXPECT(lfx_grid_match_rotations(0.0, 181u, 0.01, two) == LFX_ERR_INVALID_ARGUMENT);
  EXPECT(lfx_grid_match_rotations(0.0, 0u, std::numeric_limits<double>::quiet_NaN(), two) == LFX_OK && two[0] == 1.0);
  // candidates at the window's corners, and the conversions at their edges
  lfx_grid_match_search_config s;
  lfx_grid_match_search_default_config(&s);
  s.half_x = 256; s.half_y = 256; s.half_theta = 180; s.step_cells = 16; s.theta_step = 0.01;
  std::uint32_t dims[3];
  EXPECT(lfx_grid_match_search_size(&s, dims) == LFX_OK && dims[0] == 513u && dims[1] == 513u && dims[2] == 361u);
  const double centre[3] = {1.0, 2.0, 0.5};
  double pose2[3];
  EXPECT(lfx_grid_match_candidate(&s, 0.5f, centre, 0u, pose2) == LFX_OK && pose2[0] == 1.0 - 2048.0 && pose2[1] == 2.0 - 2048.0);
  EXPECT(lfx_grid_match_candidate(&s, 0.5f, centre, 513u * 513u * 361u - 1u, pose2) == LFX_OK && pose2[0] == 1.0 + 2048.0);
  EXPECT(lfx_grid_match_candidate(&s, 0.5f, centre, 513u * 513u * 361u, pose2) == LFX_ERR_INVALID_ARGUMENT);
  EXPECT(lfx_grid_match_candidate(&s, 0.5f, centre, 0xFFFFFFFFu, pose2) == LFX_ERR_INVALID_ARGUMENT);
  s.step_cells = 17;
  EXPECT(lfx_grid_match_candidate(&s, 0.5f, centre, 0u, pose2) == LFX_ERR_INVALID_ARGUMENT);
  double pose[12];
  EXPECT(lfx_grid_match_pose3(centre, nullptr, 3.0, pose) == LFX_OK && pose[3] == 1.0 && pose[7] == 2.0 && pose[11] == 3.0 && pose[10] == 1.0);
  EXPECT(lfx_grid_match_pose3(nullptr, nullptr, 3.0, pose) == LFX_ERR_INVALID_ARGUMENT);
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
"""


def test_host_side_under_sanitizers(tmp_path):
    """lfx_gridmatchmap.cpp built alone with a small driver under -fsanitize=address,undefined: tables and rotations of every
    size in blocks of exactly their size, the refusals, the float-to-integer conversions at their edges -- no sanitizer
    reports.  The sanitizer runtimes are linked into the executable, so the driver runs in the environment as it is."""
    drv = tmp_path / "driver.cpp"
    drv.write_text(DRIVER)
    exe = tmp_path / "gridmatchmap_asan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), os.path.join(CSRC, "lfx_gridmatchmap.cpp"), str(drv), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=300)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "runtime error" not in out and "Sanitizer" not in out and "0 failures" in out, out[-4000:]
