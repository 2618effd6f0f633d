"""The distance section without a device: the restatement (tests/distance_restatement.py) held to itself -- its separable
form against its brute force on every case small enough, both against scipy's exact transform where scipy is there -- and
the library's host side held to it: lfx_distance_cost_table byte for byte, its anchors, what it refuses, and lfx_distmap.cpp
built alone with a small main of its own under -fsanitize=address,undefined and run as a program (nothing is loaded into
Python under a sanitizer), the way tests/test_occupancy_files.py treats lfx_occmap.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from lidar_feature_extraction_amd import binding as B
from lidar_feature_extraction_amd import distance_config, distance_cost_config, distance_cost_table
from tests import distance_cases as DC
from tests import distance_restatement as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_feature_extraction_amd", "csrc")


def _small_cases():
    cases = DC.smallest() + DC.capped() + DC.breakers()
    cases += [("shape_%dx%d" % (w, h), DC.shape_grid(w, h), {}) for w, h in ((63, 2), (65, 67), (257, 2), (5, DC.SEG_ROWS + 1))]
    return cases


def test_the_separable_form_is_the_brute_force():
    for name, G, fields in _small_cases():
        for inside in (False, True):
            cfg = D.config(**dict(fields, inside=int(inside)))
            DC.same_bytes(D.d2_separable(G, cfg, inside), D.d2_brute(G, cfg, inside), (name, inside))


def test_hand_values():
    """the cap's three cells of the issue, and what the smallest grids hold"""
    g = DC.with_obstacles(9, 9, [(0, 0)])
    d2 = D.d2_brute(g, D.config(max_cells=5))
    assert d2[4, 3] == 25 and d2[0, 5] == 25 and d2[1, 5] == D.FAR and d2[0, 0] == 0
    assert (D.d2_brute(g, D.config(max_cells=1)) != D.FAR).sum() == 3
    assert D.d2_brute(g, D.config())[8, 8] == 128 and D.d2_brute(g, D.config(max_cells=32767))[8, 8] == 128
    free = DC.grid(3, 4)
    assert (D.d2_brute(free, D.config()) == D.FAR).all() and D.stats(free, D.config(), D.d2_brute(free, D.config()))["max_d2"] == 0
    full = DC.grid(3, 4, DC.OCC_V)
    assert (D.d2_brute(full, D.config()) == 0).all() and (D.d2_brute(full, D.config(), inside=True) == D.FAR).all()
    unk = DC.grid(2, 2, DC.UNK_V)
    assert (D.classes(unk, D.config()) == D.UNKNOWN).all() and (D.classes(unk, D.config(unknown_is_obstacle=1)) == D.OBSTACLE).all()
    v = np.array([[40, 41, 39, -1]], np.int8)
    assert D.classes(v, D.config(occupied_percent=40)).tolist() == [[D.OBSTACLE, D.OBSTACLE, D.FREE, D.UNKNOWN]]
    assert D.classes(v, D.config(occupied_percent=41)).tolist() == [[D.FREE, D.OBSTACLE, D.FREE, D.UNKNOWN]]
    m = D.metres(D.classes(g, D.config()), D.d2_brute(g, D.config(max_cells=5)), None, 0.5)
    assert m[0, 0] == 0.0 and m[4, 3] == np.float32(2.5) and m[1, 5] == np.inf and m.dtype == np.float32
    both = D.metres(D.classes(g, D.config()), D.d2_brute(g, D.config()), D.d2_brute(g, D.config(), inside=True), 0.5)
    assert both[0, 0] == np.float32(-0.5) and both[0, 1] == np.float32(0.5)


def test_both_are_scipys_exact_transform():
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, G, fields in _small_cases():
        cfg = D.config(**dict(fields, max_cells=0))
        for inside in (False, True):
            sites = (D.classes(G, cfg) == D.OBSTACLE) != inside
            if not sites.any():
                continue
            want = np.rint(ndimage.distance_transform_edt(~sites) ** 2).astype(np.uint32)
            DC.same_bytes(D.d2_brute(G, cfg, inside), want, (name, inside, "brute"))
            DC.same_bytes(D.d2_separable(G, cfg, inside), want, (name, inside, "separable"))


# --- the cost table --------------------------------------------------------------------------------------------------------------
COST_CASES = [({}, 0.05), ({}, 0.1), (dict(inscribed_radius=0.75, inflation_radius=1.25), 0.25), (dict(inscribed_radius=0.0, inflation_radius=0.0), 0.05),
              (dict(cost_scaling_factor=0.0), 0.05), (dict(inscribed_radius=0.3, inflation_radius=3.0, cost_scaling_factor=2.5), 0.02),
              (dict(inflation_radius=64.0), 0.0625), (dict(inscribed_radius=0.5, inflation_radius=0.5, cost_scaling_factor=100.0), 0.01)]


@pytest.mark.parametrize("fields,res", COST_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_cost_table_is_the_restatements(fields, res):
    """Equal everywhere, except where 252 exp(...) lies within 1e-9 of an integer: there libm and numpy may round exp to
    either side, a difference of 1 is allowed, and the library's bytes are what the device gets."""
    cfg = D.cost_config(**fields)
    want, exact = D.cost_table(cfg, res, with_exact=True)
    got = distance_cost_table(cfg, res)
    assert got.dtype == np.uint8 and got.shape == want.shape and len(got) == D.cost_cells(cfg, res) ** 2 + 1
    loose = np.abs(exact - np.rint(exact)) < 1e-9                         # (nan where no exp is taken: False)
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    assert (diff[~loose] == 0).all() and (diff[loose] <= 1).all(), (np.nonzero(diff)[0][:5], loose.sum())
    # the anchors
    assert got[0] == 254
    d = np.sqrt(np.arange(len(got), dtype=np.float64)) * np.float64(np.float32(res))
    inscribed, inflation = np.float64(np.float32(cfg["inscribed_radius"])), np.float64(np.float32(cfg["inflation_radius"]))
    assert (got[1:][d[1:] <= inscribed] == 253).all() and (got[1:][d[1:] > inflation] == 0).all()
    assert (np.diff(got.astype(np.int64)) <= 0).all()
    assert (got[1:][(d[1:] > inscribed) & (d[1:] <= inflation)] <= 252).all()


def test_cost_table_on_the_radii():
    """resolution 0.25, radii 0.75 and 1.25: sqrt(9) * 0.25 and sqrt(25) * 0.25 land exactly on them"""
    lut = distance_cost_table(dict(inscribed_radius=0.75, inflation_radius=1.25, cost_scaling_factor=10.0), 0.25)
    assert len(lut) == 26
    assert lut[9] == 253 and lut[8] == 253 and lut[10] == int(252.0 * np.exp(-10.0 * (np.sqrt(10.0) * 0.25 - 0.75))) < 252
    assert lut[25] == int(252.0 * np.exp(-10.0 * 0.5)) == 1 and lut[24] >= lut[25]
    # one cell more of inflation: 26 .. 36 exist and lie beyond the radius
    wider = distance_cost_table(dict(inscribed_radius=0.75, inflation_radius=1.26, cost_scaling_factor=10.0), 0.25)
    assert len(wider) == 37 and wider[25] == 1 and (wider[27:] == 0).all()


def test_cost_table_refuses():
    L = B.load()
    n = C.c_uint32(7)
    lut = np.zeros(1 << 21, np.uint8)
    p = C.c_void_p(lut.ctypes.data)

    def size(res=0.05, **fields):
        cfg = distance_cost_config(**fields)
        return L.lfx_distance_cost_table_size(C.byref(cfg), C.c_float(res), C.byref(n))

    # (0.55f / 0.05f is a little above 11 in double: Rc = 12, as the header's expression says)
    assert size() == 0 and n.value == 12 * 12 + 1 == D.cost_cells(D.cost_config(), 0.05) ** 2 + 1
    assert size(res=0.0625, inflation_radius=64.0) == 0 and n.value == 1024 * 1024 + 1    # Rc = 1024: the largest
    assert size(res=0.0625, inflation_radius=64.03) == -1                                 # Rc = 1025
    assert size(inflation_radius=0.1) == -1 and size(inscribed_radius=0.6) == -1      # radii out of order
    for bad in (float("nan"), float("inf"), -1.0):
        assert size(inscribed_radius=bad) == -1 and size(cost_scaling_factor=bad) == -1 and size(res=bad) == -1
    assert size(inflation_radius=float("nan")) == -1 and size(inflation_radius=float("inf")) == -1
    assert size(res=0.0) == -1 and size(track_unknown=2) == -1
    cfg = distance_cost_config()
    assert L.lfx_distance_cost_table_size(None, C.c_float(0.05), C.byref(n)) == -1 and L.lfx_distance_cost_table_size(C.byref(cfg), C.c_float(0.05), None) == -1
    assert L.lfx_distance_cost_table(C.byref(cfg), C.c_float(0.05), p, 145) == 0 and lut[0] == 254 and lut[145] == 0
    for wrong in (0, 144, 146):
        assert L.lfx_distance_cost_table(C.byref(cfg), C.c_float(0.05), p, wrong) == -1
    assert L.lfx_distance_cost_table(C.byref(cfg), C.c_float(0.05), None, 145) == -1 and L.lfx_distance_cost_table(None, C.c_float(0.05), p, 145) == -1
    bad = distance_cost_config(inflation_radius=float("nan"))
    assert L.lfx_distance_cost_table(C.byref(bad), C.c_float(0.05), p, 145) == -1
    with pytest.raises(B.LfxError):
        distance_cost_table(dict(inflation_radius=100.0), 0.05)


def test_default_configs():
    c, k = distance_config(), distance_cost_config()
    assert (c.occupied_percent, c.unknown_is_obstacle, c.max_cells, c.inside, c.reserved) == (65, 0, 0, 0, 0)
    assert (k.inscribed_radius, k.inflation_radius, k.cost_scaling_factor, k.track_unknown) == (np.float32(0.22), np.float32(0.55), 10.0, 1)
    assert D.config() == {n: getattr(c, n) for n, _ in B.DistanceConfig._fields_}
    with pytest.raises(TypeError):
        distance_config(radius=3)


DRIVER = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>
#include "lfx.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); fails++; } } while (0)

int main()
{
  lfx_distance_config d;
  lfx_distance_default_config(&d);
  lfx_distance_default_config(nullptr);
  EXPECT(d.occupied_percent == 65 && d.max_cells == 0u && d.inside == 0u && d.unknown_is_obstacle == 0u && d.reserved == 0u);
  lfx_distance_cost_config k;
  lfx_distance_cost_default_config(&k);
  lfx_distance_cost_default_config(nullptr);
  const float nan = std::numeric_limits<float>::quiet_NaN();
  // tables of every size up to the largest, each in a block of exactly its size: a byte too far is a report
  const float radii[] = {0.0f, 0.06f, 0.0625f, 0.55f, 1.0f, 7.77f, 64.0f};
  const float res = 0.0625f;
  for (float r : radii) {
    lfx_distance_cost_config c = k;
    c.inflation_radius = r < c.inscribed_radius ? c.inscribed_radius : r;
    std::uint32_t n = 0;
    EXPECT(lfx_distance_cost_table_size(&c, res, &n) == LFX_OK);
    const std::uint32_t rc = (std::uint32_t)std::ceil((double)c.inflation_radius / (double)res);
    EXPECT(n == rc * rc + 1u);
    std::vector<std::uint8_t> lut(n, 7);
    EXPECT(lfx_distance_cost_table(&c, res, lut.data(), n) == LFX_OK);
    EXPECT(lut[0] == 254);
    for (std::uint32_t i = 1; i < n; i++) {EXPECT(lut[i] <= lut[i - 1] && lut[i] <= 253);}
    EXPECT(lfx_distance_cost_table(&c, res, lut.data(), n + 1u) == LFX_ERR_INVALID_ARGUMENT);
    EXPECT(lfx_distance_cost_table(&c, res, lut.data(), n - 1u) == LFX_ERR_INVALID_ARGUMENT);
  }
  std::uint32_t n = 0;
  std::uint8_t one = 0;
  lfx_distance_cost_config c = k;
  c.inflation_radius = 64.03f;
  EXPECT(lfx_distance_cost_table_size(&c, 0.0625f, &n) == LFX_ERR_INVALID_ARGUMENT);
  c.inflation_radius = 3.0e38f;                 // (a quotient far beyond uint32: refused, not converted)
  EXPECT(lfx_distance_cost_table_size(&c, 1.0e-38f, &n) == LFX_ERR_INVALID_ARGUMENT);
  EXPECT(lfx_distance_cost_table(&c, 1.0e-38f, &one, 1u) == LFX_ERR_INVALID_ARGUMENT);
  c = k; c.inflation_radius = nan;
  EXPECT(lfx_distance_cost_table_size(&c, 0.05f, &n) == LFX_ERR_INVALID_ARGUMENT);
  c = k; c.inscribed_radius = 0.6f;
  EXPECT(lfx_distance_cost_table_size(&c, 0.05f, &n) == LFX_ERR_INVALID_ARGUMENT);
  c = k; c.cost_scaling_factor = -1.0f;
  EXPECT(lfx_distance_cost_table_size(&c, 0.05f, &n) == LFX_ERR_INVALID_ARGUMENT);
  EXPECT(lfx_distance_cost_table_size(&k, nan, &n) == LFX_ERR_INVALID_ARGUMENT);
  EXPECT(lfx_distance_cost_table_size(&k, 0.0f, &n) == LFX_ERR_INVALID_ARGUMENT);
  EXPECT(lfx_distance_cost_table_size(nullptr, 0.05f, &n) == LFX_ERR_INVALID_ARGUMENT);
  EXPECT(lfx_distance_cost_table_size(&k, 0.05f, nullptr) == LFX_ERR_INVALID_ARGUMENT);
  EXPECT(lfx_distance_cost_table(&k, 0.05f, nullptr, 145u) == LFX_ERR_INVALID_ARGUMENT);
  // a scaling that makes exp underflow, and none at all
  c = k; c.cost_scaling_factor = 3.0e38f; c.inflation_radius = 2.0f;
  EXPECT(lfx_distance_cost_table_size(&c, 0.05f, &n) == LFX_OK);
  std::vector<std::uint8_t> lut(n);
  EXPECT(lfx_distance_cost_table(&c, 0.05f, lut.data(), n) == LFX_OK && n > 1000u && lut[1000] == 0 && lut[10] == 253);
  c.cost_scaling_factor = 0.0f;
  EXPECT(lfx_distance_cost_table(&c, 0.05f, lut.data(), n) == LFX_OK && lut[1000] == 252 && lut[10] == 253);
  std::printf("%d failures\n", fails);
  return fails ? 1 : 0;
}
"""


def test_cost_table_under_sanitizers(tmp_path):
    """lfx_distmap.cpp built alone with a small driver under -fsanitize=address,undefined: tables of every size in blocks of
    exactly their size, the refusals, the float-to-integer conversions at their edges -- no sanitizer reports.  The
    sanitizer runtimes are linked into the executable, so the driver runs in the environment as it is."""
    drv = tmp_path / "driver.cpp"
    drv.write_text(DRIVER)
    exe = tmp_path / "distmap_asan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), os.path.join(CSRC, "lfx_distmap.cpp"), str(drv), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=300)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "runtime error" not in out and "Sanitizer" not in out and "0 failures" in out, out[-4000:]
