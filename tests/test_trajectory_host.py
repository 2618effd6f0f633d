"""The host side of the trajectory de-skew (include/lfx.h, the de-skew section): the segment table and the gyro integration
against the numpy restatement (tests/trajectory_restatement.py), the model itself against rays cast from a sensor entering
a turn, the two-knot case against the constant-motion restatement, and the two helpers under sanitizers.  No device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from lidar_feature_extraction_amd import binding as B
from tests import deskew_restatement as R
from tests import trajectory_cases as TC
from tests import trajectory_restatement as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_feature_extraction_amd", "csrc")


@pytest.fixture(scope="module")
def lfx():
    if not os.path.exists(B.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    import lidar_feature_extraction_amd as pkg
    B.load()
    return pkg


def _t_ref(rng, times, i):
    """At a knot, between knots, outside, by turns; the first knot every sixth time."""
    kind = i % 6
    if kind == 0:
        return times[0]
    if kind in (1, 2):
        return times[rng.integers(0, len(times))]
    if kind in (3, 4):
        return rng.uniform(times[0], times[-1])
    return times[0] - 0.3 * (times[-1] - times[0]) if i % 12 == 5 else times[-1] + 0.3 * (times[-1] - times[0])


def test_segments_against_the_restatement(lfx):
    """1 000 seeded trajectories of 2 - 64 knots, up to 0.3 rad between knots (every tenth below 1e-8), positions up to 50 m,
    t_ref at a knot, between knots and outside: every entry within 1e-12, the bound of the motion helpers' test for the same
    depth of arithmetic.  With t_ref == times[0] segment 0's A and q are the identity and zero exactly."""
    rng = np.random.default_rng(20262)
    for i in range(1000):
        knots = (2, 3, 64)[i] if i < 3 else int(rng.integers(2, 65))
        times, poses = TC.seeded(rng, knots, small=i % 10 == 9, t0=(0.0, 1.7e9 + 0.25)[i % 2], span=(1.0, 0.1)[i % 2])
        t_ref = _t_ref(rng, times, i)
        got = lfx.trajectory_segments(times, poses, t_ref)
        want = T.segments(times, poses, t_ref)
        assert got.shape == (knots - 1, 24)
        assert np.abs(got - want).max() <= 1e-12, (i, knots, np.abs(got - want).max())
        assert np.array_equal(got[:, T.TIME], times[:-1]), i
        if t_ref == times[0]:
            assert got[0, T.A:T.A + 9].tobytes() == np.eye(3).tobytes() and got[0, T.Q:T.Q + 3].tobytes() == np.zeros(3).tobytes(), i
        small = got[:, T.THETA] < 1e-8
        assert not got[small, T.K:T.K + 3].any()


def test_segments_refusals(lfx):
    L = B.load()
    rng = np.random.default_rng(3)
    times, poses = TC.seeded(rng, 5)
    out = np.zeros((64, 24))

    def rc(t, p, t_ref, n=None):
        t, p = np.ascontiguousarray(t, np.float64), np.ascontiguousarray(p, np.float64)
        tr = B.Trajectory(len(t) if n is None else n, t.ctypes.data_as(C.POINTER(C.c_double)), p.ctypes.data_as(C.POINTER(C.c_double)), t_ref)
        return L.lfx_trajectory_segments(C.byref(tr), out.ctypes.data_as(C.POINTER(C.c_double)))

    assert rc(times, poses, 0.5) == 0
    assert L.lfx_trajectory_segments(None, out.ctypes.data_as(C.POINTER(C.c_double))) == B.ERR_INVALID_ARGUMENT
    tr = B.Trajectory(5, None, None, 0.0)
    assert L.lfx_trajectory_segments(C.byref(tr), out.ctypes.data_as(C.POINTER(C.c_double))) == B.ERR_INVALID_ARGUMENT
    for n in (0, 1, 65, 0xFFFFFFFF):
        assert rc(times, poses, 0.5, n) == B.ERR_INVALID_ARGUMENT
    for bad in (np.nan, np.inf, -np.inf):
        assert rc(times, poses, bad) == B.ERR_INVALID_ARGUMENT
        t2 = times.copy()
        t2[2] = bad
        assert rc(t2, poses, 0.5) == B.ERR_INVALID_ARGUMENT
        p2 = poses.copy()
        p2[3, 1, 2] = bad
        assert rc(times, p2, 0.5) == B.ERR_INVALID_ARGUMENT
    t2 = times.copy()
    t2[3] = t2[2]
    assert rc(t2, poses, 0.5) == B.ERR_INVALID_ARGUMENT            # not strictly ascending
    assert rc(times[::-1], poses, 0.5) == B.ERR_INVALID_ARGUMENT
    with pytest.raises(B.LfxError):
        lfx.trajectory_segments(np.arange(65.0), np.tile(R.IDENTITY, (65, 1, 1)), 0.0)


def test_from_gyro(lfx):
    """Against the restatement to 1e-12; a constant rate about a fixed axis over 64 samples gives Exp(rate (t_j - t_0)) within
    1e-12; a bias equal to the rate gives identities byte for byte; what is refused."""
    rng = np.random.default_rng(20263)
    for i in range(200):
        n = int(rng.integers(2, 65))
        times = 100.0 + np.cumsum(rng.uniform(0.001, 0.01, n))
        rates = rng.normal(0.0, 1.5, (n, 3)) if i % 10 else rng.normal(0.0, 1e-7, (n, 3))
        bias = None if i % 3 == 0 else rng.normal(0.0, 0.01, 3)
        velocity = None if i % 4 == 0 else rng.normal(0.0, 10.0, 3)
        got = lfx.trajectory_from_gyro(times, rates, bias, velocity)
        assert got.shape == (n, 3, 4) and got[0].tobytes() == R.IDENTITY.tobytes()
        assert np.abs(got - T.from_gyro(times, rates, bias, velocity)).max() <= 1e-12, i
    times = 5.0 + np.arange(64) * 0.0025
    rate = TC.unit(rng) * 2.0
    got = lfx.trajectory_from_gyro(times, np.tile(rate, (64, 1)), None, [3.0, -1.0, 0.5])
    for j in range(64):
        assert np.abs(got[j, :, :3] - R.exp_so3(rate * (times[j] - times[0]))).max() <= 1e-12, j
        assert np.abs(got[j, :, 3] - np.array([3.0, -1.0, 0.5]) * (times[j] - times[0])).max() <= 1e-12
    still = lfx.trajectory_from_gyro(times, np.tile(rate, (64, 1)), rate, None)
    assert still.tobytes() == np.tile(R.IDENTITY, (64, 1, 1)).tobytes()
    L = B.load()
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    rates, out = np.zeros((64, 3)), np.zeros((64, 12))
    assert L.lfx_trajectory_from_gyro(pd(times), pd(rates), 64, None, None, pd(out)) == 0
    assert L.lfx_trajectory_from_gyro(pd(times), pd(rates), 1, None, None, pd(out)) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_trajectory_from_gyro(pd(times), pd(rates), 0, None, None, pd(out)) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_trajectory_from_gyro(None, pd(rates), 64, None, None, pd(out)) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_trajectory_from_gyro(pd(times), None, 64, None, None, pd(out)) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_trajectory_from_gyro(pd(times), pd(rates), 64, None, None, None) == B.ERR_INVALID_ARGUMENT
    for bad in (np.nan, np.inf):
        t2 = times.copy()
        t2[7] = bad
        assert L.lfx_trajectory_from_gyro(pd(t2), pd(rates), 64, None, None, pd(out)) == B.ERR_INVALID_ARGUMENT
    t2 = times.copy()
    t2[8] = t2[7]
    assert L.lfx_trajectory_from_gyro(pd(t2), pd(rates), 64, None, None, pd(out)) == B.ERR_INVALID_ARGUMENT
    t2 = np.ascontiguousarray(times[::-1])
    assert L.lfx_trajectory_from_gyro(pd(t2), pd(rates), 64, None, None, pd(out)) == B.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("where", ["start", "end", "inside"])
def test_the_model_is_physically_right(lfx, where):
    """A 16 x 900 sweep of a sensor entering a turn (21 knots over 0.1 s at 15 m/s, a yaw rate of 35 deg/s (1 + 2 sin(2 pi t / T))
    with a little roll and pitch): the restatement's float32 output carried to the world by P(t_ref) is within
    4 * 2^-24 * max|coordinate| of the measured world points (tests/test_deskew_host.py derives the bound); the
    constant-motion restatement with the motion between the first and the last knot misses the same points by more than
    0.1 m on average."""
    from lidar_feature_extraction_amd.synth import trajectory_poses
    times, poses = TC.turning(R.pose([0.0, 0.0, 0.4], [-2.0, 1.0, 1.8]))
    rec, world, t = lfx.make_sweep_trajectory(16, 900, seed=77, times=times, poses=poses)
    n = len(rec)
    assert n == 16 * 900 and np.array_equal(t, np.arange(n) / n)
    raw = np.stack([rec["x"], rec["y"], rec["z"], rec["pad"]], axis=1)
    t_ref = {"start": times[0], "end": times[-1], "inside": 0.437}[where]
    out = T.deskew(raw, T.time_from_index(np.arange(n), n), times, poses, t_ref)
    assert np.array_equal(out[:, 3], raw[:, 3])
    Rr, pr = trajectory_poses(times, poses, [t_ref])
    carry = np.hstack([Rr[0], pr[0].reshape(3, 1)])
    err = np.linalg.norm(R.apply(carry, out[:, :3].astype(np.float64)) - world, axis=1)
    bound = 4.0 * 2.0 ** -24 * max(np.abs(raw[:, :3]).max(), np.abs(out[:, :3]).max())
    print("trajectory de-skew to %s: max %.3g m (bound %.3g m)" % (where, err.max(), bound))
    assert err.max() <= bound
    if where != "inside":
        D = TC.constant_motion(poses)
        flat = R.deskew(raw, R.alpha_from_index(np.arange(n), n), D, where == "end")
        miss = np.linalg.norm(R.apply(carry, flat[:, :3].astype(np.float64)) - world, axis=1)
        rawmiss = np.linalg.norm(R.apply(carry, raw[:, :3].astype(np.float64)) - world, axis=1)
        print("constant motion between the first and last knot: mean %.3f m, max %.3f m; raw points: mean %.3f m" % (
            miss.mean(), miss.max(), rawmiss.mean()))
        assert miss.mean() > 0.1


def test_two_knots_equal_the_constant_motion_restatement():
    """Two knots with t_ref = times[0] equal deskew_restatement.deskew(..., to_end=False) as values, on general and
    small-angle motions, from a general P_0, with index times and with times in seconds."""
    rng = np.random.default_rng(20264)
    for i in range(20):
        w = TC.unit(rng) * (rng.uniform(0.0, 0.3) if i % 4 else 10.0 ** rng.uniform(-12, -8.5))
        D = R.pose(w, TC.unit(rng) * rng.uniform(0.0, 3.0))
        P0 = R.pose(TC.unit(rng) * rng.uniform(0.0, 3.0), rng.uniform(-50, 50, 3))
        P1 = R.compose(P0, D)
        rec = np.concatenate([rng.uniform(-60, 60, (500, 3)), rng.uniform(0, 1, (500, 1))], axis=1).astype(np.float32)
        if i % 2:
            t0, t1 = 1.7e9 + 0.25, 1.7e9 + 0.35
            t = rng.uniform(t0 - 0.002, t1 + 0.002, 500)
            alpha = R.alpha_from_time(t, 1.0, t0, t1)
        else:
            t0, t1 = 0.0, 1.0
            t = T.time_from_index(rng.integers(0, 14400, 500), 14400)
            alpha = t
        t[7] = np.nan
        alpha[7] = np.nan
        got = T.deskew(rec, t, [t0, t1], [P0, P1], t0)
        want = R.deskew(rec, alpha, R.between(P0, P1), False)
        assert np.array_equal(got, want), (i, int((got != want).sum()))
        assert got[7].tobytes() == rec[7].tobytes()


DRIVER = r"""
#include "lfx.h"
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
static int fails = 0;
static void expect(int got, int want, const char * what)
{
  if (got != want) {std::printf("FAIL %s: %d, expected %d\n", what, got, want); fails++;}
}
int main()
{
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  for (unsigned n : {2u, 3u, 21u, 64u}) {
    std::vector<double> times(n), rates(3 * n), poses(12 * n), table(24 * (n - 1));
    for (unsigned j = 0; j < n; j++) {
      times[j] = 10.0 + 0.1 * j / (n - 1);
      rates[3 * j] = 0.1; rates[3 * j + 1] = -0.2; rates[3 * j + 2] = 0.6 + j * 0.05;
    }
    const double bias[3] = {0.001, 0.002, -0.001}, velocity[3] = {15.0, 0.0, 0.0};
    expect(lfx_trajectory_from_gyro(times.data(), rates.data(), n, bias, velocity, poses.data()), LFX_OK, "from_gyro");
    expect(lfx_trajectory_from_gyro(times.data(), rates.data(), n, nullptr, nullptr, poses.data()), LFX_OK, "from_gyro without bias");
    for (double t_ref : {times[0], times[n - 1], 10.033, 9.0, 11.0}) {
      lfx_trajectory tr{n, times.data(), poses.data(), t_ref};
      expect(lfx_trajectory_segments(&tr, table.data()), LFX_OK, "segments");
      for (double v : table) {
        if (!std::isfinite(v)) {std::printf("FAIL a table entry is not finite\n"); fails++; break;}
      }
    }
    lfx_trajectory tr{n, times.data(), poses.data(), nan};
    expect(lfx_trajectory_segments(&tr, table.data()), LFX_ERR_INVALID_ARGUMENT, "t_ref NaN");
    tr.t_ref = 10.0;
    tr.n_knots = 1;
    expect(lfx_trajectory_segments(&tr, table.data()), LFX_ERR_INVALID_ARGUMENT, "one knot");
    tr.n_knots = 65;
    expect(lfx_trajectory_segments(&tr, table.data()), LFX_ERR_INVALID_ARGUMENT, "65 knots");
    tr.n_knots = n;
    tr.times = nullptr;
    expect(lfx_trajectory_segments(&tr, table.data()), LFX_ERR_INVALID_ARGUMENT, "no times");
    tr.times = times.data();
    tr.poses = nullptr;
    expect(lfx_trajectory_segments(&tr, table.data()), LFX_ERR_INVALID_ARGUMENT, "no poses");
    tr.poses = poses.data();
    expect(lfx_trajectory_segments(&tr, nullptr), LFX_ERR_INVALID_ARGUMENT, "no output");
    expect(lfx_trajectory_segments(nullptr, table.data()), LFX_ERR_INVALID_ARGUMENT, "no trajectory");
    const double keep = times[n - 1];
    times[n - 1] = times[n - 2];
    expect(lfx_trajectory_segments(&tr, table.data()), LFX_ERR_INVALID_ARGUMENT, "equal times");
    expect(lfx_trajectory_from_gyro(times.data(), rates.data(), n, nullptr, nullptr, poses.data()), LFX_ERR_INVALID_ARGUMENT, "gyro equal times");
    times[n - 1] = inf;
    expect(lfx_trajectory_segments(&tr, table.data()), LFX_ERR_INVALID_ARGUMENT, "infinite time");
    expect(lfx_trajectory_from_gyro(times.data(), rates.data(), n, nullptr, nullptr, poses.data()), LFX_ERR_INVALID_ARGUMENT, "gyro infinite time");
    times[n - 1] = keep;
    poses[12 * (n - 1) + 5] = nan;
    expect(lfx_trajectory_segments(&tr, table.data()), LFX_ERR_INVALID_ARGUMENT, "NaN pose");
    expect(lfx_trajectory_from_gyro(times.data(), rates.data(), 1, nullptr, nullptr, poses.data()), LFX_ERR_INVALID_ARGUMENT, "one sample");
    expect(lfx_trajectory_from_gyro(nullptr, rates.data(), n, nullptr, nullptr, poses.data()), LFX_ERR_INVALID_ARGUMENT, "gyro no times");
    expect(lfx_trajectory_from_gyro(times.data(), nullptr, n, nullptr, nullptr, poses.data()), LFX_ERR_INVALID_ARGUMENT, "gyro no rates");
    expect(lfx_trajectory_from_gyro(times.data(), rates.data(), n, nullptr, nullptr, nullptr), LFX_ERR_INVALID_ARGUMENT, "gyro no output");
  }
  std::printf("trajectory helpers: %d failures\n", fails);
  return fails ? 3 : 0;
}
"""


def test_helpers_under_sanitizers(tmp_path):
    """lfx_pcd.cpp built alone with a small driver under -fsanitize=address,undefined (the sanitizer runtimes linked into the
    executable, as tests/test_map_files.py does it): the two host helpers on valid inputs, at 2 and 64 knots and on every
    refused input, without a sanitizer report."""
    drv = tmp_path / "driver.cpp"
    drv.write_text(DRIVER)
    exe = tmp_path / "trajectory_asan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), os.path.join(CSRC, "lfx_pose.cpp"), str(drv), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=300)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "runtime error" not in out and "Sanitizer" not in out and "FAIL" not in out, out[-4000:]
    assert "trajectory helpers: 0 failures" in out
