"""What the trajectory de-skew tests share: a sensor entering a turn, seeded trajectories, the device plumbing on top of
tests/deskew_cases.py."""
import numpy as np

from tests import deskew_cases as K
from tests import deskew_restatement as R


def unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def turning(start, knots=21, period=0.1, speed=15.0, yaw_deg=35.0, unit_time=True):
    """The sensor's true poses at `knots` evenly spaced times of one sweep: `speed` m/s along its own x, a yaw rate of
    yaw_deg / s * (1 + 2 sin(2 pi t / period)) with a little roll and pitch, integrated in 200 steps per knot interval from
    the pose `start`.  Returns (times, poses [knots][3][4]); times are fractions of the sweep (unit_time) or seconds."""
    p = np.asarray(start, np.float64).reshape(3, 4).copy()
    poses, sub = [p.copy()], 200
    h = period / (knots - 1) / sub
    for i in range((knots - 1) * sub):
        t = (i + 0.5) * h
        rate = np.array([0.1, -0.2, np.deg2rad(yaw_deg) * (1.0 + 2.0 * np.sin(2.0 * np.pi * t / period))])
        half = p[:, :3] @ R.exp_so3(rate * (0.5 * h))
        p[:, 3] = p[:, 3] + half @ np.array([speed * h, 0.0, 0.0])
        p[:, :3] = p[:, :3] @ R.exp_so3(rate * h)
        if (i + 1) % sub == 0:
            poses.append(p.copy())
    times = np.arange(knots) / (knots - 1.0)
    return (times if unit_time else times * period), np.stack(poses)


def seeded(rng, knots, small=False, t0=0.0, span=1.0):
    """A trajectory of `knots` knots over [t0, t0 + span]: uneven times, a rotation of up to 0.3 rad between knots (below
    1e-8 with `small`), positions up to 50 m from the origin."""
    cuts = np.sort(rng.uniform(0.05, 0.95, knots - 2)) if knots > 2 else np.zeros(0)
    times = t0 + span * np.concatenate([[0.0], cuts, [1.0]])
    if len(np.unique(times)) != knots:
        times = t0 + span * np.arange(knots) / (knots - 1.0)
    p = R.pose(unit(rng) * rng.uniform(0.0, 3.0), rng.uniform(-45.0, 45.0, 3))
    poses = [p]
    for _ in range(knots - 1):
        w = unit(rng) * (10.0 ** rng.uniform(-12, -8.5) if small else rng.uniform(0.0, 0.3))
        p = R.compose(p, R.pose(w, unit(rng) * rng.uniform(0.0, 5.0 / knots)))
        poses.append(p)
    return times, np.stack(poses)


def constant_motion(poses):
    """Today's model of the same sweep: the motion between the first and the last knot."""
    return R.between(poses[0], poses[-1])


def same_result(a, b):
    """Two odometry results, bit for bit (an error of NaN equals one of NaN)."""
    return a["pose"].tobytes() == b["pose"].tobytes() and (a["code"], a["iteration"], a["aligned"], a["n_edge_map"], a["n_surface_map"]) == (
        b["code"], b["iteration"], b["aligned"], b["n_edge_map"], b["n_surface_map"]) and (
        a["error"] == b["error"] or (np.isnan(a["error"]) and np.isnan(b["error"])))


def store(odo):
    """An odometry's view and its store's two clouds on the host."""
    v = odo.view()
    return v, K.d2h(v["edge_points"], v["n_edge"]), K.d2h(v["surface_points"], v["n_surface"])
