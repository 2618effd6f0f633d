"""Synthetic spinning-lidar scans in the reference's input layout.

One scan = R rings x C columns of 32-byte PointXYZIR records
(/root/reference/lib/include/lidar_feature_library/point_type.hpp:62-86; wire offsets
x0 y4 z8 pad12 intensity16 ring20, /root/reference/point_type_converter/point_type_converter/convert.py:134-145),
emitted column-major (all rings of one firing, then the next azimuth), which is the order a
driver publishes and the order the reference node receives.

Scene: the sensor stands in an axis-aligned 20 m x 12 m room with thin pillars at 3-5.5 m
(edges + occlusions), a ground plane for the downward beams, an "open door" sector whose
returns lie beyond max_range, a sector of returns closer than min_range, and isolated
single-column range spikes (parallel-beam hits).  Every range carries additive Gaussian noise
(sigma = 1 cm): that removes exact curvature ties, whose order the reference leaves to an
unstable std::sort.  No point is (0,0,0) (the upstream converter drops those, convert.py:162-163).
"""
import numpy as np

POINT_DTYPE = np.dtype({"names": ["x", "y", "z", "pad", "intensity", "ring"],
                        "formats": ["<f4", "<f4", "<f4", "<f4", "<f4", "<u2"],
                        "offsets": [0, 4, 8, 12, 16, 20], "itemsize": 32})

SENSORS = {
    # name: (rings, columns, vertical field of view in degrees)
    "plumbing-16x900": (16, 900, 15.0),
    "vlp16-16x1800": (16, 1800, 15.0),
    "hdl64-64x1800": (64, 1800, 15.0),
    "os1-128x2048": (128, 2048, 22.5),
}


def _ray_room(cx, cy, dx, dy, x0, x1, y0, y1):
    with np.errstate(divide="ignore", invalid="ignore"):
        tx = np.where(dx > 0, (x1 - cx) / dx, np.where(dx < 0, (x0 - cx) / dx, np.inf))
        ty = np.where(dy > 0, (y1 - cy) / dy, np.where(dy < 0, (y0 - cy) / dy, np.inf))
    return np.minimum(tx, ty)


def _ray_circle(cx, cy, dx, dy, px, py, rad):
    ox, oy = cx - px, cy - py
    b = ox * dx + oy * dy
    c = ox * ox + oy * oy - rad * rad
    disc = b * b - c
    t = -b - np.sqrt(np.where(disc > 0, disc, np.nan))
    return np.where((disc > 0) & (t > 0), t, np.inf)


def make_scan(rings=64, cols=1800, seed=1234, vfov_deg=15.0, sigma=0.01, n_pillars=14,
              drop_fraction=0.0, shuffle=False, start_col=0, reverse=False,
              out_of_range=True, spikes=True, sensor_pose=None):
    """Return one scan as a POINT_DTYPE array (rings*cols points, fewer with drop_fraction).

    drop_fraction  drop this share of points at random (ragged rings, as after the zero filter)
    shuffle        permute the points (forces the general ring projection, not the presorted one)
    start_col      rotate the firing sequence (scan starts at another azimuth)
    reverse        clockwise sensors: azimuth decreases with time
    sensor_pose    (x, y, yaw): the sensor moved by (x, y) metres from its usual place in the same static room and turned
                   by yaw radians about the vertical; rays are cast in the room, points are given in the sensor's frame.
                   None (the default) is the usual place and gives the same bytes as before the keyword existed.
    """
    rng = np.random.Generator(np.random.PCG64(seed))
    az = -np.pi + 2.0 * np.pi * (np.arange(cols) + 0.5) / cols
    elev = np.deg2rad(np.linspace(-vfov_deg, vfov_deg, rings))
    dx, dy = np.cos(az), np.sin(az)                 # ray directions in the sensor's frame
    cx0, cy0, h = 1.3, -0.7, 1.8                    # the sensor's usual position in the room, height over ground
    if sensor_pose is None:
        cx, cy, wx, wy = cx0, cy0, dx, dy
    else:
        mx, my, yaw = (float(v) for v in sensor_pose)
        cx, cy = cx0 + mx, cy0 + my
        wx, wy = np.cos(az + yaw), np.sin(az + yaw)  # ... and in the room's
    r = _ray_room(cx, cy, wx, wy, -10.0, 10.0, -6.0, 6.0)
    pr = np.random.Generator(np.random.PCG64(4242))  # the scene is the same for every seed
    for k in range(n_pillars):
        ang = 2.0 * np.pi * (k + 0.37) / n_pillars + pr.uniform(-0.1, 0.1)
        dist = pr.uniform(3.0, 5.5)
        r = np.minimum(r, _ray_circle(cx, cy, wx, wy, cx0 + dist * np.cos(ang), cy0 + dist * np.sin(ang),
                                      pr.uniform(0.08, 0.2)))
    r2 = np.broadcast_to(r, (rings, cols)).copy()
    # downward beams hit the ground before the wall
    with np.errstate(divide="ignore"):
        ground = np.where(elev < -1e-6, h / np.tan(-elev), np.inf)
    r2 = np.minimum(r2, ground[:, None])
    if out_of_range:
        far = (az > 2.2) & (az < 2.45)               # open door: returns beyond max_range (100 m)
        r2[:, far] = 150.0 + 5.0 * np.sin(40.0 * az[far])[None, :]
        near = (az > -0.6) & (az < -0.52)            # something on the sensor housing: < min_range
        r2[:, near] = 0.05
    r2 = r2 + sigma * rng.standard_normal((rings, cols))
    if spikes:
        n_spk = max(1, rings * cols // 700)
        rr = rng.integers(0, rings, n_spk)
        cc = rng.integers(8, cols - 8, n_spk)
        r2[rr, cc] *= rng.uniform(0.55, 0.8, n_spk)
    r2 = np.maximum(r2, 0.02)

    order = np.arange(cols)
    if reverse:
        order = order[::-1]
    order = np.roll(order, -start_col)
    pts = np.zeros(rings * cols, POINT_DTYPE)
    grid = pts.reshape(cols, rings)                  # column-major emission: [column][ring]
    rs = r2[:, order].T                              # [col][ring]
    grid["x"] = (rs * dx[order][:, None]).astype(np.float32)
    grid["y"] = (rs * dy[order][:, None]).astype(np.float32)
    grid["z"] = (rs * np.tan(elev)[None, :]).astype(np.float32)
    grid["pad"] = 1.0
    grid["intensity"] = rng.uniform(0.0, 255.0, (cols, rings)).astype(np.float32)
    grid["ring"] = np.arange(rings, dtype=np.uint16)[None, :]
    if drop_fraction > 0.0:
        keep = rng.uniform(0.0, 1.0, pts.shape[0]) >= drop_fraction
        pts = pts[keep]
    if shuffle:
        pts = pts[rng.permutation(pts.shape[0])]
    return np.ascontiguousarray(pts)


def make_batch(n_scans, rings=64, cols=1800, seed=1234, **kw):
    """n_scans scans with seeds seed, seed+1, ... (seeds 1234+scan_id)."""
    return [make_scan(rings, cols, seed + i, **kw) for i in range(n_scans)]


def make_sequence(n_scans, rings=64, cols=1800, seed=1234, step=0.05, yaw_step_deg=0.5, **kw):
    """A moving sensor in the static room: scan k is taken at (k * step, 0) metres from the usual place, turned by
    k * yaw_step_deg degrees, with seed seed + k.  Returns (clouds, poses): poses[k] is the ground truth of what odometry
    estimates, scan k's frame in scan 0's frame as 3 x 4 [R | t] (point_to_map, scan 0 = identity)."""
    clouds, poses = [], []
    for k in range(n_scans):
        x, yaw = k * step, np.deg2rad(k * yaw_step_deg)
        clouds.append(make_scan(rings, cols, seed + k, sensor_pose=(x, 0.0, yaw), **kw))
        c, s = np.cos(yaw), np.sin(yaw)
        poses.append(np.array([[c, -s, 0.0, x], [s, c, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]], np.float64))
    return clouds, np.stack(poses)


def _exp_so3(w):
    """Rotation matrices of angle-axis vectors w [..., 3] (Rodrigues)."""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w, axis=-1)[..., None, None]
    K = np.zeros(w.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -w[..., 2], w[..., 1], w[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -w[..., 0], -w[..., 1], w[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(th > 1e-12, np.sin(th) / th, 1.0)
        b = np.where(th > 1e-12, (1.0 - np.cos(th)) / (th * th), 0.5)
    return np.eye(3) + a * K + b * (K @ K)


def _log_so3(R):
    """The angle-axis vector of a rotation matrix (angles below pi)."""
    R = np.asarray(R, np.float64)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = 0.5 * np.linalg.norm(v), 0.5 * (np.trace(R) - 1.0)
    th = np.arctan2(s, c)
    return np.zeros(3) if s < 1e-300 else v * (th / (2.0 * s))


def _cast_sweep(rng, rings, cols, Rm, o, sigma, vfov_deg, n_pillars, ceiling):
    """make_sweep's room seen from the world rotations Rm [n, 3, 3] and positions o [n, 3] of the sensor at every point's
    time: (records without a time, the measured points in the world)."""
    n = rings * cols
    col, ring = np.arange(n) // rings, np.arange(n) % rings
    az = -np.pi + 2.0 * np.pi * (col + 0.5) / cols
    el = np.deg2rad(np.linspace(-vfov_deg, vfov_deg, rings))[ring]
    d_s = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1)     # unit rays, sensor frame
    d = np.einsum("nij,nj->ni", Rm, d_s)
    lo, hi = np.array([-10.0, -6.0, 0.0]), np.array([10.0, 6.0, float(ceiling)])
    with np.errstate(divide="ignore", invalid="ignore"):
        tb = np.where(d > 0, (hi - o) / d, np.where(d < 0, (lo - o) / d, np.inf))
    t = tb.min(axis=1)
    pr = np.random.Generator(np.random.PCG64(4242))      # make_scan's pillars
    a2 = d[:, 0] ** 2 + d[:, 1] ** 2
    for k in range(n_pillars):
        ang = 2.0 * np.pi * (k + 0.37) / n_pillars + pr.uniform(-0.1, 0.1)
        dist = pr.uniform(3.0, 5.5)
        rad = pr.uniform(0.08, 0.2)
        ox, oy = o[:, 0] - (1.3 + dist * np.cos(ang)), o[:, 1] - (-0.7 + dist * np.sin(ang))
        b = ox * d[:, 0] + oy * d[:, 1]
        disc = b * b - a2 * (ox * ox + oy * oy - rad * rad)
        with np.errstate(divide="ignore", invalid="ignore"):
            tp = (-b - np.sqrt(np.where(disc > 0, disc, np.nan))) / a2
        t = np.minimum(t, np.where((disc > 0) & (tp > 0), tp, np.inf))
    t = np.maximum(t + sigma * rng.standard_normal(n), 0.02)
    pts = np.zeros(n, POINT_DTYPE)
    local = t[:, None] * d_s
    pts["x"], pts["y"], pts["z"] = local[:, 0].astype(np.float32), local[:, 1].astype(np.float32), local[:, 2].astype(np.float32)
    pts["pad"] = 1.0
    pts["intensity"] = rng.uniform(0.0, 255.0, n).astype(np.float32)
    pts["ring"] = ring.astype(np.uint16)
    return pts, o + t[:, None] * d


def make_sweep(rings=16, cols=900, seed=1234, pose0=None, motion=None, sigma=0.01, vfov_deg=15.0, n_pillars=14,
               t0=0.0, period=0.1, ceiling=3.0):
    """One sweep of a sensor that MOVES while it fires: point i (column-major, i = column * rings + ring) is measured at
    alpha = i / n of the sweep, from the pose P0 M(alpha), M(alpha) = [Exp(alpha w) | alpha v] with [Exp(w) | v] = motion
    (the sensor frame at the sweep's end in its frame at the start: LOAM's model, include/lfx.h's de-skew section).  Rays
    are cast in 3-D in a closed box room (make_scan's 20 m x 12 m walls, the floor at z = 0, a ceiling) with make_scan's
    vertical pillars, Gaussian noise of sigma along the ray; every point is given in the sensor frame of its own time.

    pose0   the sensor's world pose at the start, 3 x 4 [R | t]; None: make_scan's usual place, 1.8 m over the floor
    motion  3 x 4; None: the identity (a static scan)
    Returns (records, world, alpha): POINT_DTYPE records (the point's time t0 + alpha * period also as a float32 at byte 24,
    in the record's padding), the measured points in the world [n, 3] float64, alpha [n] float64."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = rings * cols
    P0 = np.array([[1, 0, 0, 1.3], [0, 1, 0, -0.7], [0, 0, 1, 1.8]], np.float64) if pose0 is None else np.asarray(pose0, np.float64).reshape(3, 4)
    D = np.eye(4)[:3] if motion is None else np.asarray(motion, np.float64).reshape(3, 4)
    w, v = _log_so3(D[:, :3]), D[:, 3]
    alpha = np.arange(n, dtype=np.float64) / n
    Rm = P0[:, :3] @ _exp_so3(alpha[:, None] * w[None, :])                                       # world rotation at alpha
    o = (alpha[:, None] * v[None, :]) @ P0[:, :3].T + P0[:, 3]                                  # world position at alpha
    pts, world = _cast_sweep(rng, rings, cols, Rm, o, sigma, vfov_deg, n_pillars, ceiling)
    pts.view(np.uint8).reshape(n, POINT_DTYPE.itemsize)[:, 24:28] = (t0 + alpha * period).astype("<f4").view(np.uint8).reshape(n, 4)
    return np.ascontiguousarray(pts), world, alpha


def trajectory_poses(times, poses, t):
    """The sensor's pose at every time of t [n] along a trajectory (include/lfx.h, the de-skew section): between knots j and
    j + 1 the rotation along the geodesic, the position along the straight line; j = clamp(#{times[k] <= t} - 1, 0, k - 2),
    so the first and the last segment extrapolate.  Returns (R [n, 3, 3], p [n, 3])."""
    times = np.asarray(times, np.float64).reshape(-1)
    P = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    t = np.asarray(t, np.float64).reshape(-1)
    j = np.clip(np.searchsorted(times[:-1], t, side="right") - 1, 0, len(times) - 2)
    beta = (t - times[j]) * (1.0 / (times[j + 1] - times[j]))
    w = np.stack([_log_so3(P[k, :, :3].T @ P[k + 1, :, :3]) for k in range(len(times) - 1)])
    R = P[j, :, :3] @ _exp_so3(beta[:, None] * w[j])
    p = P[j, :, 3] + beta[:, None] * (P[j + 1, :, 3] - P[j, :, 3])
    return R, p


def make_sweep_trajectory(rings=16, cols=900, seed=1234, times=(0.0, 1.0), poses=None, t0=None, period=None, time_dtype="f32",
                          sigma=0.01, vfov_deg=15.0, n_pillars=14, ceiling=3.0):
    """make_sweep with the sensor's pose at a point's time taken from a trajectory (trajectory_poses): point i is measured
    at t0 + (i / n) * period (default: from the first knot's time over the span of the knots), from the world pose the knots
    times [k], poses [k][3][4] give for that time.

    time_dtype  "f32": the point's time as a float32 at byte 24, as make_sweep stores it; "f64": as a double at bytes 24 - 31
                (a knot time can then be stored exactly)
    Returns (records, world, t): POINT_DTYPE records, the measured points in the world [n, 3] float64, the times [n] float64."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = rings * cols
    times = np.asarray(times, np.float64).reshape(-1)
    t0 = times[0] if t0 is None else float(t0)
    period = times[-1] - times[0] if period is None else float(period)
    t = t0 + (np.arange(n, dtype=np.float64) / n) * period
    Rm, o = trajectory_poses(times, poses, t)
    pts, world = _cast_sweep(rng, rings, cols, Rm, o, sigma, vfov_deg, n_pillars, ceiling)
    raw = pts.view(np.uint8).reshape(n, POINT_DTYPE.itemsize)
    if time_dtype == "f64":
        raw[:, 24:32] = t.astype("<f8").view(np.uint8).reshape(n, 8)
    elif time_dtype == "f32":
        raw[:, 24:28] = t.astype("<f4").view(np.uint8).reshape(n, 4)
    else:
        raise ValueError("time_dtype must be 'f32' or 'f64'")
    return np.ascontiguousarray(pts), world, t


def concat(clouds):
    """Back-to-back copy of several scans, keeping the 32-byte record layout (np.concatenate would
    repack the fields)."""
    out = np.zeros(sum(len(c) for c in clouds), POINT_DTYPE)
    at = 0
    for c in clouds:
        out[at:at + len(c)] = c
        at += len(c)
    return out
