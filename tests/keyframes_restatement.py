"""Test-side restatement of the keyframe store (lfx_keyframes, include/lfx.h) in numpy, no GPU: sensor-frame records per
keyframe and kind, one pose per keyframe, the world cloud of a range of keyframes (tests/odometry_restatement.transform per
keyframe: every coordinate ((r0*x + r1*y) + r2*z) + t in double rounded once to float, the 4th float copied), the submap's
selection ((dx^2 + dy^2) + dz^2 <= radius^2 in double, d = t - centre), its cut at a capacity and its result record.
tests/test_keyframes_expect.py holds it to hand-written cases; tests/test_keyframes_gpu.py holds the device to it, byte for
byte.  The module also makes the clouds and poses both files use."""
import functools

import numpy as np

from tests.odometry_restatement import transform

EDGE, SURFACE = 0, 1
# lfx::kKfRun (csrc/lfx_kernels_keyframes.hpp): the source records one workgroup of the transform kernel has, kKfThreads (256)
# lanes x kKfPerLane (4) records; a wave takes 64 consecutive records in each of its four steps (kKfWave)
RUN, WAVE = 1024, 64
DRAWN = (0, 0, 0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)


class Store:
    def __init__(self, max_keyframes, max_points):
        self.max_keyframes = int(max_keyframes)
        self.max_points = (max_points, max_points) if np.isscalar(max_points) else tuple(max_points)
        self.clouds = ([], [])                      # per kind, per keyframe: [n, 4] float32, sensor frame
        self.pose = []                              # per keyframe: [3, 4] float64

    def __len__(self):
        return len(self.pose)

    def begin(self, kind):
        """the exclusive prefix of the counts: [n + 1] uint64"""
        return np.concatenate([[0], np.cumsum([len(c) for c in self.clouds[kind]])]).astype(np.uint64)

    def records(self, kind):
        return np.concatenate(self.clouds[kind] + [np.zeros((0, 4), np.float32)])

    def add(self, edge, surface, poses):
        """n keyframes (edge[s], surface[s] at poses[s]); 'capacity' / 'invalid' and nothing changed where the device refuses"""
        poses = np.asarray(poses, np.float64).reshape(-1, 3, 4)
        if not np.isfinite(poses).all():
            return "invalid"
        if len(self) + len(poses) > self.max_keyframes:
            return "capacity"
        for kind, clouds in ((EDGE, edge), (SURFACE, surface)):
            if int(self.begin(kind)[-1]) + sum(len(c) for c in clouds) > self.max_points[kind]:
                return "capacity"
        first = len(self)
        for e, s, p in zip(edge, surface, poses):
            self.clouds[EDGE].append(np.array(e, np.float32).reshape(-1, 4))
            self.clouds[SURFACE].append(np.array(s, np.float32).reshape(-1, 4))
            self.pose.append(p.copy())
        return first

    def set_poses(self, poses, first=0):
        for k, p in enumerate(np.asarray(poses, np.float64).reshape(-1, 3, 4)):
            self.pose[first + k] = p.copy()

    def poses(self):
        return np.array(self.pose).reshape(-1, 3, 4)

    def build(self, kind, first=0, count=None, keyframes=None):
        """the world cloud of keyframes [first, first + count) (or of the listed ones) at the current poses"""
        ks = range(first, len(self) if count is None else first + count) if keyframes is None else keyframes
        return np.concatenate([transform(self.pose[k], self.clouds[kind][k]) for k in ks] + [np.zeros((0, 4), np.float32)])

    def select(self, center, radius, first=0, count=None):
        """which keyframes of the window lie within the radius: bool [count]"""
        count = len(self) - first if count is None else count
        c = np.asarray(center, np.float64)
        t = self.poses()[first:first + count, :, 3].reshape(-1, 3)
        dx, dy, dz = t[:, 0] - c[0], t[:, 1] - c[1], t[:, 2] - c[2]
        return (dx * dx + dy * dy) + dz * dz <= np.float64(radius) * np.float64(radius)

    def submap(self, kind, center, radius, first=0, count=None, capacity=None):
        """(cloud, result): the selected keyframes in ascending id, each whole, until the first that would pass `capacity`"""
        sel = self.select(center, radius, first, count)
        ids = [first + int(k) for k in np.nonzero(sel)[0]]
        written, n = [], 0
        for k in ids:
            c = len(self.clouds[kind][k])
            if capacity is not None and n + c > capacity:
                break
            written.append(k)
            n += c
        res = dict(n_selected=len(ids), n_written_keyframes=len(written), n_points=n, first_id=written[0] if written else None,
                   last_id=written[-1] if written else None, truncated=len(written) < len(ids))
        return self.build(kind, keyframes=written), res


# --- the cases -------------------------------------------------------------------------------------------------------------------
def rotation(axis_angle):
    th = np.asarray(axis_angle, np.float64)
    k = np.linalg.norm(th)
    if k == 0:
        return np.eye(3)
    u = th / k
    Kx = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + np.sin(k) * Kx + (1 - np.cos(k)) * Kx @ Kx


def pose(axis_angle, t):
    return np.hstack([rotation(axis_angle), np.asarray(t, np.float64).reshape(3, 1)])


def bits_counts():
    """The counts of the `build` case, per keyframe.  First a staircase that puts a keyframe boundary at -1, 0 and +1 of every
    multiple of 64 up to 4096 (63, 1, 1, then 62, 1, 1 again and again); then 100 counts drawn from DRAWN with, inside them,
    a run of 300 one-record keyframes and a run of 40 empty ones.  (100 draws, not 200: the drawn counts average 542 records,
    and the cloud stays at about 60 000.)"""
    rng = np.random.default_rng(20250)
    stairs = [63, 1, 1] + [62, 1, 1] * 63
    drawn = [int(c) for c in rng.choice(DRAWN, 100)]
    return stairs + drawn[:30] + [1] * 300 + drawn[30:60] + [0] * 40 + drawn[60:]


def bits_clouds(counts, seed):
    """records for the counts: coordinates N(0, 40), random 4th floats, and among them -0.0, subnormals and +-inf"""
    rng = np.random.default_rng(seed)
    all_ = rng.normal(0, 40, (int(sum(counts)), 4)).astype(np.float32)
    special = np.array([-0.0, 1e-45, -3e-42, np.inf, -np.inf, 0.0], np.float32)
    where = rng.choice(all_.size, min(all_.size, 600), replace=False)
    all_.reshape(-1)[where] = special[rng.integers(0, len(special), len(where))]
    all_[0] = [-0.0, -0.0, -0.0, -0.0]
    at = np.concatenate([[0], np.cumsum(counts)])
    return [all_[at[k]:at[k + 1]].copy() for k in range(len(counts))]


def bits_poses(n, seed):
    rng = np.random.default_rng(seed)
    return np.array([pose(rng.normal(0, 1.5, 3), rng.normal(0, 60, 3)) for _ in range(n)])


@functools.lru_cache(maxsize=None)
def bits_case():
    """(store, edge clouds, surface clouds, poses) of the `build` case: the surface counts are the edge counts reversed"""
    counts = bits_counts()
    edge, surface = bits_clouds(counts, 1), bits_clouds(counts[::-1], 2)
    poses = bits_poses(len(counts), 3)
    s = Store(len(counts), (sum(counts), sum(counts)))
    assert s.add(edge, surface, poses) == 0
    return s, edge, surface, poses


def bits_ranges(begin):
    """(first, count) of the range builds: ranges that start and end inside a workgroup's run (their first record's offset
    into a run of RUN, and their length, are no multiples of RUN or WAVE), the whole store, a range of only empty keyframes,
    a range of one keyframe, and the last keyframe alone"""
    n = len(begin) - 1
    counts = np.diff(begin.astype(np.int64))
    empty = next(k for k in range(n - 5) if (counts[k:k + 5] == 0).all())
    one = next(k for k in range(n) if counts[k] == 4097)
    return [(0, n), (200, n - 260), (195, 400), (empty, 5), (one, 1), (n - 1, 1), (7, 0)]


def sphere_case():
    """The hand case of the selection: keyframes on, inside and just outside two spheres.  Centre (1, 2, 3).  Radius 5:
    t - centre = (3, 4, 0) and (0, -5, 0) are ON the sphere (9 + 16 = 25 exactly: in), (3, 4, 0) with x one float64 step
    further out is out, (1, 1, 1) is in, (4, 4, 0) is out.  Radius 7: (2, 3, 6) is on (4 + 9 + 36 = 49: in)."""
    c = np.array([1.0, 2.0, 3.0])
    d = [(3, 4, 0), (0, -5, 0), (np.nextafter(4.0, 5.0) - 1.0, 4, 0), (1, 1, 1), (4, 4, 0), (2, 3, 6), (2, 3, np.nextafter(9.0, 10.0) - 3.0)]
    poses = np.array([pose([0.0, 0.0, 0.1 * k], c + np.array(v, np.float64)) for k, v in enumerate(d)])
    assert poses[2, 0, 3] == np.nextafter(4.0, 5.0) and poses[6, 2, 3] == np.nextafter(9.0, 10.0)
    rng = np.random.default_rng(5)
    counts = [3, 2, 4, 0, 5, 6, 1]
    edge = [rng.normal(0, 10, (k, 4)).astype(np.float32) for k in counts]
    surface = [rng.normal(0, 10, (k + 1, 4)).astype(np.float32) for k in counts]
    s = Store(len(counts), (sum(counts), sum(counts) + len(counts)))
    assert s.add(edge, surface, poses) == 0
    return s, c, edge, surface, poses


SPHERE_WANT = {5.0: [True, True, False, True, False, False, False], 7.0: [True, True, True, True, True, True, False]}
