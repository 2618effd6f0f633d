"""The rolling voxel map of include/lfx.h (lfx_rolling_map_*) restated in numpy: voxel, key, slot, window, the insert rule
and the order of an extraction, bit for bit.  One Store per kind; the transform is the odometry's
(tests/odometry_restatement.transform).  tests/test_rolling_map_expect.py pins it on cases written out by hand."""
import numpy as np

from tests.odometry_restatement import transform

LIMIT = np.float32(2 ** 20)
MASK = 0x1FFFFF


def inverse_leaf(leaf):
    return np.float32(1.0) / np.float32(leaf)


def voxel_axis(p, inv):
    """(floorf(p * inv) as float32, whether it names a voxel) for an array of coordinates"""
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.floor(np.asarray(p, np.float32) * np.float32(inv))
        ok = np.abs(f) < LIMIT              # (false for NaN and the infinities)
    return f, ok


def voxels(points, inv):
    """int64 [n, 3] voxels of points [n, >= 3] and which points have one (the others' rows are 0)"""
    p = np.asarray(points, np.float32).reshape(len(points), -1)[:, :3]
    f, ok = voxel_axis(p, inv)
    ok = ok.all(axis=1)
    v = np.zeros(p.shape, np.int64)
    v[ok] = f[ok].astype(np.int64)
    return v, ok


def key(v):
    vx, vy, vz = (int(x) for x in v)
    return (1 << 63) | (vx & MASK) | ((vy & MASK) << 21) | ((vz & MASK) << 42)


class Store:
    def __init__(self, leaf, dims):
        self.leaf = np.float32(leaf)
        self.inv = inverse_leaf(leaf)
        self.n = tuple(int(d) for d in dims)
        self.o = tuple(-(d // 2) for d in self.n)
        self.keys, self.points = {}, {}      # by slot, the written ones only (a key: a python int, 64 bits without a sign)
        self.counts = dict(inserted=0, merged=0, outside=0, nonfinite=0)

    def slot(self, v):
        sx, sy, sz = (int(v[a]) % self.n[a] for a in range(3))    # (python's % is the non-negative modulus)
        return (sz * self.n[1] + sy) * self.n[0] + sx

    def inside(self, v):
        return all(self.o[a] <= int(v[a]) < self.o[a] + self.n[a] for a in range(3))

    def live(self, v):
        return self.inside(v) and self.keys.get(self.slot(v), 0) == key(v)

    def recenter(self, center):
        c = np.asarray(center, np.float64).astype(np.float32)
        f, ok = voxel_axis(c, self.inv)
        assert ok.all()
        self.o = tuple(int(f[a]) - self.n[a] // 2 for a in range(3))

    def insert(self, clouds, poses):
        """One call: clouds in the order of their index (where they lie in memory is not the restatement's business).  The
        first record in (cloud, index) order to reach a voxel that is not live is stored; the later ones find it live."""
        for cloud, pose in zip(clouds, poses):
            c = np.asarray(cloud, np.float32).reshape(-1, 4)
            if len(c) == 0:
                continue
            q = transform(pose, c)
            v, ok = voxels(q, self.inv)
            for i in range(len(q)):
                if not ok[i]:
                    self.counts["nonfinite"] += 1
                elif not self.inside(v[i]):
                    self.counts["outside"] += 1
                elif self.live(v[i]):
                    self.counts["merged"] += 1
                else:
                    s = self.slot(v[i])
                    self.keys[s] = key(v[i])
                    self.points[s] = q[i]
                    self.counts["inserted"] += 1

    def box(self, lo, hi):
        """the inclusive voxel ranges of the box lo .. hi (m) clipped to the window, or None"""
        out = []
        for a in range(3):
            with np.errstate(over="ignore"):
                fl = np.floor(np.float32(np.float64(lo[a])) * self.inv)
                fh = np.floor(np.float32(np.float64(hi[a])) * self.inv)
            first = int(min(max(fl, -LIMIT), LIMIT - np.float32(1)))
            last = int(min(max(fh, -LIMIT), LIMIT - np.float32(1)))
            first = max(first, self.o[a], -2 ** 20)
            last = min(last, self.o[a] + self.n[a] - 1, 2 ** 20 - 1)
            if last < first:
                return None
            out.append((first, last))
        return out

    def extract(self, lo, hi):
        """the live voxels of the box in ascending (vz, vy, vx).  A written slot holds the voxel its key names; that voxel is
        live where it lies in the window, and the box is clipped to the window."""
        b = self.box(lo, hi)
        if b is None or not self.keys:
            return np.zeros((0, 4), np.float32)
        slots = np.array(list(self.keys.keys()), np.int64)
        keys = np.array(list(self.keys.values()), np.uint64)
        v = []
        for a in range(3):
            c = ((keys >> np.uint64(21 * a)) & np.uint64(MASK)).astype(np.int64)
            v.append(np.where(c >= 2 ** 20, c - 2 ** 21, c))            # 21 bits, two's complement
        keep = np.ones(len(keys), bool)
        for a in range(3):
            keep &= (v[a] >= b[a][0]) & (v[a] <= b[a][1])
        order = np.lexsort((v[0][keep], v[1][keep], v[2][keep]))
        return np.array([self.points[s] for s in slots[keep][order]], np.float32).reshape(-1, 4)

    def window(self):
        """the whole window in metres (voxel centres of its corners)"""
        lo = [(self.o[a] + 0.5) * float(self.leaf) for a in range(3)]
        hi = [(self.o[a] + self.n[a] - 0.5) * float(self.leaf) for a in range(3)]
        return lo, hi

    def extract_all(self):
        return self.extract(*self.window())


def compose(a, b):
    """a x b for poses [R | t] (3 x 4) in double, every 3-term sum as (a0 b0 + a1 b1) + a2 b2, the translation's + t"""
    a, b = np.asarray(a, np.float64).reshape(3, 4), np.asarray(b, np.float64).reshape(3, 4)
    out = np.zeros((3, 4))
    for i in range(3):
        for j in range(4):
            v = (a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]
            out[i, j] = v + a[i, 3] if j == 3 else v
    return out


def inverse(a):
    """[R^T | -(R^T t)] with the same sums"""
    a = np.asarray(a, np.float64).reshape(3, 4)
    out = np.zeros((3, 4))
    for i in range(3):
        out[i, :3] = a[:3, i]
        out[i, 3] = -((a[0, i] * a[0, 3] + a[1, i] * a[1, 3]) + a[2, i] * a[2, 3])
    return out


NOT_RUN = 6                                  # LFX_ALIGN_NOT_RUN


class RollingMap:
    """The two stores ('edge', 'surface') under one recentring and lfx_rolling_map_update_batch's loop over them.  align: a
    callable (edge_box, surface_box, scan, initial_pose) -> dict(pose, code, success, ...), the place of the optimizer --
    the oracle's (oracle_align), or a replay of what a device reported."""

    def __init__(self, edge_leaf=0.2, surface_leaf=0.4, edge_dims=(512, 512, 128), surface_dims=(256, 256, 64),
                 match_half_extent=(50.0, 50.0, 12.8), n_neighbors=15, initial_pose=None):
        self.stores = dict(edge=Store(edge_leaf, edge_dims), surface=Store(surface_leaf, surface_dims))
        self.half = np.asarray(match_half_extent, np.float32).astype(np.float64)
        self.k = n_neighbors
        self.pose = np.eye(4)[:3].copy() if initial_pose is None else np.asarray(initial_pose, np.float64).reshape(3, 4).copy()
        self.correction = np.eye(4)[:3].copy()

    def recenter(self, center):
        for s in self.stores.values():
            s.recenter(center)

    def wants_recentre(self, t):
        for s in self.stores.values():
            f, ok = voxel_axis(np.asarray(t, np.float64).astype(np.float32), s.inv)
            assert ok.all()
            for a in range(3):
                if abs(int(f[a]) - (s.o[a] + s.n[a] // 2)) > s.n[a] // 4:
                    return True
        return False

    def boxes(self, t):
        t = np.asarray(t, np.float64)
        return self.stores["edge"].extract(t - self.half, t + self.half), self.stores["surface"].extract(t - self.half, t + self.half)

    def update(self, scan, align, odom=None):
        """One scan (edge cloud, surface cloud: raw records) through the loop.  Returns what lfx_rolling_map_result holds, and
        the boxes the scan met under 'edge_box' / 'surface_box'."""
        initial = self.pose.copy() if odom is None else compose(self.correction, odom)
        t = initial[:, 3]
        r = dict(initial_pose=initial, recentered=self.wants_recentre(t), aligned=False, inserted=True, code=NOT_RUN, pose=initial)
        if r["recentered"]:
            self.recenter(t)
        eb, sb = self.boxes(t)
        r.update(edge_box=eb, surface_box=sb, n_edge_map=len(eb), n_surface_map=len(sb))
        pose = initial
        if len(eb) >= self.k and len(sb) >= self.k:
            got = align(eb, sb, scan, initial)
            r.update(got, aligned=True)
            if got["success"]:
                pose = np.asarray(got["pose"], np.float64).reshape(3, 4)
                if odom is not None:
                    self.correction = compose(pose, inverse(odom))
            else:
                r["inserted"] = False
        if r["inserted"]:
            self.stores["edge"].insert([scan[0]], [pose])
            self.stores["surface"].insert([scan[1]], [pose])
        self.pose = pose.copy()
        return r


def oracle_align(k=15, max_iter=20, leaf=1.0):
    """Optimizer::Run by the oracle over a scan's edge cloud and its downsampled surface cloud"""
    from tests.odometry_restatement import downsample, optimize_scan

    def align(edge_box, surface_box, scan, initial):
        return optimize_scan(edge_box, surface_box, k, scan[0], downsample(scan[1], leaf), initial, max_iter)
    return align
