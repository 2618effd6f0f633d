"""Test-side restatement of the voxel filter (lfx_voxel_filter, include/lfx.h, the voxel filter section) in numpy, no GPU:
float32 floor(p * inv) for the voxel, float64 for q and the centroid, int64 sums, np.rint (nearest even), the order of first
appearance, the counts, every field of the result and the table-full rule.  tests/test_voxel_filter_expect.py holds it to
hand-written cases; tests/test_voxel_filter_gpu.py holds the device to it, byte for byte.

The module also states the kernel's hash (csrc/lfx_kernels_voxelfilter.hpp, vf_home), so that the tests can build voxels that
share a home entry, and the constants the GPU cases are built around."""
import numpy as np

LIMIT = 1 << 20                     # |voxel| < 2^20 per axis (lfx::kRollVoxelLimit)
SCALE = 16777216.0                  # 2^24
HASH = 0x9E3779B97F4A7C15           # vf_home: the top log2_slots bits of key * HASH mod 2^64
WAVE = 64                           # lanes whose equal-key runs the add merges (lfx::kVfWave)
RUN = 1024                          # records per workgroup of an add (lfx::kVfRun)
SCAN_TILE = 32768                   # ranks per workgroup of the emit's scan (lfx::kVfScanTile)
HOST_CHUNK = 1 << 16                # records per chunk of add_host


def key(vx, vy, vz):
    """roll_key (csrc/lfx_kernels_voxel.hpp): bit 63, then 21 bits per axis"""
    m = 0x1FFFFF
    return (1 << 63) | (int(vx) & m) | ((int(vy) & m) << 21) | ((int(vz) & m) << 42)


def home(k, log2_slots):
    return ((int(k) * HASH) & ((1 << 64) - 1)) >> (64 - log2_slots)


def sharing_home(log2_slots, slot, n, vy=0, vz=0):
    """the first n voxels (vx, vy, vz), vx = 0, 1, .., whose home entry is `slot`"""
    out, vx = [], 0
    while len(out) < n:
        if home(key(vx, vy, vz), log2_slots) == slot:
            out.append((vx, vy, vz))
        vx += 1
    return out


def inverse(leaf):
    return np.float32(1.0) / np.float32(leaf)


def voxel(p, inv):
    """floorf(p * inv), the product in float32: float32 array"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.floor(np.asarray(p, np.float32) * np.float32(inv))


def q_of(p, inv, v):
    """(int64) rint((((double)p * (double)inv) - (double)v) * 2^24)"""
    return np.rint((np.asarray(p, np.float32).astype(np.float64) * np.float64(inv) - np.asarray(v, np.float64)) * SCALE).astype(np.int64)


def centroid(v, s, n, inv):
    """(float)((((double)v) + ((double)S / (double)n) * 2^-24) / (double)inv)"""
    v, s, n = np.asarray(v, np.int64), np.asarray(s, np.int64), np.asarray(n, np.uint64)
    return ((v.astype(np.float64) + (s.astype(np.float64) / n.astype(np.float64)) * 2.0 ** -24) / np.float64(inv)).astype(np.float32)


class Filter:
    def __init__(self, log2_slots, max_records):
        assert 4 <= log2_slots <= 30 and 1 <= max_records <= 1 << 40
        self.slots, self.max_records = 1 << log2_slots, int(max_records)
        self.leaf = None

    def reset(self, leaf):
        leaf = np.float32(leaf)
        assert np.isfinite(leaf) and leaf > 0
        self.leaf, self.inv = leaf, inverse(leaf)
        self.base = 0
        self.vox = {}                     # (vx, vy, vz) -> [least rank, count, Sx, Sy, Sz], in order of first appearance
        self.n_nonfinite = self.n_out_of_range = self.n_table_full = self.n_accumulated = 0

    def add(self, points, keep=None):
        """records [n, 4]; keep (bool [n], optional): the others take a rank and nothing else.  'capacity' and nothing changed
        where the ranks run out."""
        p = np.asarray(points, np.float32).reshape(-1, 4)
        if self.base + len(p) > self.max_records:
            return "capacity"
        keep = np.ones(len(p), bool) if keep is None else np.asarray(keep, bool)
        xyz = p[:, :3]
        finite = np.isfinite(xyz).all(axis=1)
        v = voxel(xyz, self.inv)
        with np.errstate(invalid="ignore"):
            inside = (np.abs(v) < LIMIT).all(axis=1)
        self.n_nonfinite += int((keep & ~finite).sum())
        self.n_out_of_range += int((keep & finite & ~inside).sum())
        ok = np.nonzero(keep & finite & inside)[0]
        vi = v[ok].astype(np.int64)
        q = q_of(xyz[ok], self.inv, vi)
        for r, vv, qq in zip(ok.tolist(), map(tuple, vi.tolist()), q.tolist()):
            e = self.vox.get(vv)
            if e is None:
                if len(self.vox) == self.slots:      # no entry left (which voxel loses on the device depends on the race)
                    self.n_table_full += 1
                    continue
                e = self.vox[vv] = [self.base + r, 0, 0, 0, 0]
            e[1] += 1
            e[2] += qq[0]
            e[3] += qq[1]
            e[4] += qq[2]
            self.n_accumulated += 1
        self.base += len(p)
        return None

    def emit(self, min_points=1, capacity=None):
        """(status, cloud [n, 4] float32, counts [n] uint32, result): status 'capacity' -- and an empty cloud -- where a record
        found no entry or the voxels to write are more than `capacity`"""
        assert min_points >= 1
        live = [(vv, e) for vv, e in self.vox.items() if e[1] >= min_points]
        live.sort(key=lambda t: t[1][0])
        res = dict(n_records=self.base, n_accumulated=self.n_accumulated, n_nonfinite=self.n_nonfinite, n_out_of_range=self.n_out_of_range,
                   n_table_full=self.n_table_full, n_voxels=len(self.vox), n_written=len(live))
        if self.n_table_full or (capacity is not None and len(live) > capacity):
            return "capacity", np.zeros((0, 4), np.float32), np.zeros(0, np.uint32), res
        cloud = np.ones((len(live), 4), np.float32)
        counts = np.zeros(len(live), np.uint32)
        if live:
            v = np.array([vv for vv, _ in live], np.int64)
            e = np.array([ee for _, ee in live], np.int64)
            cloud[:, :3] = centroid(v, e[:, 2:5], e[:, 1:2], self.inv)
            counts[:] = np.minimum(e[:, 1], 0xFFFFFFFF)
        return "ok", cloud, counts, res


def filtered(points, leaf, min_points=1, log2_slots=20, keep=None):
    """one reset, one add, one emit: (cloud, counts, result)"""
    f = Filter(log2_slots, max(len(points), 1))
    f.reset(leaf)
    assert f.add(points, keep) is None
    status, cloud, counts, res = f.emit(min_points)
    assert status == "ok"
    return cloud, counts, res


def centre_points(voxels, leaf=1.0, w=7.0):
    """one record at the centre of each voxel (leaf a power of two: exact)"""
    v = np.asarray(voxels, np.float64).reshape(-1, 3)
    out = np.full((len(v), 4), w, np.float32)
    out[:, :3] = (v + 0.5) * leaf
    return out
