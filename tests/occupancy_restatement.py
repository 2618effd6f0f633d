"""numpy / pure-Python restatement of the occupancy section of include/lfx.h, written from the model there: the reduce of a
scan to W beams (gates, levelled direction, the bisection over the column tables, the two winners per column), the render
(origin and end cells, the skipped beams, the integer Bresenham, one vote per cell and scan with a hit beating a miss), the
emit through the look-up table, and the map.pgm / map.yaml bytes -- operation for operation in float64, unfused, so that the
device's beams, counts, counters and bytes can be compared byte for byte.  The column tables come from the library
(lfx_occupancy_tables, host only), as the device's do; the look-up table is restated here (libm's exp, as the library's) and
held to the library's in tests/test_occupancy_files.py."""
import math

import numpy as np

from lidar_feature_extraction_amd import occupancy_config, occupancy_emit_config, occupancy_tables

NONE, HIT, CLEAR = 0, 1, 2
CELL_LIMIT = float(1 << 30)
COUNTERS = ("n_hit_beams", "n_clear_beams", "n_skipped_beams", "n_occupied_votes", "n_free_votes", "n_window_miss")


def config(**fields):
    return occupancy_config(None, **fields)


def emit_config(**fields):
    return occupancy_emit_config(None, **fields)


# --- reduce ------------------------------------------------------------------------------------------------------------------
def columns(cs, sn, dx, dy):
    """The header's bisection for float64 directions: the column of every direction."""
    W = len(cs)
    m0 = np.where(dy >= 0.0, W // 2, 0).astype(np.int64)
    lo, hi = np.zeros(len(dx), np.int64), np.full(len(dx), W // 2 - 1, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        while (lo < hi).any():
            mid = (lo + hi + 1) >> 1
            m = m0 + mid
            ge = (cs[m] * dy - sn[m] * dx) >= 0.0
            go = lo < hi
            lo = np.where(go & ge, mid, lo)
            hi = np.where(go & ~ge, mid - 1, hi)
    return m0 + lo


def candidates(cfg, x, y, z, pose, cls=None, obstacle_mask=15, clear_mask=15):
    """Per record of a scan (float32 coordinates, the scan's pose [3][4]): (obstacle [n] bool, clear [n] bool, column [n],
    kf [n] float32, dz [n] float64)."""
    cs, sn = occupancy_tables(cfg)
    x, y, z = (np.asarray(a, np.float32) for a in (x, y, z))
    xd, yd, zd = (a.astype(np.float64) for a in (x, y, z))
    p = np.asarray(pose, np.float64).reshape(3, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        xy2 = xd * xd + yd * yd
        r = np.sqrt(xy2 + zd * zd)
        keep = np.isfinite(xd) & np.isfinite(yd) & np.isfinite(zd) & ~(xy2 == 0.0)
        keep &= ~(r < np.float64(cfg.min_range)) & ~(r >= np.float64(cfg.max_range))
        dx = (p[0, 0] * xd + p[0, 1] * yd) + p[0, 2] * zd
        dy = (p[1, 0] * xd + p[1, 1] * yd) + p[1, 2] * zd
        dz = (p[2, 0] * xd + p[2, 1] * yd) + p[2, 2] * zd
        h2 = dx * dx + dy * dy
        keep &= ~(h2 == 0.0)
        kf = h2.astype(np.float32)
        band = (np.float64(cfg.z_min) <= dz) & (dz <= np.float64(cfg.z_max))
    col = columns(cs, sn, dx, dy)
    if cls is None:
        ok_obstacle = ok_clear = np.ones(len(x), bool)
    else:
        c = np.asarray(cls, np.int64)
        ok_obstacle = (c < 4) & (((int(obstacle_mask) >> np.minimum(c, 4)) & 1) == 1)
        ok_clear = (c < 4) & (((int(clear_mask) >> np.minimum(c, 4)) & 1) == 1)
    obstacle = keep & band & ok_obstacle
    clear = keep & ~obstacle & ok_clear
    return obstacle, clear, col, kf, dz


def reduce_scan(cfg, x, y, z, pose, cls=None, obstacle_mask=15, clear_mask=15):
    """(xyz [W][3] float32, kind [W] uint32): the beams of one scan."""
    W = int(cfg.n_beams)
    x, y, z = (np.asarray(a, np.float32) for a in (x, y, z))
    xyz, kind = np.zeros((W, 3), np.float32), np.zeros(W, np.uint32)
    if len(x) == 0:
        return xyz, kind
    obstacle, clear, col, kf, _ = candidates(cfg, x, y, z, pose, cls, obstacle_mask, clear_mask)
    bits = kf.view(np.uint32).astype(np.int64)             # (kf is not negative: its bits order as it does)
    idx = np.arange(len(x), dtype=np.int64)
    for who, what, key in ((clear, CLEAR, -bits), (obstacle, HIT, bits)):          # (an obstacle winner overwrites a clear one)
        i = idx[who]
        if len(i) == 0:
            continue
        order = np.lexsort((i, key[who], col[who]))                                # column, then the key, then the lower index
        c = col[who][order]
        first = np.concatenate([[True], c[1:] != c[:-1]])
        w = i[order][first]
        xyz[c[first]] = np.stack([x[w], y[w], z[w]], axis=1)
        kind[c[first]] = what
    return xyz, kind


# --- render ------------------------------------------------------------------------------------------------------------------
def line_cells(ox, oy, ex, ey):
    """The header's Bresenham, in Python integers: every cell from (ox, oy) to (ex, ey), the end cell last."""
    ax, ay = abs(ex - ox), abs(ey - oy)
    sx, sy = (ex > ox) - (ex < ox), (ey > oy) - (ey < oy)
    err, x, y = ax - ay, ox, oy
    out = []
    for _ in range(max(ax, ay) + 1):
        out.append((x, y))
        if (x, y) == (ex, ey):
            break
        e2 = 2 * err
        if e2 > -ay:
            err -= ay
            x += sx
        if e2 < ax:
            err += ax
            y += sy
    return out


def cell_of(v, origin, inv_res):
    """floor((v - origin) * inv_res) as an integer, or None where it is not finite or not below 2^30 in size."""
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor((np.float64(v) - np.float64(origin)) * np.float64(inv_res))
    if not (abs(c) < CELL_LIMIT):
        return None
    return int(c)


def inv_res_of(cfg):
    return np.float64(1.0) / np.float64(np.float32(cfg.resolution))


def reach_of(cfg):
    """A scan's window reaches so many cells from its origin cell on either side (its side: 2 * ceil(max_range * inv_res) + 5)."""
    return int(math.ceil(float(np.float64(np.float32(cfg.max_range)) * inv_res_of(cfg)))) + 2


def end_cells(cfg, xyz, kind, pose):
    """Per beam of one scan: (ok [W] bool, ox, oy, ex [W], ey [W]) -- ok: kind != NONE and the four coordinates are cells."""
    p = np.asarray(pose, np.float64).reshape(3, 4)
    inv = inv_res_of(cfg)
    b = np.asarray(xyz, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        wx = ((p[0, 0] * b[:, 0] + p[0, 1] * b[:, 1]) + p[0, 2] * b[:, 2]) + p[0, 3]
        wy = ((p[1, 0] * b[:, 0] + p[1, 1] * b[:, 1]) + p[1, 2] * b[:, 2]) + p[1, 3]
    ox, oy = cell_of(p[0, 3], cfg.origin_x, inv), cell_of(p[1, 3], cfg.origin_y, inv)
    ex = [cell_of(v, cfg.origin_x, inv) for v in wx]
    ey = [cell_of(v, cfg.origin_y, inv) for v in wy]
    ok = np.array([k != NONE and ox is not None and oy is not None and a is not None and c is not None for k, a, c in zip(kind, ex, ey)], bool)
    z = lambda v: 0 if v is None else v
    return ok, z(ox), z(oy), np.array([z(v) for v in ex], np.int64), np.array([z(v) for v in ey], np.int64)


def scan_votes(cfg, xyz, kind, pose):
    """(occupied [h][w] bool, free [h][w] bool, counters dict) of one scan: all its beams walked in step, one Bresenham step
    per turn (the line of every beam is line_cells's: tests/test_occupancy_expect.py holds the two together)."""
    w, h = int(cfg.width), int(cfg.height)
    kind = np.asarray(kind, np.uint32)
    passed, hit_end = np.zeros((h, w), bool), np.zeros((h, w), bool)
    ok, ox, oy, ex, ey = end_cells(cfg, xyz, kind, pose)
    live = kind != NONE
    res = dict.fromkeys(COUNTERS, 0)
    res["n_skipped_beams"] = int((live & ~ok).sum())
    res["n_hit_beams"] = int((ok & (kind == HIT)).sum())
    res["n_clear_beams"] = int((ok & (kind == CLEAR)).sum())
    if ok.any():
        ex, ey, hit = ex[ok], ey[ok], (kind[ok] == HIT)
        ax, ay = np.abs(ex - ox), np.abs(ey - oy)
        sx, sy = np.sign(ex - ox), np.sign(ey - oy)
        steps = np.maximum(ax, ay) + 1
        err, x, y = ax - ay, np.full(len(ex), ox, np.int64), np.full(len(ex), oy, np.int64)
        reach = reach_of(cfg)
        for step in range(int(steps.max())):
            active = step < steps
            last = step == steps - 1
            inside = active & (x >= 0) & (x < w) & (y >= 0) & (y < h)
            window = (np.abs(x - ox) <= reach) & (np.abs(y - oy) <= reach)
            res["n_window_miss"] += int((inside & ~window).sum())
            inside &= window
            end_hit = inside & last & hit
            hit_end[y[end_hit], x[end_hit]] = True
            free = inside & ~(last & hit)
            passed[y[free], x[free]] = True
            e2 = 2 * err
            mx, my = active & ~last & (e2 > -ay), active & ~last & (e2 < ax)
            err = err - np.where(mx, ay, 0) + np.where(my, ax, 0)
            x = x + np.where(mx, sx, 0)
            y = y + np.where(my, sy, 0)
    occupied = hit_end
    free = passed & ~hit_end
    res["n_occupied_votes"], res["n_free_votes"] = int(occupied.sum()), int(free.sum())
    return occupied, free, res


class Grid:
    """The object: beams and poses kept per scan, counts and counters accumulated by render, zeroed by clear."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.xyz, self.kind, self.pose = [], [], []
        self.clear()

    def clear(self):
        self.hits = np.zeros((int(self.cfg.height), int(self.cfg.width)), np.uint32)
        self.misses = np.zeros_like(self.hits)
        self.counters = dict.fromkeys(COUNTERS, 0)

    def __len__(self):
        return len(self.pose)

    def add_beams(self, xyz, kind, pose):
        self.xyz.append(np.asarray(xyz, np.float32).reshape(-1, 3))
        self.kind.append(np.asarray(kind, np.uint32))
        self.pose.append(np.array(pose, np.float64).reshape(3, 4))

    def add_scans(self, clouds, poses, select=None, classes=None, obstacle_mask=15, clear_mask=15):
        """lfx_occupancy_add_batch: clouds with x, y, z fields, one pose each; classes: per cloud or None."""
        for s, (c, p) in enumerate(zip(clouds, poses)):
            if select is not None and not select[s]:
                continue
            self.add_beams(*reduce_scan(self.cfg, c["x"], c["y"], c["z"], p, None if classes is None else classes[s], obstacle_mask, clear_mask), p)

    def beams(self):
        W = int(self.cfg.n_beams)
        if not self.xyz:
            return np.zeros((0, W, 3), np.float32), np.zeros((0, W), np.uint32)
        return np.stack(self.xyz), np.stack(self.kind)

    def set_poses(self, poses, first=0):
        for k, p in enumerate(np.asarray(poses, np.float64).reshape(-1, 3, 4)):
            self.pose[first + k] = p.copy()

    def render(self, first=0, count=None):
        count = len(self) - first if count is None else count
        for k in range(first, first + count):
            occupied, free, res = scan_votes(self.cfg, self.xyz[k], self.kind[k], self.pose[k])
            self.hits += occupied.astype(np.uint32)
            self.misses += free.astype(np.uint32)
            for n in COUNTERS:
                self.counters[n] += res[n]

    def emit(self, ecfg=None):
        return emit(self.hits, self.misses, ecfg if ecfg is not None else emit_config())


# --- emit --------------------------------------------------------------------------------------------------------------------
def emit_table(ecfg):
    """lut[j] = (int8) rint(100.0 / (1.0 + exp(-(double)(l_min + j) / 100.0))), j = 0 .. l_max - l_min."""
    out = []
    for l in range(int(ecfg.l_min), int(ecfg.l_max) + 1):
        try:
            e = math.exp(-float(l) / 100.0)
        except OverflowError:
            e = math.inf
        out.append(int(np.rint(100.0 / (1.0 + e))))
    return np.array(out, np.int8)


def emit(hits, misses, ecfg):
    """int8 [h][w]: -1 under min_observations, else the table at the clamped log-odds."""
    h, m = np.asarray(hits, np.uint32).astype(np.int64), np.asarray(misses, np.uint32).astype(np.int64)
    lut = emit_table(ecfg)
    L = np.clip(h * int(ecfg.w_hit) - m * int(ecfg.w_miss), int(ecfg.l_min), int(ecfg.l_max))
    return np.where(h + m < int(ecfg.min_observations), np.int8(-1), lut[L - int(ecfg.l_min)]).astype(np.int8)


# --- files -------------------------------------------------------------------------------------------------------------------
def pgm_bytes(grid, occupied_percent=65, free_percent=25):
    g = np.asarray(grid, np.int8)
    v = g.astype(np.int64)
    px = np.where(v == -1, 205, np.where(v >= occupied_percent, 0, np.where(v <= free_percent, 254, 205))).astype(np.uint8)
    return b"P5\n%d %d\n255\n" % (g.shape[1], g.shape[0]) + px[::-1].tobytes()


def yaml_bytes(resolution, origin_x, origin_y, occupied_percent=65, free_percent=25):
    return ("image: map.pgm\nresolution: %.17g\norigin: [%.17g, %.17g, 0.0]\nnegate: 0\noccupied_thresh: %.17g\nfree_thresh: %.17g\n" % (
        float(np.float32(resolution)), float(origin_x), float(origin_y), occupied_percent / 100.0, free_percent / 100.0)).encode()
