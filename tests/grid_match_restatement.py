"""The grid-match section of include/lfx.h restated in numpy: the score table, the score field, the scans' points, the
candidate arithmetic, `score`, `search` with its tie rule, slice_best and volume, `candidate` and `pose3`.  Doubles, one
operation at a time, in the header's order; cosines, sines and exponentials come from `math`, so the host's libm is the
source the library shares.  tests/test_grid_match_expect.py holds this file to a triple-loop brute force and to hand values,
tests/test_grid_match_gpu.py holds the device to it bit for bit."""
import math

import numpy as np

FAR = 0xFFFFFFFF
HIT = 1
MAX_CELLS, MAX_HALF, MAX_HALF_THETA = 64, 256, 180
LIMIT = 2.0 ** 30
f32 = np.float32


def geometry(width, height, resolution, origin_x=0.0, origin_y=0.0):
    return dict(width=int(width), height=int(height), resolution=float(f32(resolution)), origin_x=float(origin_x), origin_y=float(origin_y))


def table_config(**fields):
    cfg = dict(sigma=0.2, max_distance=2.0, peak=1000)
    cfg.update(fields)
    return dict(sigma=float(f32(cfg["sigma"])), max_distance=float(f32(cfg["max_distance"])), peak=int(cfg["peak"]))


def table_cells(cfg, resolution):
    return int(math.ceil(cfg["max_distance"] / float(f32(resolution))))


def table(cfg, resolution):
    res, rs = float(f32(resolution)), table_cells(cfg, resolution)
    assert rs <= MAX_CELLS
    denom = (2.0 * cfg["sigma"]) * cfg["sigma"]
    lut = np.zeros(rs * rs + 1, np.uint16)
    for k in range(rs * rs + 1):
        d = math.sqrt(float(k)) * res
        lut[k] = 0 if d > cfg["max_distance"] else int(round(float(cfg["peak"]) * math.exp(-(d * d) / denom)))
    return lut


def field(d2, lut):
    d2 = np.asarray(d2, np.uint32)
    inside = d2 < len(lut)                                   # (FAR is above every n)
    return np.where(inside, np.asarray(lut, np.uint16)[np.where(inside, d2, 0)], 0).astype(np.uint16)


def points(xyz, kind, levels=None):
    """xyz float32 [n][W][3], kind uint32 [n][W], levels None or [n][3][3]: a list of float64 [k][2], the HIT beams whose
    levelled x and y are finite, in beam order."""
    out = []
    for s in range(len(xyz)):
        l = np.eye(3) if levels is None else np.asarray(levels[s], np.float64).reshape(3, 3)
        x, y, z = (xyz[s][:, k].astype(np.float64) for k in range(3))
        with np.errstate(all="ignore"):
            px = (l[0, 0] * x + l[0, 1] * y) + l[0, 2] * z
            py = (l[1, 0] * x + l[1, 1] * y) + l[1, 2] * z
        keep = (np.asarray(kind[s]) == HIT) & np.isfinite(px) & np.isfinite(py)
        out.append(np.stack([px[keep], py[keep]], axis=1))
    return out


def cells(pts, tx, ty, c, s, geom):
    """(ex, ey int64, ok): the cells of the points under candidate (tx, ty, c, s); ok False where OUTSIDE by the size rule"""
    inv_res = 1.0 / geom["resolution"]
    px, py = pts[:, 0], pts[:, 1]
    with np.errstate(all="ignore"):
        wx = (c * px - s * py) + tx
        wy = (s * px + c * py) + ty
        ex = np.floor((wx - geom["origin_x"]) * inv_res)
        ey = np.floor((wy - geom["origin_y"]) * inv_res)
        ok = (np.abs(ex) < LIMIT) & (np.abs(ey) < LIMIT)      # (a NaN compares False)
    return np.where(ok, ex, 0).astype(np.int64), np.where(ok, ey, 0).astype(np.int64), ok


def _in_grid(x, y, geom):
    return (x >= 0) & (x < geom["width"]) & (y >= 0) & (y < geom["height"])


def score(S, pts, candidates, geom):
    """(score, inside) uint32 [P] of candidates float64 [P][4] = (tx, ty, c, s)"""
    candidates = np.asarray(candidates, np.float64).reshape(-1, 4)
    sc, ins = np.zeros(len(candidates), np.uint32), np.zeros(len(candidates), np.uint32)
    for p, (tx, ty, c, s) in enumerate(candidates):
        ex, ey, ok = cells(pts, tx, ty, c, s, geom)
        ok = ok & _in_grid(ex, ey, geom)
        sc[p] = int(S[ey[ok], ex[ok]].astype(np.uint64).sum())
        ins[p] = int(ok.sum())
    return sc, ins


def search_config(**fields):
    cfg = dict(half_x=10, half_y=10, step_cells=1, half_theta=0, theta_step=0.0)
    cfg.update(fields)
    return cfg


def search_size(cfg):
    return 2 * cfg["half_x"] + 1, 2 * cfg["half_y"] + 1, 2 * cfg["half_theta"] + 1


def angle(yaw0, half_theta, theta_step, j):
    return float(yaw0) if half_theta == 0 else float(yaw0) + float(j - half_theta) * float(theta_step)


def rotations(yaw0, half_theta, theta_step):
    return np.array([[math.cos(angle(yaw0, half_theta, theta_step, j)), math.sin(angle(yaw0, half_theta, theta_step, j))]
                     for j in range(2 * half_theta + 1)])


def search(S, pts_list, centres, cfg, geom):
    """best uint32 [n][4] = (score, index, inside, n_points), slice_best uint32 [n][T][2], volume uint32 [n][T][Ny][Nx]"""
    Nx, Ny, T = search_size(cfg)
    H, W = S.shape
    pad = np.zeros((H + 2, W + 2), np.uint64)
    pad[1:-1, 1:-1] = S
    dx = (np.arange(Nx) - cfg["half_x"]) * cfg["step_cells"]
    dy = (np.arange(Ny) - cfg["half_y"]) * cfg["step_cells"]
    n = len(pts_list)
    best, sl, vol = np.zeros((n, 4), np.uint32), np.zeros((n, T, 2), np.uint32), np.zeros((n, T, Ny, Nx), np.uint32)
    for k, (pts, (x0, y0, yaw0)) in enumerate(zip(pts_list, np.asarray(centres, np.float64).reshape(-1, 3))):
        cs = rotations(yaw0, cfg["half_theta"], cfg["theta_step"])
        kept = []
        for j in range(T):
            bx, by, ok = cells(pts, x0, y0, cs[j, 0], cs[j, 1], geom)
            bx, by = bx[ok], by[ok]
            kept.append((bx, by))
            v = np.zeros((Ny, Nx), np.uint64)
            for a in range(0, len(bx), 64):
                xs = np.clip(bx[a:a + 64, None] + dx[None, :], -1, W) + 1
                ys = np.clip(by[a:a + 64, None] + dy[None, :], -1, H) + 1
                v += pad[ys[:, :, None], xs[:, None, :]].sum(axis=0)
            vol[k, j] = v
            at = int(np.argmax(v))                          # (the first of equal maxima: the lowest index)
            sl[k, j] = (int(v.reshape(-1)[at]), j * Ny * Nx + at)
        jb = int(np.argmax(sl[k, :, 0]))
        index = int(sl[k, jb, 1])
        ix, iy = index % Nx, (index // Nx) % Ny
        bx, by = kept[jb]
        inside = int(_in_grid(bx + dx[ix], by + dy[iy], geom).sum())
        best[k] = (int(sl[k, jb, 0]), index, inside, len(pts))
    return best, sl, vol


def candidate(cfg, resolution, centre, index):
    Nx, Ny, T = search_size(cfg)
    ix, iy, j = index % Nx, (index // Nx) % Ny, index // (Nx * Ny)
    res = float(f32(resolution))
    return np.array([centre[0] + float((ix - cfg["half_x"]) * cfg["step_cells"]) * res, centre[1] + float((iy - cfg["half_y"]) * cfg["step_cells"]) * res,
                     angle(centre[2], cfg["half_theta"], cfg["theta_step"], j)])


def pose3(pose2, level=None, z=0.0):
    l = np.eye(3) if level is None else np.asarray(level, np.float64).reshape(3, 3)
    c, s = math.cos(pose2[2]), math.sin(pose2[2])
    rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    out = np.zeros((3, 4))
    for r in range(3):
        for k in range(3):
            out[r, k] = (rz[r, 0] * l[0, k] + rz[r, 1] * l[1, k]) + rz[r, 2] * l[2, k]
    out[:, 3] = (pose2[0], pose2[1], z)
    return out


# --- the brute force the restatement is held to (tests/test_grid_match_expect.py): plain loops, one cell at a time -------------
def brute_search(S, pts, centre, cfg, geom):
    """the volume [T][Ny][Nx] as Python ints, and the best (score, index) under the tie rule"""
    Nx, Ny, T = search_size(cfg)
    inv_res = 1.0 / geom["resolution"]
    vol = [[[0] * Nx for _ in range(Ny)] for _ in range(T)]
    best = (-1, 0)
    for j in range(T):
        a = angle(centre[2], cfg["half_theta"], cfg["theta_step"], j)
        c, s = math.cos(a), math.sin(a)
        base = []
        for px, py in pts:
            ex = math.floor(((c * px - s * py) + centre[0] - geom["origin_x"]) * inv_res) if math.isfinite((c * px - s * py) + centre[0]) else None
            ey = math.floor(((s * px + c * py) + centre[1] - geom["origin_y"]) * inv_res) if math.isfinite((s * px + c * py) + centre[1]) else None
            if ex is not None and ey is not None and abs(ex) < LIMIT and abs(ey) < LIMIT:
                base.append((ex, ey))
        for iy in range(Ny):
            for ix in range(Nx):
                total = 0
                for bx, by in base:
                    x, y = bx + (ix - cfg["half_x"]) * cfg["step_cells"], by + (iy - cfg["half_y"]) * cfg["step_cells"]
                    if 0 <= x < geom["width"] and 0 <= y < geom["height"]:
                        total += int(S[y, x])
                vol[j][iy][ix] = total
                if total > best[0]:
                    best = (total, (j * Ny + iy) * Nx + ix)
    return vol, best
