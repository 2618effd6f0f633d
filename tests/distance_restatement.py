"""The distance section of include/lfx.h restated in numpy, from the header alone: the classes of a grid, the squared distance
of every cell to the nearest obstacle cell (brute force, and the separable form for grids too large for it), metres, the
cost table and the costmap.  Integer arithmetic in int64 up to `metres`; nothing here shares code with the library."""
import numpy as np

FAR = 0xFFFFFFFF
FREE, UNKNOWN, OBSTACLE = 0, 1, 2
MAX_COST_CELLS = 1024


def config(**fields):
    cfg = dict(occupied_percent=65, unknown_is_obstacle=0, max_cells=0, inside=0, reserved=0)
    assert set(fields) <= set(cfg), fields
    cfg.update(fields)
    return cfg


def cost_config(**fields):
    cfg = dict(inscribed_radius=0.22, inflation_radius=0.55, cost_scaling_factor=10.0, track_unknown=1)
    assert set(fields) <= set(cfg), fields
    cfg.update(fields)
    return cfg


def classes(G, cfg):
    """uint8 [H][W]: OBSTACLE iff G >= occupied_percent or (G < 0 and unknown_is_obstacle), else UNKNOWN iff G < 0, else FREE"""
    G = np.asarray(G, np.int8).astype(np.int64)
    obstacle = (G >= cfg["occupied_percent"]) | ((G < 0) & bool(cfg["unknown_is_obstacle"]))
    return np.where(obstacle, OBSTACLE, np.where(G < 0, UNKNOWN, FREE)).astype(np.uint8)


def _capped(best, cfg):
    """int64 minima (-1: no site) as the uint32 field: FAR without a site and above R * R"""
    R = int(cfg["max_cells"])
    far = best < 0
    if R:
        far |= best > R * R
    return np.where(far, FAR, best).astype(np.uint32)


def _sites(G, cfg, inside):
    obstacle = classes(G, cfg) == OBSTACLE
    return ~obstacle if inside else obstacle


def d2_brute(G, cfg, inside=False):
    """every cell against every site, int64; inside: the sites are the cells that are NOT obstacles (the field i2)"""
    sites = _sites(G, cfg, inside)
    H, W = sites.shape
    ys, xs = np.nonzero(sites)
    if len(ys) == 0:
        return np.full((H, W), FAR, np.uint32)
    best = np.full((H, W), -1, np.int64)
    cy, cx = np.mgrid[0:H, 0:W].astype(np.int64)
    for at in range(0, len(ys), 256):
        d = (cy[..., None] - ys[at:at + 256]) ** 2 + (cx[..., None] - xs[at:at + 256]) ** 2
        m = d.min(axis=-1)
        best = np.where(best < 0, m, np.minimum(best, m))
    return _capped(best, cfg)


def d2_separable(G, cfg, inside=False):
    """column distances, then per row a W x W minimum"""
    sites = _sites(G, cfg, inside)
    H, W = sites.shape
    none = np.int64(1) << 40
    g = np.full((H, W), none, np.int64)
    last = np.full(W, -1, np.int64)
    for y in range(H):                                    # the nearest site at or below
        last = np.where(sites[y], y, last)
        g[y] = np.where(last >= 0, y - last, none)
    nxt = np.full(W, -1, np.int64)
    for y in range(H - 1, -1, -1):                        # ... at or above
        nxt = np.where(sites[y], y, nxt)
        g[y] = np.minimum(g[y], np.where(nxt >= 0, nxt - y, none))
    x = np.arange(W, dtype=np.int64)
    dx2 = (x[:, None] - x[None, :]) ** 2                  # [x][x']
    best = np.empty((H, W), np.int64)
    for y in range(H):
        col2 = np.where(g[y] >= none, none, g[y] * g[y])
        best[y] = (dx2 + col2[None, :]).min(axis=1)
    best = np.where(best >= none, -1, best)
    return _capped(best, cfg)


def stats(G, cfg, d2):
    cl = classes(G, cfg)
    near = d2[d2 != FAR]
    return dict(n_obstacle=int((cl == OBSTACLE).sum()), n_unknown=int((cl == UNKNOWN).sum()), n_far=int((d2 == FAR).sum()),
                max_d2=int(near.max()) if near.size else 0)


def metres(cl, d2, i2, resolution):
    """float32 [H][W]; i2: None without `inside`"""
    res = np.float64(np.float32(resolution))
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.where(d2 == FAR, np.float32(np.inf), (np.sqrt(d2.astype(np.float64)) * res).astype(np.float32)).astype(np.float32)
        if i2 is None:
            inner = np.zeros(d2.shape, np.float32)
        else:
            inner = np.where(i2 == FAR, np.float32(-np.inf), -((np.sqrt(i2.astype(np.float64)) * res).astype(np.float32))).astype(np.float32)
    return np.where(cl == OBSTACLE, inner, out).astype(np.float32)


def cost_cells(cfg, resolution):
    """Rc = ceil((double)inflation_radius / (double)resolution)"""
    return int(np.ceil(np.float64(np.float32(cfg["inflation_radius"])) / np.float64(np.float32(resolution))))


def cost_table(cfg, resolution, with_exact=False):
    """uint8 [Rc * Rc + 1]; with_exact: also the float64 values 252 exp(...) before truncation (nan where no exp is taken)"""
    res = np.float64(np.float32(resolution))
    inscribed, inflation = np.float64(np.float32(cfg["inscribed_radius"])), np.float64(np.float32(cfg["inflation_radius"]))
    scaling = np.float64(np.float32(cfg["cost_scaling_factor"]))
    Rc = cost_cells(cfg, resolution)
    assert Rc <= MAX_COST_CELLS
    k = np.arange(Rc * Rc + 1, dtype=np.float64)
    d = np.sqrt(k) * res
    raw = 252.0 * np.exp(-scaling * (d - inscribed))
    decays = ~(d <= inscribed) & ~(d > inflation)
    lut = np.where(d <= inscribed, 253, np.where(d > inflation, 0, np.where(decays, raw, 0.0).astype(np.uint8))).astype(np.uint8)
    lut[0] = 254
    if with_exact:
        exact = np.where(decays, raw, np.nan)
        exact[0] = np.nan
        return lut, exact
    return lut


def costmap(cl, d2, lut, cfg):
    """uint8 [H][W] given the table (its length is Rc * Rc + 1)"""
    rc2 = len(lut) - 1
    inflated = (d2 != FAR) & (d2.astype(np.int64) <= rc2)
    cost = np.where(inflated, lut[np.where(inflated, d2, 0).astype(np.int64)], 0).astype(np.uint8)
    cost = np.where((cl == UNKNOWN) & bool(cfg["track_unknown"]), 255, cost)
    return np.where(cl == OBSTACLE, 254, cost).astype(np.uint8)
