"""numpy restatement of the place recognition section of include/lfx.h: the scan-context descriptor of a cloud and the
distance of two descriptors under every column shift, operation for operation (float64, unfused, every sum in the
header's order), so that the device results can be compared bit for bit.  The tables come from the library
(lfx_scan_context_tables, host only), as the device's do.  Also the inputs the place tests share: the six keyframes and
24 revisits of the prototype."""
import numpy as np

from lidar_feature_extraction_amd import scan_context_config, scan_context_tables


def config(**fields):
    return scan_context_config(None, **fields)


def cells(cfg, x, y):
    """(keep, ring, sector) of records with float32 coordinates x, y (finite or not), by the header's counts."""
    cs, sn, r2tab = scan_context_tables(cfg)
    R, S = int(cfg.n_rings), int(cfg.n_sectors)
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        xd, yd = x.astype(np.float64), y.astype(np.float64)
        r2 = xd * xd + yd * yd
        min_r2 = np.float64(cfg.min_radius) * np.float64(cfg.min_radius)
        keep = np.isfinite(x) & np.isfinite(y) & (r2 >= min_r2) & (r2 < r2tab[R])
        ring = (r2[:, None] >= r2tab[None, 1:R]).sum(axis=1)
        cross = cs[None, :] * yd[:, None] - sn[None, :] * xd[:, None]
        ge = cross >= 0.0
        sector = np.where(y >= 0.0, S // 2 + ge[:, S // 2 + 1:].sum(axis=1), ge[:, 1:S // 2].sum(axis=1))
    return keep, ring.astype(np.int64), sector.astype(np.int64)


def descriptor(cfg, x, y, z):
    """The [R][S] float32 descriptor of one cloud."""
    R, S = int(cfg.n_rings), int(cfg.n_sectors)
    z = np.asarray(z, np.float32)
    keep, ring, sector = cells(cfg, x, y)
    keep = keep & np.isfinite(z)
    zmax = np.full(R * S, -np.inf, np.float32)
    np.maximum.at(zmax, (ring * S + sector)[keep], z[keep])
    has = np.zeros(R * S, bool)
    has[(ring * S + sector)[keep]] = True
    with np.errstate(invalid="ignore", over="ignore"):
        v = (zmax + np.float32(cfg.sensor_height)).astype(np.float32)
    return np.where(has & (v > 0), v, np.float32(0.0)).astype(np.float32).reshape(R, S)


def descriptor_of_cloud(cfg, cloud):
    return descriptor(cfg, cloud["x"], cloud["y"], cloud["z"])


def atan2_sectors(cfg, x, y):
    S = int(cfg.n_sectors)
    return np.floor((np.arctan2(np.asarray(y, np.float64), np.asarray(x, np.float64)) + np.pi) * S / (2.0 * np.pi)).astype(np.int64)


def column_norms(d):
    """[..., S] norms of descriptors [..., R, S]: the squares summed in the order i = 0 .. R-1."""
    d = np.asarray(d, np.float32).astype(np.float64)
    total = np.zeros(d.shape[:-2] + d.shape[-1:])
    for i in range(d.shape[-2]):
        total = total + d[..., i, :] * d[..., i, :]
    return np.sqrt(total)


def shift_distances(q, entries):
    """d(s) of query q [R][S] against entries [E][R][S]: float64 [E][S]."""
    q = np.asarray(q, np.float32).astype(np.float64)
    c = np.asarray(entries, np.float32).astype(np.float64)
    E, R, S = c.shape
    nq, nc = column_norms(q), column_norms(c)
    col = (np.arange(S)[None, :] + np.arange(S)[:, None]) % S           # [s][j] = (j + s) mod S
    g = np.zeros((E, S, S))
    for i in range(R):
        g = g + q[i][None, None, :] * c[:, i, :][:, col]
    ncs = nc[:, col]                                                    # [E][s][j]
    valid = (nq[None, None, :] > 0.0) & (ncs > 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        term = g / (nq[None, None, :] * ncs)
    total, count = np.zeros((E, S)), np.zeros((E, S))
    for j in range(S):
        total = np.where(valid[:, :, j], total + term[:, :, j], total)
        count = count + valid[:, :, j]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(count > 0, 1.0 - total / count, 1.0)


def yaw_of_shift(shift, S):
    step = (2.0 * np.pi) / float(S)
    return float(shift) * step if 2 * shift <= S else (float(shift) - float(S)) * step


def query(q, entries, k, first=0, count=None):
    """The k best of entries[first : first + count] for one query: [(entry or None, shift, distance, yaw)] * k."""
    entries = np.asarray(entries, np.float32)
    S = entries.shape[-1]
    count = len(entries) - first if count is None else count
    out = []
    if count:
        d = shift_distances(q, entries[first:first + count])
        shift = np.argmin(d, axis=1)                                    # (the first of equal minima)
        best = d[np.arange(count), shift]
        for e in np.lexsort((np.arange(count), best))[:k]:
            out.append((first + int(e), int(shift[e]), float(best[e]), yaw_of_shift(int(shift[e]), S)))
    while len(out) < k:
        out.append((None, 0, float("inf"), 0.0))
    return out


# --- the prototype's places --------------------------------------------------------------------------------------------
KEYFRAME_PLACES = [(-4.0, 2.0), (0.0, 0.0), (3.0, 1.5), (6.0, -2.0), (-7.0, -3.0), (5.0, 3.0)]
REVISIT_YAWS_DEG = [0.0, 37.0, -128.0, 179.0]
REVISIT_OFFSET = (0.2, -0.15)
RINGS, COLS = 16, 900

_PLACES = {}


def keyframes():
    """The six keyframe scans (16 x 900, seeds 100 ...), made once."""
    from lidar_feature_extraction_amd import make_scan
    if "key" not in _PLACES:
        _PLACES["key"] = [make_scan(RINGS, COLS, seed=100 + i, sensor_pose=(x, y, 0.0)) for i, (x, y) in enumerate(KEYFRAME_PLACES)]
    return _PLACES["key"]


def revisits():
    """The 24 revisits: [(cloud, keyframe index, yaw in radians)], seeds 900 ..., made once."""
    from lidar_feature_extraction_amd import make_scan
    if "rev" not in _PLACES:
        out = []
        for i, (x, y) in enumerate(KEYFRAME_PLACES):
            for j, deg in enumerate(REVISIT_YAWS_DEG):
                yaw = np.deg2rad(deg)
                cloud = make_scan(RINGS, COLS, seed=900 + 4 * i + j, sensor_pose=(x + REVISIT_OFFSET[0], y + REVISIT_OFFSET[1], yaw))
                out.append((cloud, i, float(yaw)))
        _PLACES["rev"] = out
    return _PLACES["rev"]


def yaw_error(a, b):
    d = (a - b + np.pi) % (2.0 * np.pi) - np.pi
    return abs(d)
