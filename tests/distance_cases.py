"""The grids the distance tests share (tests/test_distance_expect.py on the restatement, tests/test_distance_gpu.py on the
device), as functions of a seed, and the expected fields of each -- computed once and handed out unchanged.

What the shapes are built around (csrc/lfx_kernels_distance.hpp): the column pass works on y-segments of SEG_ROWS rows and
tiles of TILE columns; the row pass is the outward search for caps of 1 .. SEARCH_MAX cells and otherwise the envelope kernel,
whose workgroup of 64, 256 or 1024 threads owns SITES columns per thread -- rows of up to 1024, up to 4096 and wider ones."""
import numpy as np

from tests import distance_restatement as D

SEG_ROWS, TILE, SITES, SEARCH_MAX = 64, 256, 16, 64
ENVELOPE_WIDTHS = (64 * SITES, 256 * SITES)               # 1024, 4096: the widest row of the 64- and of the 256-thread form
FREE_V, OCC_V, UNK_V = 0, 100, -1
_EXPECTED = {}


def grid(h, w, fill=FREE_V):
    return np.full((h, w), fill, np.int8)


def with_obstacles(h, w, cells, fill=FREE_V):
    g = grid(h, w, fill)
    for x, y in cells:
        g[y, x] = OCC_V
    return g


def random_grid(h, w, density, unknown=0.3, seed=0):
    """obstacles (65 .. 100) at `density`, `unknown` of the rest -1, the others 0 .. 64"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 65, (h, w)).astype(np.int8)
    g[rng.uniform(0, 1, (h, w)) < unknown] = UNK_V
    occ = rng.uniform(0, 1, (h, w)) < density
    g[occ] = rng.integers(65, 101, (h, w)).astype(np.int8)[occ]
    return g


def smallest(seed=0):
    """(name, grid, config fields)"""
    out = []
    for name, v in (("obstacle", OCC_V), ("free", FREE_V), ("unknown", UNK_V)):
        out.append(("1x1_" + name, grid(1, 1, v), {}))
    out.append(("1x7", with_obstacles(1, 7, [(2, 0)]), {}))
    out.append(("7x1", with_obstacles(7, 1, [(0, 5)]), {}))
    out.append(("2x2", with_obstacles(2, 2, [(1, 0)]), {}))
    out.append(("no_obstacle", random_grid(9, 11, 0.0, seed=seed), {}))
    out.append(("all_obstacles", grid(9, 11, OCC_V), {}))
    out.append(("all_unknown_as_obstacles", grid(5, 6, UNK_V), dict(unknown_is_obstacle=1)))
    out.append(("all_unknown", grid(5, 6, UNK_V), dict(unknown_is_obstacle=0)))
    g = grid(6, 7, 10)
    g[2, 3] = 40
    g[4, 1] = 41
    out.append(("percent_at_the_value", g, dict(occupied_percent=40)))
    out.append(("percent_one_above", g, dict(occupied_percent=41)))
    out.append(("percent_two_above", g, dict(occupied_percent=42)))
    return out


def capped(seed=0):
    """one obstacle at (0, 0) of 9 x 9 under the caps; SEARCH_MAX and one more: either side of the two row kernels"""
    g = with_obstacles(9, 9, [(0, 0)])
    return [("cap_%d" % r, g, dict(max_cells=r)) for r in (5, 1, 32767, 0, SEARCH_MAX, SEARCH_MAX + 1)]


def breakers(seed=0):
    """65 wide, 63 high"""
    w, h = 65, 63
    out = [("staircase", with_obstacles(h, w, [(k, k) for k in range(0, 63, 1)]), {}),
           ("staircase_steep", with_obstacles(h, w, [(k // 3, k) for k in range(63)]), {})]
    cb = grid(h, w)
    cb[(np.add.outer(np.arange(h), np.arange(w)) % 2) == 0] = OCC_V
    out.append(("checkerboard", cb, {}))
    out.append(("equidistant_pair", with_obstacles(h, w, [(10, 31), (54, 31)]), {}))
    out.append(("equidistant_pair_vertical", with_obstacles(h, w, [(32, 3), (32, 59)]), {}))
    row = grid(h, w)
    row[17, :] = OCC_V
    out.append(("obstacle_row", row, {}))
    col = grid(h, w)
    col[:, 40] = OCC_V
    out.append(("obstacle_column", col, {}))
    for k, density in enumerate((0.001, 0.05, 0.5)):
        out.append(("random_%g" % density, random_grid(h, w, density, seed=seed + 10 + k), {}))
        out.append(("random_%g_cap7" % density, random_grid(h, w, density, seed=seed + 20 + k), dict(max_cells=7)))
    return out


SHAPE_WIDTHS = (63, 64, 65, 255, 256, 257, 1023, 1025)
SHAPE_HEIGHTS = (1, 2, 67)
TRANSPOSED = ((63, 67), (257, 67), (1023, 67))            # (width, height) whose transposes run too
# ... and around the tiles: a y-segment, the envelope kernel's widest rows
EXTRA_SHAPES = ((5, SEG_ROWS - 1), (5, SEG_ROWS), (5, SEG_ROWS + 1), (3, 2 * SEG_ROWS + 1), (ENVELOPE_WIDTHS[0], 3), (ENVELOPE_WIDTHS[1] - 1, 2),
                (ENVELOPE_WIDTHS[1], 2), (ENVELOPE_WIDTHS[1] + 1, 2))


def shapes():
    out = [(w, h) for w in SHAPE_WIDTHS for h in SHAPE_HEIGHTS]
    out += [(h, w) for w, h in TRANSPOSED]
    return out + list(EXTRA_SHAPES)


def shape_grid(w, h, seed=0):
    """a few obstacles, placed by the seed, the first and the last cell among them in turn; 30 % unknown"""
    rng = np.random.default_rng(seed + 7 * w + h)
    g = random_grid(h, w, 0.0, seed=seed + w + 3 * h)
    n = max(1, (w * h) // 3000)
    g.reshape(-1)[rng.integers(0, w * h, n)] = OCC_V
    g[(h - 1) * ((w + h) % 2), (w - 1) * (w % 2)] = OCC_V
    return g


def largest():
    """(name, grid, fields): one obstacle at one end, uncapped and capped at 100"""
    out = []
    for w, h in ((16384, 2), (2, 16384)):
        g = with_obstacles(h, w, [(0, 0)])
        for r in (0, 100):
            out.append(("%dx%d_cap%d" % (w, h, r), g, dict(max_cells=r)))
    return out


def expected(name, G, fields, inside=False):
    """(classes, d2, i2 or None, stats) of a case, from the restatement: brute force where the case is small enough for it,
    the separable form otherwise.  Computed once per name."""
    key = (name, bool(inside), G.shape, hash(G.tobytes()), tuple(sorted(fields.items())))
    if key not in _EXPECTED:
        cfg = D.config(**dict(fields, inside=int(inside)))
        cl = D.classes(G, cfg)
        h, w = G.shape

        def field(inv):
            n_sites = int((cl != D.OBSTACLE).sum() if inv else (cl == D.OBSTACLE).sum())
            return D.d2_brute(G, cfg, inv) if n_sites * w * h <= 40_000_000 else D.d2_separable(G, cfg, inv)
        d2 = field(False)
        i2 = field(True) if inside else None
        for a in (cl, d2, i2):
            if a is not None:
                a.setflags(write=False)
        _EXPECTED[key] = (cl, d2, i2, D.stats(G, cfg, d2))
    return _EXPECTED[key]


def same_bytes(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        g, w = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
        bad = np.argwhere(g != w)
        raise AssertionError((what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))
