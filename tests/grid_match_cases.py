"""The shapes the grid-match tests share (tests/test_grid_match_expect.py on the restatement, tests/test_grid_match_gpu.py on
the device), and what each is built around in lfx_kernels_gridmatch.hpp:

  field    four cells per thread (a size that is no multiple of 4 ends in the scalar tail: 1 x 1, 67 x 5, 300 x 257) and a grid
           of at most FIELD_BLOCKS workgroups of 256 threads, beyond which a thread takes a second step (FIELD_STRIDE cells);
  scans    one workgroup of 256 threads per scan walks the beams 256 at a time, a ballot per wave of 64: 0, 1, 63, 64, 65 and
           4096 HIT beams among the others;
  score    256 candidates per workgroup (P = 1, 63, 64, 65, 1025: a lone lane, a wave's edge, five workgroups) and the scan's
           points through LDS SCORE_CHUNK at a time (a scan of 4096 points takes four rounds);
  search   a workgroup owns TILE_X x TILE_Y = 64 x 16 candidates of one heading, a thread one ix and 4 iy: Nx and Ny of 1, 3,
           63, 65 and 129 put the window's edge inside the first tile, on a wave's last lane, one past it and two tiles on;
           points whose every candidate of a tile is inside the grid take a loop without bounds checks, the others the checked
           one, points no candidate of the tile brings inside are dropped -- windows overhanging each side of the grid and a
           window wholly outside walk all three."""
import numpy as np

from tests import grid_match_restatement as G

f32 = np.float32
TILE_X, TILE_Y, SCORE_CHUNK, FIELD_BLOCKS = 64, 16, 1024, 2048
FIELD_STRIDE = FIELD_BLOCKS * 256 * 4
NONE, HIT, CLEAR = 0, 1, 2

FIELD_SIZES = [(1, 1), (67, 5), (300, 257)]                  # (width, height)
FIELD_STRIDE_SIZE = (2048, 1030)                             # ... and one beyond FIELD_STRIDE cells
HIT_COUNTS = [0, 1, 63, 64, 65, 4096]
SCORE_P = [1, 63, 64, 65, 1025]
# (half_x, half_y, half_theta, step_cells): Nx, Ny over {1, 3, 63, 65, 129}, T over {1, 3, 7}, both steps
WINDOWS = [(0, 0, 0, 1), (1, 31, 1, 1), (31, 1, 0, 3), (32, 32, 1, 1), (64, 0, 3, 1), (0, 64, 0, 3), (32, 1, 3, 3), (64, 31, 0, 1)]

# the hand field, 5 x 4 cells of 1 m from the world origin, written out: S[y][x]
HAND_S = np.array([[0, 1, 2, 3, 4],
                   [10, 11, 12, 13, 14],
                   [20, 21, 22, 23, 24],
                   [30, 31, 32, 33, 34]], np.uint16)
HAND_GEOM = G.geometry(5, 4, 1.0)
# three points seen from a sensor at the origin
HAND_POINTS = np.array([[0.5, 0.5], [1.5, 0.5], [0.5, 2.5]])


def same_bytes(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError((what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def random_grid(h, w, density, seed):
    """an int8 grid in the emit's format: obstacles (100) at `density`, a few unknown cells, the rest free"""
    rng = np.random.default_rng(seed)
    g = np.zeros((h, w), np.int8)
    r = rng.random((h, w))
    g[r < density] = 100
    g[r > 0.97] = -1
    return g


def random_field(h, w, seed, peak=1000):
    """a score field that is not one of any distance field: every cell its own value -- a wrong cell shows in the sum"""
    return np.random.default_rng(seed).integers(0, peak + 1, (h, w)).astype(np.uint16)


def beams(n, W, n_hit, seed, reach=20.0):
    """(xyz float32 [n][W][3], kind uint32 [n][W]): n_hit HIT beams at random places among NONE and CLEAR ones, which carry
    coordinates too (a CLEAR beam's end is a real point; neither may score)"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-reach, reach, (n, W, 3)).astype(f32)
    xyz[..., 2] = rng.uniform(-1.0, 1.0, (n, W)).astype(f32)
    kind = np.zeros((n, W), np.uint32)
    for s in range(n):
        others = rng.integers(0, 2, W).astype(np.uint32) * CLEAR
        kind[s] = others
        kind[s, rng.permutation(W)[:n_hit]] = HIT
        xyz[s, kind[s] == NONE] = 0.0
    return xyz, kind


def pack_beams(xyz, kind):
    """float32 [n][W][4] with the kind's bits in the fourth float: lfx_occupancy_view_t.beams"""
    out = np.zeros(xyz.shape[:2] + (4,), f32)
    out[..., :3] = xyz
    out[..., 3] = np.ascontiguousarray(kind, np.uint32).view(f32)
    return out


def yaw_levels(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for a in rng.uniform(-np.pi, np.pi, n):
        out.append([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return np.array(out)


def candidates(P, geom, seed, reach=8.0):
    """P candidates around the grid's middle, any heading"""
    rng = np.random.default_rng(seed)
    mx = geom["origin_x"] + 0.5 * geom["width"] * geom["resolution"]
    my = geom["origin_y"] + 0.5 * geom["height"] * geom["resolution"]
    a = rng.uniform(-np.pi, np.pi, P)
    return np.stack([mx + rng.uniform(-reach, reach, P), my + rng.uniform(-reach, reach, P), np.cos(a), np.sin(a)], axis=1)


def window(half_x, half_y, half_theta, step_cells, theta_step=0.013):
    return G.search_config(half_x=half_x, half_y=half_y, half_theta=half_theta, step_cells=step_cells, theta_step=theta_step if half_theta else 0.0)


def as_u32(t):
    """a device tensor of int32 holding uint32 bits, on the host as uint32"""
    return t.cpu().numpy().view(np.uint32)


# --- the end-to-end scene: a room of 40 x 24 m drawn on the hand grid of 96 x 40 cells of 1 m ----------------------------------
ROOM = (20.5, 8.5, 60.5, 32.5)                               # x0, y0, x1, y1 of its walls: through the middle of their cells
E2E_BEAMS = 16
E2E_SENSORS = [(40.8, 27.3, -2.1), (53.5, 17.7, -0.5), (50.0, 19.1, 0.3), (26.8, 24.3, 0.2)]     # x, y, yaw: no ray grazes another's wall cell
E2E_QUERY = 2                                                # the scan searched for
E2E_OFF = (3, -3, 2)                                         # the centre is so many cells, cells and heading steps off
E2E_THETA_STEP = 0.01
E2E_WINDOW = dict(half_x=5, half_y=4, half_theta=3, step_cells=1, theta_step=E2E_THETA_STEP)


def e2e_config():
    from tests import occupancy_cases as OC
    return OC.hand_config(E2E_BEAMS, 96, 40, max_range=60.0)


def e2e_scans():
    """(clouds, poses): from every sensor one record on the room's wall per beam column, seen in the sensor's frame; scans of
    2 x 16 records as the hand cases', the rest (0, 0, 0)"""
    from tests import segment_restatement as R
    clouds, poses = [], []
    x0, y0, x1, y1 = ROOM
    for sx, sy, yaw in E2E_SENSORS:
        c, s = np.cos(yaw), np.sin(yaw)
        recs = []
        for k in range(E2E_BEAMS):
            a = -np.pi + (k + 0.5) * 2.0 * np.pi / E2E_BEAMS                  # the middle of column k, in the world
            ux, uy = np.cos(a), np.sin(a)
            t = min(((x1 if ux > 0 else x0) - sx) / ux, ((y1 if uy > 0 else y0) - sy) / uy)
            wx, wy = t * ux, t * uy                                           # the wall point from the sensor, world axes
            recs.append((f32(c * wx + s * wy), f32(-s * wx + c * wy), f32(0), 0))
        recs += [(f32(0), f32(0), f32(0), k // 16) for k in range(len(recs), 32)]
        clouds.append(R.cloud_of(recs))
        poses.append(np.array([[c, -s, 0.0, sx], [s, c, 0.0, sy], [0.0, 0.0, 1.0, 0.0]]))
    return clouds, np.stack(poses)


def e2e_centre(poses):
    tx, ty = poses[E2E_QUERY][0, 3], poses[E2E_QUERY][1, 3]
    return np.array([tx + E2E_OFF[0] * 1.0, ty + E2E_OFF[1] * 1.0, E2E_OFF[2] * E2E_THETA_STEP])


def e2e_true_index():
    w = E2E_WINDOW
    Nx, Ny = 2 * w["half_x"] + 1, 2 * w["half_y"] + 1
    return ((w["half_theta"] - E2E_OFF[2]) * Ny + (w["half_y"] - E2E_OFF[1])) * Nx + (w["half_x"] - E2E_OFF[0])
