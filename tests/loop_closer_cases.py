"""What the loop closer's tests share: hand cases of the gate, and THE DRIVE -- twelve keyframes of 16 x 900.  Nodes 0-5 are
the six keyframes of tests/scan_context_restatement.py, nodes 6-11 one revisit of each place, each with a different one of
its yaws.  The true poses come from KEYFRAME_PLACES, REVISIT_OFFSET and the yaws; the chain edges are measured from the
truth with a fixed, same-signed jitter per step (as examples/close_loop.cpp measures its odometry, without the noise), so
the chained poses drift.  search_radius is below the least spacing of the places (2.5 m), so the drifted poses decide which
entries are eligible."""
import numpy as np

from lidar_feature_extraction_amd import motion_between
from tests import scan_context_restatement as SC

N = 12
MIN_GAP, SEARCH_RADIUS, MAX_DISTANCE, N_CANDIDATES = 6, 2.0, 1.0, 3
REVISIT_YAW = [i % 4 for i in range(6)]                                 # node 6 + i: the revisit of place i turned by its yaw i % 4
# the jitter of every chain step: a motion multiplied onto the true step from the right
JITTER_YAW, JITTER_T = 0.002, (0.08, 0.06, 0.0)
SIGMA_ROT, SIGMA_T = 0.005, 0.1                                          # the chain edges' information: diag(1 / sigma^2)
SUBMAP = dict(submap_half_window=2, submap_radius=5.0)

_MADE = {}


def planar(yaw, x, y, z=0.0):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0.0, x], [s, c, 0.0, y], [0.0, 0.0, 1.0, z]], np.float64)


def product(a, b):
    """a b, both [R | t]: every sum of three terms is (a0 b0 + a1 b1) + a2 b2, as examples/close_loop.cpp has it"""
    a, b = np.asarray(a, np.float64).reshape(3, 4), np.asarray(b, np.float64).reshape(3, 4)
    out = np.zeros((3, 4))
    for r in range(3):
        for c in range(4):
            out[r, c] = (a[r, 0] * b[0, c] + a[r, 1] * b[1, c]) + a[r, 2] * b[2, c]
        out[r, 3] += a[r, 3]
    return out


def clouds():
    """The twelve scans."""
    rev = SC.revisits()
    return list(SC.keyframes()) + [rev[4 * i + REVISIT_YAW[i]][0] for i in range(6)]


def truth():
    """[12][3][4]: the sensor's true poses"""
    rev = SC.revisits()
    out = [planar(0.0, x, y) for x, y in SC.KEYFRAME_PLACES]
    for i, (x, y) in enumerate(SC.KEYFRAME_PLACES):
        out.append(planar(rev[4 * i + REVISIT_YAW[i]][2], x + SC.REVISIT_OFFSET[0], y + SC.REVISIT_OFFSET[1]))
    return np.stack(out)


def true_place(q):
    """(place, yaw) node q >= 6 revisits"""
    return q - 6, SC.revisits()[4 * (q - 6) + REVISIT_YAW[q - 6]][2]


def chain():
    """(edges, chained): the eleven chain edges as (i, j, z [3][4], information [6][6]) and the poses chained from them,
    node 0 at its true pose."""
    if "chain" not in _MADE:
        t = truth()
        jitter = planar(JITTER_YAW, *JITTER_T)
        info = np.diag([1.0 / SIGMA_ROT ** 2] * 3 + [1.0 / SIGMA_T ** 2] * 3)
        edges, chained = [], [t[0].copy()]
        for k in range(N - 1):
            z = product(np.asarray(motion_between(t[k], t[k + 1])).reshape(3, 4), jitter)
            edges.append((k, k + 1, z, info))
            chained.append(product(chained[-1], z))
        _MADE["chain"] = (edges, np.stack(chained))
    return _MADE["chain"]


def worst_error(poses, nodes=range(6, 12)):
    """the worst position error of `nodes` against the truth"""
    p, t = np.asarray(poses, np.float64).reshape(-1, 3, 4), truth()
    return max(float(np.linalg.norm(p[k][:, 3] - t[k][:, 3])) for k in nodes)


# --- hand cases of the gate: (translations of the entries then of the query, radius, the eligible entries) -------------------
GATE_CASES = [
    ([(3, 4, 0), (0, 3, 4), (0, 0, 0)], 5.0, [0, 1]),                   # 9 + 16 = 25 exactly: in
    ([(3, 4, 0), (0, 3, 4), (0, 0, 0)], float(np.nextafter(5.0, 0.0)), []),
    ([(3, 4, 0), (0, 3, 4), (1e300, 0, 0), (0, 0, 0)], float("inf"), [0, 1, 2]),
    ([(1, 0, 0), (np.nan, 0, 0), (0, 0, 0)], float("inf"), [0]),        # a pose that is not finite is never eligible
    ([(0, 0, 0), (0, 0, 0)], 0.0, [0]),
]
