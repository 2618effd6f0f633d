#!/usr/bin/env python3
"""An independent reference for the pose graph's residual r = (Log(R_E), t_E) (include/lfx.h, the pose graph section),
computed with mpmath at 50 digits and written to tests/golden/pose_graph_residual_reference.json.

The inputs are doubles: T_i, T_j, Z ([3][4] each), made here from integers (a small linear congruential generator: no
library's random stream is involved, so that the file can be written again bit for bit) so that the residual rotation has
a chosen angle about a random axis and the residual translation is of the order of a metre.  From those doubles, exactly:
  R_E = R_Z^T R_i^T R_j,  t_E = R_Z^T (R_i^T (t_j - t_i) - t_Z)
Log(R_E) does NOT go the header's way (the antisymmetric part and the trace).  The three matrices are rotations rounded to
doubles, so R_E is a rotation to about 1e-16: it is first brought to the nearest rotation (the polar factor, Newton's
iteration X <- (X + X^-T) / 2 to 50 digits), that rotation's unit quaternion is taken by the largest-component rule, and
phi = 2 atan2(|q_v|, q_w) q_v / |q_v|.  Every result is rounded once, to the nearest double, and written as a hex float.

    python tools/pose_graph_reference.py            writes the file
    python tools/pose_graph_reference.py --check    compares the file with what would be written"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "pose_graph_residual_reference.json")
ANGLES = ("0", "1e-12", "1e-7", "9.9e-5", "1.01e-4", "1e-2", "1.0", "2.5", "2.9", "2.99")
DIGITS = 50


class Lcg:
    """integers only: x <- (a x + c) mod 2^32; a value is the top 20 bits as a fraction in [-1, 1)"""

    def __init__(self, seed):
        self.x = seed & 0xFFFFFFFF

    def unit(self):
        self.x = (1664525 * self.x + 1013904223) & 0xFFFFFFFF
        return ((self.x >> 12) - (1 << 19)) / float(1 << 19)

    def vector(self, scale=1.0):
        return [scale * self.unit() for _ in range(3)]


def _mp():
    import mpmath
    mpmath.mp.dps = DIGITS
    return mpmath


def exp_rotation(mp, a):
    """Rodrigues' formula at 50 digits (the series where the angle is below 1e-20: exact at this precision)"""
    a = [mp.mpf(x) for x in a]
    th = mp.sqrt(a[0] ** 2 + a[1] ** 2 + a[2] ** 2)
    ax = mp.matrix([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    A = 1 - th ** 2 / 6 if th < mp.mpf("1e-20") else mp.sin(th) / th
    B = mp.mpf(1) / 2 - th ** 2 / 24 if th < mp.mpf("1e-20") else (1 - mp.cos(th)) / th ** 2
    return mp.eye(3) + A * ax + B * (ax * ax)


def rounded(m):
    """a matrix of mpf rounded to doubles (a list of rows)"""
    return [[float(m[r, c]) for c in range(m.cols)] for r in range(m.rows)]


def nearest_rotation(mp, M):
    X = M.copy()
    for _ in range(60):
        Y = (X + mp.inverse(X).T) / 2
        done = mp.norm(Y - X, 1) < mp.mpf(10) ** (-(DIGITS - 5))
        X = Y
        if done:
            break
    return X


def log_by_quaternion(mp, Q):
    """Log of the rotation Q through its unit quaternion (w, x, y, z), the largest component first (Shepperd)"""
    t = Q[0, 0] + Q[1, 1] + Q[2, 2]
    cand = [t, Q[0, 0] - Q[1, 1] - Q[2, 2], Q[1, 1] - Q[0, 0] - Q[2, 2], Q[2, 2] - Q[0, 0] - Q[1, 1]]
    k = max(range(4), key=lambda i: cand[i])
    s = 2 * mp.sqrt(1 + cand[k])
    if k == 0:
        w, x, y, z = s / 4, (Q[2, 1] - Q[1, 2]) / s, (Q[0, 2] - Q[2, 0]) / s, (Q[1, 0] - Q[0, 1]) / s
    elif k == 1:
        w, x, y, z = (Q[2, 1] - Q[1, 2]) / s, s / 4, (Q[0, 1] + Q[1, 0]) / s, (Q[0, 2] + Q[2, 0]) / s
    elif k == 2:
        w, x, y, z = (Q[0, 2] - Q[2, 0]) / s, (Q[0, 1] + Q[1, 0]) / s, s / 4, (Q[1, 2] + Q[2, 1]) / s
    else:
        w, x, y, z = (Q[1, 0] - Q[0, 1]) / s, (Q[0, 2] + Q[2, 0]) / s, (Q[1, 2] + Q[2, 1]) / s, s / 4
    if w < 0:
        w, x, y, z = -w, -x, -y, -z
    n = mp.sqrt(x ** 2 + y ** 2 + z ** 2)
    if n == 0:
        return [mp.mpf(0)] * 3
    theta = 2 * mp.atan2(n, w)
    return [theta * v / n for v in (x, y, z)]


def residual(mp, Ti, Tj, Z):
    """r = (phi, t_E) at 50 digits from the doubles Ti, Tj, Z ([3][4] lists)"""
    def split(T):
        return mp.matrix([[mp.mpf(T[r][c]) for c in range(3)] for r in range(3)]), mp.matrix([mp.mpf(T[r][3]) for r in range(3)])
    (Ri, ti), (Rj, tj), (Rz, tz) = split(Ti), split(Tj), split(Z)
    RE = Rz.T * Ri.T * Rj
    tE = Rz.T * (Ri.T * (tj - ti) - tz)
    return log_by_quaternion(mp, nearest_rotation(mp, RE)) + [tE[k] for k in range(3)]


def cases(mp):
    out = []
    for n, text in enumerate(ANGLES):
        rng = Lcg(2024 + 17 * n)
        poses = []
        for _ in range(2):
            R = rounded(exp_rotation(mp, rng.vector(2.0)))
            t = rng.vector(5.0)
            poses.append([R[r] + [t[r]] for r in range(3)])
        Ti, Tj = poses
        axis = rng.vector()
        norm = mp.sqrt(sum(mp.mpf(v) ** 2 for v in axis))
        rot = exp_rotation(mp, [mp.mpf(text) * mp.mpf(v) / norm for v in axis])
        # Z = T_i^-1 T_j from the doubles, its rotation turned back by the chosen residual, its translation a metre off
        Ri = mp.matrix([[mp.mpf(Ti[r][c]) for c in range(3)] for r in range(3)])
        Rj = mp.matrix([[mp.mpf(Tj[r][c]) for c in range(3)] for r in range(3)])
        dt = mp.matrix([mp.mpf(Tj[r][3]) - mp.mpf(Ti[r][3]) for r in range(3)])
        Rz = rounded(Ri.T * Rj * rot.T)
        tz = rounded(Ri.T * dt)
        off = rng.vector()
        Z = [Rz[r] + [tz[r][0] + off[r]] for r in range(3)]
        r = residual(mp, Ti, Tj, Z)
        out.append(dict(angle=text, Ti=[float.hex(v) for row in Ti for v in row], Tj=[float.hex(v) for row in Tj for v in row],
                        Z=[float.hex(v) for row in Z for v in row], r=[float.hex(float(v)) for v in r]))
    return out


def text():
    """the file's contents"""
    doc = dict(about="tools/pose_graph_reference.py: r = (Log(R_E), t_E) at %d digits, rounded once; hex floats, [3][4] row-major" % DIGITS,
               cases=cases(_mp()))
    return json.dumps(doc, indent=1) + "\n"


def main(argv):
    if "--check" in argv:
        with open(PATH) as f:
            same = f.read() == text()
        print("the file is what this tool writes" if same else "the file differs from what this tool writes")
        return 0 if same else 1
    with open(PATH, "w") as f:
        f.write(text())
    print("wrote", PATH)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
