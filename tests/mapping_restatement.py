"""Test-side restatement of the reference's mapping node (no GPU): PoseDiffIsSufficientlySmall (map.hpp:49-60) in the
operation order include/lfx.h states for lfx_pose_diff, MapBuilder::Callback (map.hpp:104-133) over it, and Eigen's
Quaterniond::toRotationMatrix for building the reference's test poses.  tests/test_mapping_reference.py pins it with the
reference's own vectors (tests/golden/mapping_vectors.json); tests/test_mapping_gpu.py holds the device mapper to it."""
import math

import numpy as np

from tests.odometry_restatement import transform

ADDED, EMPTY, TOO_CLOSE = 0, 1, 2


def quaternion_matrix(w, x, y, z, normalize=True):
    """Eigen's Quaterniond(w, x, y, z)[.normalized()].toRotationMatrix()."""
    if normalize:
        n = math.sqrt(((w * w + x * x) + y * y) + z * z)
        w, x, y, z = w / n, x / n, y / n, z / n
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]], np.float64)


def pose(R, t):
    return np.ascontiguousarray(np.hstack([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)]))


def pose_diff(pose0, pose1):
    """(|d.translation()|, |Quaterniond(d.rotation()).vec()|), d = pose0^-1 pose1, in lfx.h's order (Python floats are
    IEEE doubles and nothing is fused)."""
    a = [float(v) for v in np.asarray(pose0, np.float64).reshape(12)]
    b = [float(v) for v in np.asarray(pose1, np.float64).reshape(12)]

    def R0(r, c):
        return a[4 * r + c]

    def R1(r, c):
        return b[4 * r + c]

    m = [[0.0] * 3 for _ in range(3)]
    t = [0.0] * 3
    for r in range(3):
        inv_t = -((R0(0, r) * a[3] + R0(1, r) * a[7]) + R0(2, r) * a[11])
        t[r] = ((R0(0, r) * b[3] + R0(1, r) * b[7]) + R0(2, r) * b[11]) + inv_t
        for c in range(3):
            m[r][c] = (R0(0, r) * R1(0, c) + R0(1, r) * R1(1, c)) + R0(2, r) * R1(2, c)
    translation = math.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    q = [0.0] * 3
    tr = (m[0][0] + m[1][1]) + m[2][2]
    if tr > 0.0:
        s = 0.5 / math.sqrt(tr + 1.0)
        q = [(m[2][1] - m[1][2]) * s, (m[0][2] - m[2][0]) * s, (m[1][0] - m[0][1]) * s]
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        s0 = math.sqrt(((m[i][i] - m[j][j]) - m[k][k]) + 1.0)
        q[i] = 0.5 * s0
        s = 0.5 / s0
        q[j] = (m[j][i] + m[i][j]) * s
        q[k] = (m[k][i] + m[i][k]) * s
    return translation, math.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])


def small(pose0, pose1, translation_threshold, rotation_threshold):
    t, r = pose_diff(pose0, pose1)
    return t < translation_threshold and r < rotation_threshold


class MapBuilder:
    """MapBuilder<PointType>::Callback over records of 4 floats; the map as a list of transformed clouds."""

    def __init__(self, translation_threshold=1.0, rotation_threshold=0.1):
        self.tt, self.rt = translation_threshold, rotation_threshold
        self.clouds, self.n_points, self.prev = [], 0, None
        self.counts = dict(added=0, empty=0, too_close=0)

    def callback(self, cloud, pose_):
        cloud = np.asarray(cloud, np.float32).reshape(-1, 4)
        if len(cloud) == 0:
            self.counts["empty"] += 1
            return EMPTY
        if self.n_points > 0 and small(self.prev, pose_, self.tt, self.rt):
            self.counts["too_close"] += 1
            return TOO_CLOSE
        self.clouds.append(transform(pose_, cloud))
        self.n_points += len(cloud)
        self.prev = np.asarray(pose_, np.float64).reshape(3, 4).copy()
        self.counts["added"] += 1
        return ADDED

    def map(self):
        return np.concatenate(self.clouds) if self.clouds else np.zeros((0, 4), np.float32)
