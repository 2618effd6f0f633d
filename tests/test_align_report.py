"""lfx_align_report and its entry points, the part that needs no GPU: the symbols and the record's size, the argument checks,
and lfx_align_covariance_ros against its numpy restatement, bit for bit (tests/report_restatement.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lidar_feature_extraction_amd import binding as LB
from tests.report_restatement import covariance_ros_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PD = C.POINTER(C.c_double)
NEW = ["lfx_scan_to_map_align_report", "lfx_localize_batch_report", "lfx_localize_host_report", "lfx_align_covariance_ros",
       "lfx_odometry_set_reports", "lfx_odometry_reports"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LB.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return LB.load()


def _rotation(axis_angle):
    th = np.asarray(axis_angle, np.float64)
    k = np.linalg.norm(th)
    if k == 0:
        return np.eye(3)
    u = th / k
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + np.sin(k) * K + (1 - np.cos(k)) * K @ K


def test_symbols_and_the_size_of_the_record(lib, tmp_path):
    """The new names are exported and declared, and sizeof(lfx_align_report) as a C compiler sees the header is the ctypes
    mirror's (fields in the header's order: 120 doubles, 5 + 3 words)."""
    import subprocess
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in LB.EXPORTS
    text = open(os.path.join(ROOT, "include", "lfx.h")).read()
    body = re.search(r"typedef struct lfx_align_report \{(.*?)\} lfx_align_report;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b([a-z_0-9]+)(?:\[\d+\])?\s*[,;]", body)
    assert fields == [f for f, _ in LB.AlignReport._fields_]
    assert C.sizeof(LB.AlignReport) == 992
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "lfx.h"\nint main(void) {printf("%zu\\n", sizeof(lfx_align_report)); return 0;}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)]).decode()) == C.sizeof(LB.AlignReport)


def test_covariance_ros_bits_against_numpy():
    """10 000 random rotations and random symmetric positive matrices: the library's T C T^T and the restatement's are the
    same bits (same order of operations, nothing fused)."""
    from lidar_feature_extraction_amd import covariance_ros
    rng = np.random.default_rng(2024)
    for i in range(10000):
        pose = np.hstack([_rotation(rng.normal(0, 1.5, 3)), rng.normal(0, 30, (3, 1))])
        B = rng.normal(0, 1, (6, 6)) * 10.0 ** rng.uniform(-4, 2, (6, 1))
        cov = B @ B.T
        cov = 0.5 * (cov + cov.T)
        got = covariance_ros(pose, cov)
        want = covariance_ros_np(pose, cov)
        assert got.tobytes() == want.tobytes(), i
        if i < 100:                                          # and it is the congruence it says it is
            T = np.zeros((6, 6))
            T[:3, 3:] = np.eye(3)
            T[3:, :3] = pose[:, :3]
            ref = T @ cov @ T.T
            assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


def test_covariance_ros_at_the_identity_swaps_the_blocks():
    from lidar_feature_extraction_amd import covariance_ros
    rng = np.random.default_rng(5)
    B = rng.normal(0, 1, (6, 6))
    cov = B @ B.T
    cov = 0.5 * (cov + cov.T)
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    got = covariance_ros(ident, cov)
    assert got[:3, :3].tobytes() == np.ascontiguousarray(cov[3:, 3:]).tobytes()
    assert got[3:, 3:].tobytes() == np.ascontiguousarray(cov[:3, :3]).tobytes()
    assert got[:3, 3:].tobytes() == np.ascontiguousarray(cov[3:, :3]).tobytes()
    assert got[3:, :3].tobytes() == np.ascontiguousarray(cov[:3, 3:]).tobytes()
    # a translation does not enter
    moved = np.hstack([np.eye(3), [[5.0], [-7.0], [2.0]]])
    assert covariance_ros(moved, cov).tobytes() == got.tobytes()


def test_null_pointers_are_invalid_arguments(lib):
    a, c, o = np.zeros(12), np.zeros(36), np.zeros(36)
    p = lambda x: x.ctypes.data_as(PD)   # noqa: E731
    assert lib.lfx_align_covariance_ros(None, p(c), p(o)) == -1
    assert lib.lfx_align_covariance_ros(p(a), None, p(o)) == -1
    assert lib.lfx_align_covariance_ros(p(a), p(c), None) == -1
    assert lib.lfx_align_covariance_ros(p(a), p(c), p(o)) == 0
    n = C.c_uint32(7)
    rep = (LB.AlignReport * 1)()
    assert lib.lfx_odometry_set_reports(None, 1) == -1
    assert lib.lfx_odometry_reports(None, rep, 1, C.byref(n)) == -1
    # the report calls without a context, and (context or not) without a place for the reports: refused before any device work
    res = (LB.AlignResult * 1)()
    pose = np.zeros(12)
    assert lib.lfx_localize_batch_report(None, None, None, 15, 20, 1.0, 1, p(pose), res, rep, None) == -1
    assert lib.lfx_localize_batch_report(None, None, None, 15, 20, 1.0, 1, p(pose), res, None, None) == -1
    assert lib.lfx_localize_host_report(None, None, None, 15, 20, 1.0, None, 0, None, 0, p(pose), res, rep, None) == -1
    assert lib.lfx_localize_host_report(None, None, None, 15, 20, 1.0, None, 0, None, 0, p(pose), res, None, None) == -1
    assert lib.lfx_scan_to_map_align_report(None, None, None, 15, 20, None, None, None, 1, 0, 0, None, None, None, 1, 0, 0, 1,
                                            p(pose), res, rep, None) == -1
    assert lib.lfx_scan_to_map_align_report(None, None, None, 15, 20, None, None, None, 1, 0, 0, None, None, None, 1, 0, 0, 1,
                                            p(pose), res, None, None) == -1
