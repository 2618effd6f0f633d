"""The helpers of the launch-scale comparison (tests/launch_scale.py) on the CPU: the ring-major expectation inverts to the
oracle's per-point arrays, and the comparison core -- on a batch faked in numpy -- passes, ignores what lies beyond each ring's
count, and catches every kind of single wrong element."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lidar_feature_extraction_amd import make_scan, synth  # noqa: E402
from oracle import binding as OB  # noqa: E402
from tests import launch_scale as LS  # noqa: E402

R, COLS, CAP = 16, 300, 320


def _three():
    """(cloud as the device is given it, keep or None, oracle result): plain, ragged with a sparse ring, filtered through keep."""
    plain = make_scan(R, COLS, seed=8101)
    ragged = make_scan(R, COLS, seed=8102, drop_fraction=0.07)
    few = ragged["ring"] == 7
    ragged = synth.concat([ragged[~few], ragged[few][:4]])        # ring 7: 4 points, removed as sparse
    holes = make_scan(R, COLS, seed=8103)
    zero = np.random.default_rng(5).uniform(0, 1, len(holes)) < 0.06
    zero |= holes["ring"] == R - 1                                 # the last ring has no return at all
    for f in ("x", "y", "z"):
        holes[f][zero] = 0.0
    keep = np.nonzero(~zero)[0]
    out = []
    for cloud, kp in ((plain, None), (ragged, None), (holes, keep)):
        want = OB.extract(cloud if kp is None else np.ascontiguousarray(cloud[kp]), canonical_ties=False)
        LS.require_tie_free(want, "scan %d" % len(out))
        out.append((cloud, kp, want))
    return out


@pytest.fixture(scope="module")
def three():
    return _three()


def test_expectation_inverts_to_the_oracles_per_point_arrays(three):
    for i, (cloud, keep, want) in enumerate(three):
        exp = LS.expected_ring_major(want, R, CAP, keep)
        labels, curv, seen = LS.invert_ring_major(exp, len(cloud))
        at = np.arange(len(cloud)) if keep is None else keep
        assert seen[at].all() and seen.sum() == len(at), "scan %d: every kept point exactly once" % i
        assert np.array_equal(labels[at], want["labels"]), "scan %d: labels" % i
        assert curv[at].tobytes() == want["curvature"].tobytes(), "scan %d: curvature" % i
        assert exp["valid"].sum(axis=1).tolist() == exp["ring_count"][:R].tolist()
        assert exp["n_edge"] == len(want["edge_index"]) and exp["n_surface"] == len(want["surface_index"])
    assert three[1][2]["ring_status"][list(three[1][2]["ring_id"]).index(7)] != 0 and LS.expected_ring_major(three[1][2], R, CAP)["ring_skipped"][7]
    assert LS.expected_ring_major(three[2][2], R, CAP, three[2][1])["ring_count"][R - 1] == 0


POISON = 0xA5


def _fake_batch(exp, pick, routes):
    """What a device would hold: expectations at their places, POISON bytes everywhere else."""
    B = len(pick)
    begin = np.concatenate([[0], np.cumsum(exp.n_points[pick])]).astype(np.uint32)
    total = int(begin[-1])

    def poisoned(shape, dtype):
        a = np.empty(shape, dtype)
        a.view(np.uint8)[...] = POISON
        return a

    got = {"scan_begin": begin, "scan_info": np.zeros((B, 4), np.uint32), "ring_count": np.zeros((B, LS.K_RINGS), np.uint32),
           "ring_status": poisoned((B, LS.K_RINGS), np.uint8)}
    for name, dtype in (("labels_sorted", np.uint8), ("curvature_sorted", np.float64), ("sorted_index", np.uint32)):
        got[name] = poisoned((B, R, CAP), dtype)
    for kind in ("edge", "surface"):
        got[kind + "_points"] = poisoned((total, 4), np.float32)
        got[kind + "_index"] = poisoned(total, np.uint32)
    for s, u in enumerate(pick):
        e = exp.per_scan[u]
        got["scan_info"][s] = (int((e["ring_count"] > 0).sum()), routes[s], e["n_edge"], e["n_surface"])
        got["ring_count"][s] = e["ring_count"]
        occupied = e["ring_count"] > 0
        got["ring_status"][s][occupied] = np.where(e["ring_skipped"][occupied], 3, 0)
        for name in ("labels_sorted", "curvature_sorted", "sorted_index"):
            if name == "sorted_index" and routes[s] == LS.ORGANISED:
                continue                                            # (an organised scan: sorted_index holds nothing)
            got[name][s][e["valid"]] = e[name][e["valid"]]
        for kind in ("edge", "surface"):
            n = e["n_" + kind]
            got[kind + "_points"][begin[s]:begin[s] + n] = e[kind + "_points"]
            got[kind + "_index"][begin[s]:begin[s] + n] = e[kind + "_index"]
    return got


@pytest.fixture(scope="module")
def fake(three):
    exp = LS.Expected([LS.expected_ring_major(w, R, CAP, k) for _, k, w in three], [len(c) for c, _, _ in three])
    pick = np.array([0, 1, 2, 1, 0, 2, 2])
    routes = [LS.ORGANISED if u == 0 else (0x800 if u == 2 else 0x200) for u in pick]
    return exp, pick, _fake_batch(exp, pick, routes)


def _copy(got):
    return {k: v.copy() for k, v in got.items()}


def test_comparison_passes_and_ignores_what_lies_beyond_the_counts(fake):
    exp, pick, got = fake
    assert LS.compare_batch(got, pick, exp, R, "fake") == len(pick)
    other = _copy(got)
    for name in ("labels_sorted", "curvature_sorted", "sorted_index"):       # another poison: still equal
        other[name][~exp.valid[pick]] = 7
    assert LS.compare_batch(other, pick, exp, R, "fake") == len(pick)
    no_curv = _copy(got)
    no_curv["curvature_sorted"] = None
    assert LS.compare_batch(no_curv, pick, exp, R, "fake") == len(pick)


def _first_valid(exp, u, ring_from=0):
    r, k = np.argwhere(exp.valid[u][ring_from:])[len(np.argwhere(exp.valid[u][ring_from:])) // 2]
    return int(r) + ring_from, int(k)


@pytest.mark.parametrize("fault", ["label", "curvature ulp", "records swapped", "n_edge", "sorted_index", "index list", "ring_count",
                                   "ring_status", "scan_begin"])
def test_comparison_catches_a_single_wrong_element(fake, fault):
    exp, pick, got = fake
    bad = _copy(got)
    s = 5                                                           # (a position that is neither the first nor the last)
    u = int(pick[s])
    r, k = _first_valid(exp, u, 3)
    if fault == "label":
        bad["labels_sorted"][s, r, k] ^= 1
        array = "labels_sorted"
    elif fault == "curvature ulp":
        bad["curvature_sorted"][s, r, k] = np.nextafter(bad["curvature_sorted"][s, r, k], np.inf)
        array = "curvature_sorted"
    elif fault == "records swapped":
        b = int(bad["scan_begin"][s])
        assert exp.n_surface[u] >= 2
        bad["surface_points"][[b, b + 1]] = bad["surface_points"][[b + 1, b]]
        array = "surface_points"
    elif fault == "n_edge":
        bad["scan_info"][s, 2] += 1
        array = "n_edge"
    elif fault == "sorted_index":
        bad["sorted_index"][s, r, k] += 1
        array = "sorted_index"
    elif fault == "index list":
        bad["edge_index"][int(bad["scan_begin"][s]) + exp.n_edge[u] - 1] ^= 2
        array = "edge_index"
    elif fault == "ring_count":
        bad["ring_count"][s, r] -= 1
        array = "ring_count"
    elif fault == "ring_status":
        bad["ring_status"][s, r] = 0 if exp.ring_skipped[u][r] else 5
        array = "ring_status"
    else:
        bad["scan_begin"][s] += 1
        array = "scan_begin"
    with pytest.raises(AssertionError) as err:
        LS.compare_batch(bad, pick, exp, R, "fake call 0")
    text = str(err.value)
    assert "fake call 0" in text and "position %d" % s in text and "distinct scan %d" % u in text and array in text, text


def test_an_organised_scans_index_array_is_not_read(fake):
    exp, pick, got = fake
    bad = _copy(got)
    bad["sorted_index"][0] = 123                                   # position 0 holds distinct scan 0, read in place
    assert LS.compare_batch(bad, pick, exp, R, "fake") == len(pick)
    bad["scan_info"][0, 1] = 0x200                                 # ... the same scan reported as bucketed: now it counts
    with pytest.raises(AssertionError, match="sorted_index"):
        LS.compare_batch(bad, pick, exp, R, "fake")
