"""lfx_align_report at its edges on the device (align_report_scale_kernel, align_report_kernel's second half: report_finish_h /
report_finish_d), through lfx_scan_to_map_align_report on caller-laid clouds.  Cases and constants: tests/align_report_cases.py
(held to what they claim by tests/test_align_report_expect.py on the host).  Of every case's record:

  * bit for bit: error_scale with align_scale_kernel's at the same pose (a plain call with max_iter = 1 from result.pose, held
    to the oracle by tests/test_align_step_gpu.py; result.error_scale itself where the pose did not move); eigenvalues,
    eigenvectors, covariance and rank with align_report_reference.algorithm on the record's own information and sigma2; the
    whole record alone, inside a ragged batch with an empty scan in the middle, and on a second call;
  * to the 50-digit reference of the rows lfx_scan_to_map_residuals gives at result.pose: the counts (where no normalised
    error lies within 1e-6 of 1.345^2), information, error, sigma2 and the rms values within C_SUM * MARGIN * 2^-53 * the
    sum's largest term, min_eigenvalue_d within C_EIG * 2^-53 |D|_2, degenerate;
  * exactly: the symmetry of the matrices, the order of the eigenvalues, the sign rule, the rank as the count above the floor,
    a NaN sigma2 with an all-NaN covariance and valid = 1 exactly where sum w dim - 6 <= 0.

Every test prints its figures before it asserts; one context for the module; every case runs once and its tests share it."""
import math

import numpy as np
import pytest

from tests import align_report_cases as RC
from tests import align_report_reference as RR
from tests import align_step_cases as AC

pytestmark = pytest.mark.gpu

K = RC.K
HAND_MAX_ITER = 20
EMPTY = dict(name="empty", edge=np.zeros((0, 4), np.float32), surface=np.zeros((0, 4), np.float32), pose=AC.translation((0.25, 0.0, -4.0)),
             n3=0, n1=0)
SELECTION = [c["name"] for c in RC.selection_cases()]
NONEMPTY = [c["name"] for c in RC.selection_cases() if c["n3"] + c["n1"] > 0]
TINY = [c["name"] for c in RC.selection_cases() if RC.is_tiny(c) and c["n3"] + c["n1"] > 0]
HAND = list(RC.HAND)
WORST = {}                                               # field -> (the device's worst ratio to its unit so far, case)


@pytest.fixture(scope="module")
def fx():
    from lidar_feature_extraction_amd import FeatureExtraction
    ctx = FeatureExtraction(device=0, max_points_per_scan=1024, max_batch=1)
    yield ctx
    for m in _MAPS.values():
        m.close()
    for cache in (_MAPS, _OUTCOMES, _BATCHES, WORST):
        cache.clear()
    ctx.close()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _up(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype).copy()).to(torch.device("cuda", 0))


def _lay(parts):
    n = np.array([len(p) for p in parts], np.int32)
    b = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int32)
    pts = np.concatenate([np.asarray(p, np.float32).reshape(-1, 4) for p in parts] + [np.zeros((1, 4), np.float32)])
    return _up(pts, np.float32), _up(b, np.int32), _up(n, np.int32), n


def _align(fx, maps, cases, max_iter, report, poses=None):
    d_e, d_eb, d_en, en = _lay([c["edge"] for c in cases])
    d_s, d_sb, d_sn, sn = _lay([c["surface"] for c in cases])
    poses = np.stack([c["pose"] for c in cases]) if poses is None else poses
    return fx.scan_to_map_align(maps[0], maps[1], K, max_iter, d_e.data_ptr(), d_eb.data_ptr(), d_en.data_ptr(), 1, int(en.max()),
                                int(en.sum()), d_s.data_ptr(), d_sb.data_ptr(), d_sn.data_ptr(), 1, int(sn.max()), int(sn.sum()), poses,
                                _stream(), report=report)


def _rows(fx, maps, pose, edge, surface):
    """The rows of one scan at `pose` through lfx_scan_to_map_residuals (held to a 50-digit reference by tests/test_rows_gpu.py)"""
    import torch
    out = []
    for kind, m, pts, width in ((0, maps[0], edge, 3), (1, maps[1], surface, 1)):
        n = len(pts)
        d_p, d_b, d_n = _up(np.vstack([pts, np.zeros((1, 4), np.float32)]), np.float32), _up([0], np.int32), _up([n], np.int32)
        d_r = torch.zeros((n + 1, width), dtype=torch.float64, device=d_p.device)
        d_j = torch.zeros((n + 1, 7 * width), dtype=torch.float64, device=d_p.device)
        if n:
            fx.scan_to_map_residuals(kind, m, pose, K, d_p.data_ptr(), d_b.data_ptr(), d_n.data_ptr(), 1, 1, n, d_r.data_ptr(),
                                     d_j.data_ptr(), _stream())
        torch.cuda.synchronize()
        out += [d_r.cpu().numpy()[:n], d_j.cpu().numpy()[:n]]
    return out[0], out[1], out[2].reshape(-1), out[3]


_MAPS, _OUTCOMES, _BATCHES = {}, {}, {}


def _maps_of(fx, case):
    out = []
    for k in ("edge_map", "surface_map"):
        key = id(case[k])
        if key not in _MAPS:
            _MAPS[key] = fx.make_map_from_host(case[k], 1.0 if k == "edge_map" else 2.0)
        out.append(_MAPS[key])
    return out


def _case(name):
    return [c for c in RC.selection_cases() + RC.hand_cases() if c["name"] == name][0]


def _in_its_batch(fx, name):
    """(result, report) of the case inside a ragged call with an empty scan in the middle: the selection cases that share
    their maps in ONE call (the empty scan is TINY_COUNTS' (0, 0)), every other case as [case, empty, case]"""
    case = _case(name)
    shared = [c for c in RC.selection_cases() if c["edge_map"] is case["edge_map"] and c["surface_map"] is case["surface_map"]]
    if name in SELECTION and len(shared) > 1:
        if "selection" not in _BATCHES:
            res, reps = _align(fx, _maps_of(fx, case), shared, 1, True)
            empty = [i for i, c in enumerate(shared) if c["n3"] + c["n1"] == 0]
            assert empty and 0 < empty[0] < len(shared) - 1
            _BATCHES["selection"] = {c["name"]: (r, p) for c, r, p in zip(shared, res, reps)}
        return _BATCHES["selection"][name]
    res, reps = _align(fx, _maps_of(fx, case), [case, EMPTY, case], 1 if name in SELECTION else HAND_MAX_ITER, True)
    assert reps[0]["raw"] == reps[2]["raw"] and not reps[1]["valid"] and reps[1]["raw"] == bytes(len(reps[1]["raw"])), name
    return res[2], reps[2]


def _outcome(fx, name):
    """Everything the tests of one case share: its result and record in the batch, alone and on a second call, the rows at
    result.pose and their 50-digit reference."""
    if name in _OUTCOMES:
        return _OUTCOMES[name]
    case, maps = _case(name), _maps_of(fx, _case(name))
    max_iter = 1 if name in SELECTION else HAND_MAX_ITER
    res, rep = _in_its_batch(fx, name)
    alone_res, alone = _align(fx, maps, [case], max_iter, True)
    _, again = _align(fx, maps, [case], max_iter, True)
    out = dict(case=case, res=res, rep=rep, alone=alone[0], again=again[0], alone_res=alone_res[0], maps=maps, max_iter=max_iter)
    if case["n3"] + case["n1"] > 0 and rep["valid"]:
        out["rows"] = _rows(fx, maps, res["pose"], case["edge"], case["surface"])
        out["ref"] = RR.reference(res["pose"], *out["rows"])
    _OUTCOMES[name] = out
    return out


def _note(field, ratio, name):
    if field not in WORST or ratio > WORST[field][0]:
        WORST[field] = (ratio, name)


# ---- every case: the record's structure, the eigen-solves' bits, the sums to the definition -------------------------------------

def _check_structure(rep, what):
    lam, vec = rep["eigenvalues"], rep["eigenvectors"]
    assert rep["information"].tobytes() == np.ascontiguousarray(rep["information"].T).tobytes(), what
    assert rep["covariance"].tobytes() == np.ascontiguousarray(rep["covariance"].T).tobytes() or np.isnan(rep["covariance"]).all(), what
    assert np.all(np.diff(lam) >= 0), (what, lam)
    orth = float(np.abs(vec @ vec.T - np.eye(6)).max())
    assert orth <= 1e-14, (what, orth)
    for k in range(6):
        assert vec[k][int(np.argmax(np.abs(vec[k])))] > 0, (what, k, vec[k])
    assert rep["rank"] == int((lam > RR.FLOOR * lam[5]).sum()), (what, lam)
    return orth


def _check_record(o, name):
    rep, res = o["rep"], o["res"]
    assert rep["valid"], name
    ref = o["ref"]
    assert rep["raw"] == o["alone"]["raw"], name + ": the record differs between the batch and the scan alone"
    assert rep["raw"] == o["again"]["raw"], name + ": the record differs on a second call"
    assert res["pose"].tobytes() == o["alone_res"]["pose"].tobytes(), name
    near = ref["huber_margin"] <= RC.HUBER_MARGIN
    sums = RC.sum_ratios(rep, ref)
    d_err, d_bound = abs(rep["min_eigenvalue_d"] - ref["min_eigenvalue_d"]), RC.d_bound(ref)
    bad = RR.mismatches(rep)
    print(name, "code", res["code"], "iteration", res["iteration"], "|pose - start| %.3g" % float(np.abs(res["pose"] - o["case"]["pose"]).max()),
          "rows", rep["n_edge"], rep["n_surface"], "inliers", rep["n_edge_inliers"], rep["n_surface_inliers"], "no plane", rep["n_surface_no_plane"],
          "rank", rep["rank"], "degenerate", rep["degenerate"], "sigma2", rep["sigma2"], "scale", rep["error_scale"],
          "sums / unit (bound %g)" % (RC.C_SUM * RC.MARGIN), {k: float("%.3g" % v) for k, v in sums.items()},
          "min eigenvalue of D %.6g, off by %.3g 2^-53 |D|_2 (bound %g)" % (rep["min_eigenvalue_d"], d_err / d_bound * RC.C_EIG, RC.C_EIG),
          "Huber margin %.3g" % ref["huber_margin"], "eigenvalues", rep["eigenvalues"], "not the restatement's bytes:", bad)
    orth = _check_structure(rep, name)
    print(name, "orthonormal to %.3g" % orth)
    assert (rep["n_edge"], rep["n_surface"]) == (ref["n_edge"], ref["n_surface"]), name
    assert rep["n_surface_no_plane"] == ref["n_surface_no_plane"], name
    assert not bad, (name, bad)
    assert math.isnan(rep["sigma2"]) == (not ref["dim"] > 0), (name, rep["sigma2"], ref["dim"])
    if math.isnan(rep["sigma2"]):
        assert np.isnan(rep["covariance"]).all(), name
    else:
        assert np.isfinite(rep["covariance"]).all(), name
    if not near:                                         # (only the counts are a matter of rounding there: the weights are continuous)
        assert (rep["n_edge_inliers"], rep["n_surface_inliers"]) == (ref["n_edge_inliers"], ref["n_surface_inliers"]), name
    for k, v in sums.items():
        _note(k, v, name)
        assert v <= RC.C_SUM * RC.MARGIN, (name, k, v)
    _note("min_eigenvalue_d", d_err / d_bound * RC.C_EIG, name)
    assert d_err <= d_bound, (name, rep["min_eigenvalue_d"], ref["min_eigenvalue_d"], d_bound)
    if abs(ref["min_eigenvalue_d"] - 0.1) > d_bound:
        assert rep["degenerate"] == (ref["min_eigenvalue_d"] < 0.1), name
    print("the device's worst ratios so far:", {k: (float("%.3g" % v[0]), v[1]) for k, v in WORST.items()})
    return near


@pytest.mark.parametrize("name", NONEMPTY)
def test_selection_cases(fx, name):
    """The report's copy of ComputeErrors / Scale / ComputeWeights: error_scale bit for bit with align_scale_kernel's at the
    pose the report was made at; counts, sums and the rest of the record as for every case."""
    o = _outcome(fx, name)
    case, res, rep = o["case"], o["res"], o["rep"]
    _check_record(o, name)
    moved = res["pose"].tobytes() != case["pose"].tobytes()
    plain = _align(fx, o["maps"], [case], 1, False, poses=res["pose"][None])[0]
    print(name, "moved", moved, "error_scale: report %r, the step kernel's at that pose %r, result %r" % (
        rep["error_scale"], plain["error_scale"], res["error_scale"]))
    # (the report's search is warm-started from the iteration before it, the plain call's is cold: both are exact searches,
    # held to each other by tests/test_align_iterations_gpu.py, so the rows and their scale are one)
    assert AC.bits(rep["error_scale"]) == AC.bits(plain["error_scale"]), name
    if not moved:
        assert AC.bits(rep["error_scale"]) == AC.bits(res["error_scale"]), name
    if name.startswith("zero rows"):
        assert AC.bits(rep["error_scale"]) == AC.bits(0.0) and 2 * rep["n_surface_no_plane"] > rep["n_edge"] + rep["n_surface"]


def test_at_most_one_selection_case_in_sixteen_is_excluded(fx):
    near = [n for n in NONEMPTY if _outcome(fx, n)["ref"]["huber_margin"] <= RC.HUBER_MARGIN]
    print("%d of %d selection cases with a normalised error within %g of 1.345^2 at the device's pose: %s" % (
        len(near), len(NONEMPTY), RC.HUBER_MARGIN, near))
    assert 16 * len(near) <= len(NONEMPTY)
    for n3, n1 in AC.SPLIT_COUNTS:                       # both sides of the 6 144-key split are among the compared
        assert "n3 = %d, n1 = %d" % (n3, n1) in NONEMPTY and "n3 = %d, n1 = %d" % (n3, n1) not in near


def test_the_empty_scan_keeps_the_all_zero_record(fx):
    o = _outcome(fx, "n3 = 0, n1 = 0")
    print("empty scan: code", o["res"]["code"], "valid", o["rep"]["valid"])
    for rep in (o["rep"], o["alone"], o["again"]):
        assert not rep["valid"] and rep["raw"] == bytes(len(rep["raw"]))
    assert o["res"]["code"] == 4


@pytest.mark.parametrize("name", TINY)
def test_tiny_scans_and_the_nan_sigma2(fx, name):
    """One to three residuals of a kind.  sigma2 is NaN exactly where sum w dim - 6 <= 0; the record is valid all the same, its
    covariance NaN in every entry, and information, eigenvalues, eigenvectors, rank, counts and rms values are the reference's
    (checked by _check_record as for every case: test_selection_cases runs it on these names too)."""
    o = _outcome(fx, name)
    rep, ref = o["rep"], o["ref"]
    print(name, "sum w dim - 6 = %r" % ref["dim"], "sigma2", rep["sigma2"], "valid", rep["valid"], "rank", rep["rank"],
          "covariance NaN entries", int(np.isnan(rep["covariance"]).sum()))
    assert rep["valid"] and math.isnan(rep["sigma2"]) == (not ref["dim"] > 0)
    assert int(np.isnan(rep["covariance"]).sum()) == (0 if ref["dim"] > 0 else 36)
    assert np.isfinite(rep["information"]).all() and np.isfinite(rep["eigenvalues"]).all() and np.isfinite(rep["eigenvectors"]).all()
    assert not RR.mismatches(rep)
    for k in ("rms_edge", "rms_surface", "error", "min_eigenvalue_d"):
        assert math.isfinite(rep[k]), (name, k)


@pytest.mark.parametrize("name", HAND)
def test_hand_scenes(fx, name):
    """The rank ladder, the diagonal H, the tie under the sign rule, both sides of the floor, the wide dynamic range."""
    o = _outcome(fx, name)
    case, res, rep = o["case"], o["res"], o["rep"]
    near = _check_record(o, name)
    assert not near, name
    # the scenes are laid so that the gradient at the start pose is rounding (the float32 of the rotated scan: 5e-7 m): what
    # the host claims of them at the start pose holds where the device reports
    assert float(np.abs(res["pose"] - case["pose"]).max()) <= 1e-5, (name, res["pose"])
    assert rep["rank"] == RC.HAND[name], (name, rep["eigenvalues"])
    lam, vec = rep["eigenvalues"], rep["eigenvectors"]
    if name in ("box", "box_square"):
        H = rep["information"]
        off = float(np.abs(H - np.diag(np.diag(H))).max())
        equal = [k for k in range(5) if lam[k + 1] - lam[k] <= 1e-12 * lam[5]]
        print(name, "largest off-diagonal entry of the device's H %.3g (%.3g ulp of the diagonal's largest); equal neighbours at" % (
            off, off / np.spacing(np.diag(H).max())), equal)
        assert off <= 64 * RC.MARGIN * np.spacing(np.diag(H).max())
        assert len(equal) >= 2
    if name == "wall_at_45":
        tied = []
        for k in range(6):
            order = np.argsort(-np.abs(vec[k]), kind="stable")
            a, b = vec[k][order[0]], vec[k][order[1]]
            if abs(a) - abs(b) <= 1e-5 * abs(a):
                tied.append((k, a, b))
                assert a > 0, (k, vec[k])            # the header's rule, on whichever is larger in the device's own vector
        print(name, "vectors whose two largest components tie (largest, second):", tied)
        assert tied
    if name in RC.WINDOW:
        floored = name == "converging_below_floor"
        along = rep["sigma2"] / (RR.FLOOR * lam[5] if floored else lam[0])
        print(name, "lambda_0 / lambda_5 %.3e, covariance along x %.6g against sigma2 / %s = %.6g" % (
            lam[0] / lam[5], rep["covariance"][3, 3], "floor" if floored else "lambda_0", along))
        assert abs(vec[0][3]) >= 0.999
        assert abs(rep["covariance"][3, 3] - along) <= 1e-2 * along
