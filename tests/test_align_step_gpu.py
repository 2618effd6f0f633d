"""ONE iteration of the robust Gauss-Newton loop on the device (align_scale_kernel, align_update_kernel and, for the report,
align_report_scale_kernel / align_report_kernel) through the public entry points with max_iter = 1, against the CPU oracle
and against tests/align_step_restatement.py, whose sums are exact.  tests/test_align_gpu.py runs the loop to convergence on
continuous noise, which forgives a wrong weight or a mis-selected median and never produces two equal errors; here the
errors are known exactly, tie in every way, sit on both sides of every boundary of the two kernels, and what comes back
after the one step is compared

  * bit for bit: error_scale with orc_loc_scale and with the sorted() restatement; the error with math.fsum where every order
    of the additions gives one number; a scale of 0 as 0.0; every result alone and inside a ragged batch;
  * to a bound derived beforehand (align_step_restatement.py: B = (rows + 64) 2^-53 cond2(H) |dx|): the pose after the step.

Cases: tests/align_step_cases.py.  tests/test_align_step_expect.py holds cases and restatement to the oracle on the CPU."""
import numpy as np
import pytest

from tests import align_step_cases as AC
from tests.align_step_restatement import restate_step
from tests.report_restatement import restate

pytestmark = pytest.mark.gpu

K = AC.K_NEIGHBOURS
WORST = {}                                               # family -> (ratio of |dP| to B, case): printed by every test of the family


@pytest.fixture(scope="module")
def fx():
    from lidar_feature_extraction_amd import FeatureExtraction
    ctx = FeatureExtraction(device=0, max_points_per_scan=1024, max_batch=1)
    yield ctx
    ctx.close()


def _dev():
    import torch
    return torch.device("cuda", 0)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _up(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype).copy()).to(_dev())


def _run_pairs(fx, cases):
    """One lfx_align_point_pairs call with max_iter = 1 for all the problems (ragged: one after the other)."""
    counts = np.array([len(c["X"]) for c in cases], np.int32)
    begins = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32)
    total = int(counts.sum())
    X = np.concatenate([np.asarray(c["X"], np.float64).reshape(-1, 3) for c in cases] + [np.zeros((1, 3))])
    Y = np.concatenate([np.asarray(c["Y"], np.float64).reshape(-1, 3) for c in cases] + [np.zeros((1, 3))])
    dX, dY, db, dn = _up(X, np.float64), _up(Y, np.float64), _up(begins, np.int32), _up(counts, np.int32)
    return fx.align_point_pairs(dX.data_ptr(), dY.data_ptr(), db.data_ptr(), dn.data_ptr(), int(counts.max()), total, 1,
                                np.stack([c["pose"] for c in cases]), _stream())


def _same_bytes(a, b):
    return a["pose"].tobytes() == b["pose"].tobytes() and (a["code"], a["iteration"]) == (b["code"], b["iteration"]) and \
        AC.bits(a["error"]) == AC.bits(b["error"]) and AC.bits(a["error_scale"]) == AC.bits(b["error_scale"])


EMPTY = dict(X=np.zeros((0, 3)), Y=np.zeros((0, 3)), pose=AC.translation((0.25, 0.0, -4.0)), name="empty", n=0)


def _is_empty_result(r, case):
    return (r["code"], r["iteration"], r["success"]) == (4, 0, False) and AC.bits(r["error"]) == AC.bits(0.0) and \
        AC.bits(r["error_scale"]) == AC.bits(0.0) and r["pose"].tobytes() == case["pose"].tobytes()


def _report(family, ratios):
    worst = max(ratios) if ratios else (0.0, "no case with a step")
    if family not in WORST or worst[0] > WORST[family][0]:
        WORST[family] = worst
    print("family %s: the device's worst |dP| / B here %.3g (%s); so far %.3g (%s)" % ((family,) + worst + WORST[family]))


_BATCHES = {}                                            # family key -> (cases, the device's results in one ragged call)


def _batch(fx, key, build):
    """The problems of one family in ONE ragged call with an empty one in the middle (so that `begin` offsets are arbitrary),
    run once per module and shared by the tests of the family's counts."""
    if key not in _BATCHES:
        cases = build()
        half = len(cases) // 2
        got = _run_pairs(fx, cases[:half] + [EMPTY] + cases[half:])
        assert _is_empty_result(got[half], EMPTY), got[half]
        _BATCHES[key] = (cases, got[:half] + got[half + 1:])
    return _BATCHES[key]


def _check_pair(fx, case, r, ratios):
    """One problem's result inside the ragged batch: the same bytes as alone; against the restatement and the oracle."""
    what = case["name"]
    alone = _run_pairs(fx, [case])[0]
    assert _same_bytes(r, alone), (what, r, alone)
    want, orc = AC.expected(case), AC.oracle_pairs(case)
    print(what, "error", r["error"], "scale", r["error_scale"], "code", r["code"], "iteration", r["iteration"],
          "|dP|", float(np.abs(r["pose"] - want["pose"]).max()), "B", want["bound"], "cond", want["cond"], "|dx|", want["dx_norm"])
    AC.check_result(case, r, want, what, ratios)
    assert (r["code"], r["iteration"], r["success"]) == (orc["code"], orc["iteration"], orc["success"]), (what, r, orc)
    assert float(np.abs(r["pose"] - orc["pose"]).max()) <= want["pose_bound"], (what, r["pose"], orc["pose"])
    if case["kind"] != "rotated":
        assert AC.bits(r["error_scale"]) == AC.bits(orc["error_scale"]) == AC.bits(AC.oracle_scale(case["errors"])), (what, r, orc)
        if case["exact_sum"]:
            assert AC.bits(r["error"]) == AC.bits(orc["error"]), (what, r["error"], orc["error"])
        if case["kind"] in AC.ZERO_SCALE_KINDS and case["n"] > 2:
            assert AC.bits(r["error_scale"]) == AC.bits(0.0), (what, r["error_scale"])     # 0.0: not a denormal, not -0.0
    if want["degenerate"]:
        assert (r["code"], r["iteration"]) == (0, 0) and r["pose"].tobytes() == case["pose"].tobytes(), (what, r)


PAIR_PARAMS = [(kind, arrangement, n) for kind in AC.KINDS for arrangement in AC.ARRANGEMENTS for n in AC.COUNTS if AC.makes_sense(kind, n)]


@pytest.mark.parametrize("kind,arrangement,n", PAIR_PARAMS)
def test_pair_problems_with_exactly_known_errors(fx, kind, arrangement, n):
    """Family A: residuals (a_i, 0, 0) exactly, every count of AC.COUNTS (1 .. 5, around 64, around the scale kernel's 1 024
    threads = one 3 072-row sweep of the update kernel, both sides of the 6 144-key LDS / global split, 12 289), every kind of
    tie, every arrangement over the waves.  The counts of one (kind, arrangement) share one ragged call."""
    cases, got = _batch(fx, (kind, arrangement), lambda: AC.pair_cases(kind, arrangement))
    at = [c["n"] for c in cases].index(n)
    ratios = []
    _check_pair(fx, cases[at], got[at], ratios)
    _report("A", ratios)


OTHER_NAMES = ["generic, n = 200001, shuffled", "generic, n = 64, shuffled, X = 0", "two-valued-split, n = 1025, shuffled, X = 0",
               "generic, n = 1, shuffled", "generic, n = 2, shuffled", "wide-exponent, n = 2, shuffled"] + \
    ["rotated, n = %d" % n for n in AC.ROTATED_COUNTS]


@pytest.mark.parametrize("name", OTHER_NAMES)
def test_the_largest_problem_degenerate_inputs_and_rotated_poses(fx, name):
    """200 001 pairs (once); X = 0 and n = 1, 2 (no step, CONVERGED at iteration 0, the pose untouched, error and scale still
    exact); problems at generic rotated poses (errors to 1e-7, the pose by B): n mod 4, the sweep boundary, 6 144 / 6 145.
    All in one ragged call."""
    cases, got = _batch(fx, "others", lambda: [AC.big_case()] + AC.degenerate_cases() + AC.rotated_cases())
    assert [c["name"] for c in cases] == OTHER_NAMES
    at = OTHER_NAMES.index(name)
    ratios = []
    _check_pair(fx, cases[at], got[at], ratios)
    _report("A", ratios)


# ---- family B: edge and surface rows together ------------------------------------------------------------------------------

def _lay(parts, width=4):
    n = np.array([len(p) for p in parts], np.int32)
    b = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int32)
    pts = np.concatenate([np.asarray(p, np.float32).reshape(-1, width) for p in parts] + [np.zeros((1, width), np.float32)])
    return _up(pts, np.float32), _up(b, np.int32), _up(n, np.int32), n


def _align(fx, emap, smap, cases, report=False):
    d_e, d_eb, d_en, en = _lay([c["edge"] for c in cases])
    d_s, d_sb, d_sn, sn = _lay([c["surface"] for c in cases])
    return fx.scan_to_map_align(emap, smap, K, 1, d_e.data_ptr(), d_eb.data_ptr(), d_en.data_ptr(), 1, int(en.max()), int(en.sum()),
                                d_s.data_ptr(), d_sb.data_ptr(), d_sn.data_ptr(), 1, int(sn.max()), int(sn.sum()),
                                np.stack([c["pose"] for c in cases]), _stream(), report=report)


def _rows(fx, emap, smap, pose, edge, surface):
    """The rows of one scan at `pose` through lfx_scan_to_map_residuals (held to the oracle by tests/test_residuals_gpu.py)."""
    import torch
    out = []
    for kind, m, pts, width in ((0, emap, edge, 3), (1, smap, surface, 1)):
        n = len(pts)
        d_p, d_b, d_n = _up(np.vstack([pts, np.zeros((1, 4), np.float32)]), np.float32), _up([0], np.int32), _up([n], np.int32)
        d_r = torch.zeros((n + 1, width), dtype=torch.float64, device=_dev())
        d_j = torch.zeros((n + 1, 7 * width), dtype=torch.float64, device=_dev())
        if n:
            fx.scan_to_map_residuals(kind, m, pose, K, d_p.data_ptr(), d_b.data_ptr(), d_n.data_ptr(), 1, 1, n, d_r.data_ptr(),
                                     d_j.data_ptr(), _stream())
        torch.cuda.synchronize()
        out += [d_r.cpu().numpy()[:n], d_j.cpu().numpy()[:n]]
    return out


def _check_mixed(case, r, want, ratios):
    """A family-B result against the restatement of the device's own rows.  Returns whether the case was excluded (then only
    error and scale are compared)."""
    what = case["name"]
    diff = float(np.abs(r["pose"] - want["pose"]).max())
    print(what, "error", r["error"], "scale", r["error_scale"], "code", r["code"], "iteration", r["iteration"], "|dP|", diff,
          "B", want["bound"], "cond", want["cond"], "|dx|", want["dx_norm"], "excluded", want["excluded"])
    # (the device's ComputeErrors may fuse its products: the errors agree to an ulp, not to the bit, so error and scale to the
    # 1e-7 of tests/test_align_gpu.py -- except a scale of exactly 0, which no rounding of non-zero errors produces)
    assert abs(r["error"] - want["error"]) <= 1e-7 * abs(want["error"]) + 1e-18, (what, r["error"], want["error"])
    assert abs(r["error_scale"] - want["error_scale"]) <= 1e-7 * abs(want["error_scale"]) + 1e-18, (what, r["error_scale"], want["error_scale"])
    if want["error_scale"] == 0.0:
        assert AC.bits(r["error_scale"]) == AC.bits(0.0), (what, r["error_scale"])
    if want["excluded"]:
        return True
    assert (r["code"], r["iteration"]) == (want["code"], want["iteration"]), (what, r, want["code"], want["iteration"])
    assert diff <= want["pose_bound"], (what, diff, want["pose_bound"], want["cond"], want["dx_norm"])
    if want["degenerate"] or want["code"] in (4, 5):
        assert r["pose"].tobytes() == case["pose"].tobytes(), what
    if want["bound"] > 0:
        ratios.append((diff / want["bound"], what))
    return False


@pytest.fixture(scope="module")
def scene():
    return AC.mixed_scene()


@pytest.mark.parametrize("cell", [1.0, 0.0])
def test_edge_and_surface_rows_together(fx, scene, cell):
    """Family B: caller-laid clouds against grid maps and no-grid maps, one iteration.  3 n3 mod 4 and (3 n3 + n1) mod 4 take all
    16 combinations with a real step (n3 = 40 .. 43, n1 = 100 .. 103): the boundary between 3-row and 1-row residuals and the
    ragged last group at every place inside a group of four; the tiny ones (n3, n1 = 0 .. 3: surface-only, edge-only, empty);
    n3 + n1 = 6 144 and 6 145; all in one call with non-zero begins, and each alone with the same bytes.  Expected: the
    restatement of the rows the device's own residual entry point gives at the same pose."""
    assert AC.MIXED_COUNTS == [(a, b) for a in (40, 41, 42, 43) for b in (100, 101, 102, 103)]
    assert [a + b for a, b in AC.SPLIT_COUNTS] == [6144, 6145]
    cases = AC.mixed_cases(scene)
    emap = fx.make_map_from_host(scene["edge_map"], cell)
    smap = fx.make_map_from_host(scene["surface_map"], 2.0 * cell)
    got = _align(fx, emap, smap, cases)
    ratios, excluded, residues, failures = [], 0, set(), []
    for case, r in zip(cases, got):                      # (every case is looked at: the first failure does not hide the rest)
        try:
            alone = _align(fx, emap, smap, [case])[0]
            assert _same_bytes(r, alone), (case["name"], r, alone)
            want = restate_step(case["pose"], *_rows(fx, emap, smap, case["pose"], case["edge"], case["surface"]))
            excluded += int(_check_mixed(case, r, want, ratios))
            if (case["n3"], case["n1"]) in AC.MIXED_COUNTS and not want["excluded"]:
                assert not want["degenerate"] and want["dx_norm"] > 1e-6, case["name"]            # a real step
                residues.add((3 * case["n3"] % 4, (3 * case["n3"] + case["n1"]) % 4))
        except AssertionError as err:
            failures.append((case["name"], str(err)[:300]))
    assert not failures, failures
    print("family B, cell %g: %d of %d cases excluded, %d residues of 16 with a step" % (cell, excluded, len(cases), len(residues)))
    assert 16 * excluded <= len(cases), excluded
    assert len(residues) == 16
    _report("B", ratios)
    emap.close()
    smap.close()


def test_a_majority_of_zero_rows_and_its_report(fx, scene):
    """A surface map with clusters of coincident points: more than half of the scan's rows are zero rows (the device's own rows
    decide the share), so the scale is exactly 0 and every other row weighs 1.345 / sqrt(e / 1e-16).  The step against the
    restatement; the same scan through lfx_scan_to_map_align_report: its result is the plain call's, and error_scale, the
    inlier counts, sigma2 and the information matrix are report_restatement.restate's on the rows at the returned pose, under
    the tolerances of tests/test_align_report_gpu.py (1e-9 relative; counts equal) -- the only reach into the report
    kernels' selection on ties."""
    case = AC.zero_row_case(scene)
    emap = fx.make_map_from_host(scene["edge_map"], 1.0)
    smap = fx.make_map_from_host(scene["coincident_map"], 2.0)
    r3, J3, r1, J1 = _rows(fx, emap, smap, case["pose"], case["edge"], case["surface"])
    zero_rows = int((~J1.any(axis=1) & (r1.reshape(-1) == 0)).sum())
    print("zero rows: %d of %d surface rows, %d rows in all" % (zero_rows, len(r1), len(r1) + len(r3)))
    assert 2 * zero_rows > len(r1) and 2 * zero_rows > len(r1) + len(r3) and zero_rows < len(r1)
    want = restate_step(case["pose"], r3, J3, r1, J1)
    assert AC.bits(want["error_scale"]) == AC.bits(0.0) and not want["excluded"] and not want["degenerate"]
    got = _align(fx, emap, smap, [case])[0]
    ratios = []
    assert not _check_mixed(case, got, want, ratios)
    assert AC.bits(got["error_scale"]) == AC.bits(0.0)
    _report("B", ratios)
    res, reps = _align(fx, emap, smap, [case], report=True)
    assert _same_bytes(res[0], got)
    rep = reps[0]
    at = restate(got["pose"], *_rows(fx, emap, smap, got["pose"], case["edge"], case["surface"]))
    rel = lambda a, b: abs(a - b) / max(abs(b), 1e-300)   # noqa: E731
    figures = dict(error=rel(rep["error"], at["error"]), sigma2=rel(rep["sigma2"], at["sigma2"]),
                   information=np.linalg.norm(rep["information"] - at["information"]) / np.linalg.norm(at["information"]))
    print("report: error_scale", rep["error_scale"], "restated", at["error_scale"], figures, "inliers", rep["n_edge_inliers"],
          rep["n_surface_inliers"], "restated", at["n_edge_inliers"], at["n_surface_inliers"], "no plane", rep["n_surface_no_plane"])
    assert rep["valid"] and (rep["n_edge"], rep["n_surface"]) == (case["n3"], case["n1"])
    assert 2 * rep["n_surface_no_plane"] > case["n3"] + case["n1"] and rep["n_surface_no_plane"] == at["n_surface_no_plane"]
    assert at["error_scale"] == 0.0 and AC.bits(rep["error_scale"]) == AC.bits(0.0), rep["error_scale"]
    assert not at["near_threshold"], "a residual at the Huber threshold (choose another input)"
    assert (rep["n_edge_inliers"], rep["n_surface_inliers"]) == (at["n_edge_inliers"], at["n_surface_inliers"])
    for k, v in figures.items():
        assert v <= 1e-9, (k, v)
    emap.close()
    smap.close()
