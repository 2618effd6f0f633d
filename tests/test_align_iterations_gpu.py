"""The scan-to-map alignment loop from its SECOND iteration on, and the report after it, on the device through the public
entry points alone (scan_to_map_align with and without report, scan_to_map_residuals, make_map_from_host).

From iteration 1 on map_search_kernel starts every query from a bound -- reach[] of the search before plus the query's
movement since AlignState::prev_m -- and nearest_in_grid_wave then enlarges its first cube, drops rows, clips runs of cells
and grows with the bar still bounded; the report pass runs the same warm search from whatever the loop left behind; and only
across iterations do the prev_error / prev_scale tests, the `done` gating, the iterations queued ahead of the host's look and
scans of one batch stopping at different iterations come into play.  A warm search that loses one true neighbour in a few
hundred queries converges to the same pose within 1e-6, so whole runs to convergence do not notice; one iteration at a time
does (tests/test_align_iterations_expect.py: one wrong neighbour moves a step by 10^4 .. 10^7 pose_bound).

For every case of tests/align_iteration_cases.py, every (cell pair, n_neighbors) and max_iter = m = 1..5, with R_m the result:
  1. iteration m against restate_iteration on the rows the COLD entry point gives at the pose before (R_{m-1}.pose), with
     prev_error / prev_scale from the restated chain: error and scale to 1e-7, code and iteration equal, the pose within the
     restatement's derived pose_bound, the pose's bytes unchanged where no step is taken;
  2. a run that stopped early gives the same bytes under every larger limit;
  3. the oracle's own loop orc_loc_optimize_scan(start, m): code, iteration, the pose to 1e-6;
  4. report = True returns the same result bytes and a report that passes the checks of tests/test_align_report_gpu.py against
     report_restatement.restate on the cold rows at R_m.pose -- for every m, so after steps of metres too;
  5. all scans of one (cell pair, k, m) in one ragged call, an empty scan in the middle: each the bytes it has alone (result
     and report), the scans stopping at three or more different iterations from m = 3 on; and a second ragged call against the
     map of coincident clusters with the empty scan and the scan without a plane in the middle;
  6. one context for the whole module, whose first call is a 6 145-row scan (the scratch then holds stale neighbour lists and
     reaches of a longer call) and is repeated last with the same bytes.
cell = 0 is the control: no grid, no warm start.  No number here comes from the device: the references are the oracle, the
cold entry point (held to the oracle by tests/test_residuals_gpu.py) and the numpy restatements."""
import numpy as np
import pytest

from tests import align_iteration_cases as IC
from tests import align_step_cases as AC
from tests.align_step_restatement import EMPTY, LARGER_ERROR, LARGER_SCALE, MAX_ITERATION, NO_PLANE
from tests.report_restatement import restate
from tests.test_align_report_gpu import _all_zero, _check
from tests.test_align_step_gpu import _check_mixed, _lay, _report, _same_bytes, _stream, _up

pytestmark = pytest.mark.gpu

PARAMS = [(cells, k) for cells in IC.CELL_PAIRS for k in IC.NEIGHBOURS]
_STATE = {}                                              # the module's context-wide records: maps, first call, runs


@pytest.fixture(scope="module")
def scene():
    return IC.scene()


def _align(fx, maps, cases, k, max_iter, report=False):
    d_e, d_eb, d_en, en = _lay([c["edge"] for c in cases])
    d_s, d_sb, d_sn, sn = _lay([c["surface"] for c in cases])
    return fx.scan_to_map_align(maps[0], maps[1], k, max_iter, d_e.data_ptr(), d_eb.data_ptr(), d_en.data_ptr(), 1, int(en.max()), int(en.sum()),
                                d_s.data_ptr(), d_sb.data_ptr(), d_sn.data_ptr(), 1, int(sn.max()), int(sn.sum()),
                                np.stack([c["pose"] for c in cases]), _stream(), report=report)


def _cold_rows(fx, maps, pose, case, k):
    """The rows of one scan at `pose` through lfx_scan_to_map_residuals: every search from infinity."""
    import torch
    dev, out = torch.device("cuda", 0), []
    for kind, m, pts, width in ((0, maps[0], case["edge"], 3), (1, maps[1], case["surface"], 1)):
        n = len(pts)
        d_p, d_b, d_n = _up(np.vstack([pts, np.zeros((1, 4), np.float32)]), np.float32), _up([0], np.int32), _up([n], np.int32)
        d_r = torch.zeros((n + 1, width), dtype=torch.float64, device=dev)
        d_j = torch.zeros((n + 1, 7 * width), dtype=torch.float64, device=dev)
        if n:
            fx.scan_to_map_residuals(kind, m, pose, k, d_p.data_ptr(), d_b.data_ptr(), d_n.data_ptr(), 1, 1, n, d_r.data_ptr(), d_j.data_ptr(),
                                     _stream())
        torch.cuda.synchronize()
        out += [d_r.cpu().numpy()[:n], d_j.cpu().numpy()[:n]]
    return out


def _first_call(fx, scene):
    """The 6 145-row scan of family B (AC.SPLIT_COUNTS), five iterations and a report, against the 1.0 / 2.0 grids."""
    case = AC.mixed_cases(scene)[-1]
    assert case["n3"] + case["n1"] == 6145
    return _align(fx, _maps(fx, scene, IC.CELL_PAIRS[0], "scene"), [case], AC.K_NEIGHBOURS, 5, report=True)


def _maps(fx, scene, cells, which):
    key = ("maps", cells, which)
    if key not in _STATE:
        e, s = dict(scene=("edge_map", "surface_map"), small=("small_edge_map", "small_surface_map"), coincident=("edge_map", "coincident_map"))[which]
        _STATE[key] = (fx.make_map_from_host(scene[e], cells[0]), fx.make_map_from_host(scene[s], cells[1]))
    return _STATE[key]


@pytest.fixture(scope="module")
def fx(scene):
    from lidar_feature_extraction_amd import FeatureExtraction
    ctx = FeatureExtraction(device=0, max_points_per_scan=1024, max_batch=1)
    _STATE.clear()
    _STATE["first"] = _first_call(ctx, scene)            # before every small call of the module
    yield ctx
    for key, value in _STATE.items():
        if key[0] == "maps":
            value[0].close()
            value[1].close()
    _STATE.clear()
    ctx.close()


def _runs(fx, scene, cells, k):
    """Everything the device is asked for one (cell pair, k), once: per case R_m and the report call for m = 1..5, the cold
    rows at every pose met, the restated chain on them and the restated reports.  A list of per-case records."""
    key = ("runs", cells, k)
    if key in _STATE:
        return _STATE[key]
    records = []
    for case in IC.cases(scene, k):
        maps, host_maps = _maps(fx, scene, cells, case["maps"]), IC.maps_of(scene, case)
        rows_at = {}

        def cold(pose):
            b = np.ascontiguousarray(pose, np.float64).tobytes()
            if b not in rows_at:
                rows_at[b] = _cold_rows(fx, maps, pose, case, k)
            return rows_at[b]

        rec = dict(case=case, host_maps=host_maps, R={}, REP={}, want={}, want_oracle_rows={}, want_report={}, before={}, stopped_at=None,
                   gap=np.inf)
        for m in IC.MAX_ITERS:
            rec["R"][m] = _align(fx, maps, [case], k, m)[0]
            res, reps = _align(fx, maps, [case], k, m, report=True)
            rec["REP"][m] = (res[0], reps[0])
        Q, prev_error, prev_scale = np.ascontiguousarray(case["pose"], np.float64), IC.DBL_MAX, IC.DBL_MAX
        for m in IC.MAX_ITERS:
            r = rec["R"][m]
            if rec["stopped_at"] is None:
                rec["before"][m] = Q
                want = IC.restate_iteration(Q, cold(Q), prev_error, prev_scale, True, m)
                rec["want"][m] = want
                rec["want_oracle_rows"][m] = IC.restate_iteration(Q, IC.oracle_rows_at(host_maps, case, Q, k), prev_error, prev_scale, True, m)
                rec["gap"] = min(rec["gap"], IC.smallest_gap(host_maps, case, Q, k), IC.smallest_gap(host_maps, case, r["pose"], k))
                if r["code"] != MAX_ITERATION or r["iteration"] != m:
                    rec["stopped_at"] = m
                else:
                    Q, prev_error, prev_scale = np.ascontiguousarray(r["pose"]), want["error"], want["error_scale"]
            if r["code"] not in (EMPTY, NO_PLANE) and np.isfinite(r["pose"]).all():
                rec["want_report"][m] = restate(r["pose"], *cold(r["pose"]))
        records.append(rec)
    _STATE[key] = records
    return records


def _name(cells, k, rec, m):
    return "cells %g / %g, k = %d, %s, m = %d" % (cells[0], cells[1], k, rec["case"]["name"], m)


@pytest.mark.parametrize("cells,k", PARAMS)
def test_every_iteration_against_its_restatement(fx, scene, cells, k):
    """Checks 1 and 2."""
    ratios, checked, excluded, failures, gap = [], 0, 0, [], np.inf
    for rec in _runs(fx, scene, cells, k):
        gap = min(gap, rec["gap"])
        for m in IC.MAX_ITERS:
            what, r = _name(cells, k, rec, m), rec["R"][m]
            try:
                if m not in rec["want"]:                 # stopped before: the limit no longer matters
                    first = rec["R"][rec["stopped_at"]]
                    assert _same_bytes(r, first), (what, r, first)
                    continue
                want, Q = rec["want"][m], rec["before"][m]
                checked += 1
                out = want["excluded"] or want["near_stop"]
                excluded += int(out)
                skipped = _check_mixed(dict(name=what, pose=Q), r, dict(want, excluded=out), ratios)
                if not skipped and want["no_step"] and (m > 1 or want["code"] in (LARGER_ERROR, LARGER_SCALE)):
                    assert r["pose"].tobytes() == Q.tobytes(), what
                by_oracle = rec["want_oracle_rows"][m]
                if not skipped and not (by_oracle["excluded"] or by_oracle["near_stop"]):
                    assert (r["code"], r["iteration"]) == (by_oracle["code"], by_oracle["iteration"]), (what, r, by_oracle["code"])
                    assert np.abs(r["pose"] - by_oracle["pose"]).max() <= 1e-6 * (1 + np.abs(by_oracle["pose"]).max()), what
            except AssertionError as err:                # (every case is looked at: the first failure does not hide the rest)
                failures.append((what, str(err)[:400]))
    print("cells %g / %g, k = %d: %d iterations checked, %d excluded, the smallest gap between a k-th and a (k + 1)-th neighbour %.3g m" % (
        cells + (k, checked, excluded, gap)))
    _report("iterations, cells %g / %g" % cells, ratios)
    assert not failures, failures
    assert gap > IC.MIN_GAP, ("choose another input", gap)
    assert 16 * excluded <= checked, ("choose another input", excluded, checked)


@pytest.mark.parametrize("cells,k", PARAMS)
def test_the_oracle_s_own_loop(fx, scene, cells, k):
    """Check 3: orc_loc_optimize_scan(start, m) -- code and iteration equal and the pose to 1e-6; where an error or a scale of
    the restated chain ties with the one before, within one iteration and 2e-3 as tools/stress_localize.py counts it."""
    ties, checked = 0, 0
    for rec in _runs(fx, scene, cells, k):
        near = False
        for m in IC.MAX_ITERS:
            what, r = _name(cells, k, rec, m), rec["R"][m]
            near = near or (m in rec["want"] and rec["want"][m]["near_stop"])
            w = IC.oracle_loop(rec["host_maps"], rec["case"], k, m)
            checked += 1
            diff = float(np.abs(r["pose"] - w["pose"]).max())
            print(what, "code", r["code"], "iteration", r["iteration"], "the oracle's", w["code"], w["iteration"], "|dP|", diff)
            if near and (r["code"], r["iteration"]) != (w["code"], w["iteration"]):
                ties += 1
                assert abs(r["iteration"] - w["iteration"]) <= 1 and r["success"] == w["success"] and diff < 2e-3, (what, r, w)
                continue
            assert (r["code"], r["iteration"], r["success"]) == (w["code"], w["iteration"], w["success"]), (what, r, w)
            assert diff <= 1e-6 * (1 + np.abs(w["pose"]).max()), (what, diff, r, w)
    print("cells %g / %g, k = %d: %d runs against the oracle's loop, %d at a tie" % (cells + (k, checked, ties)))
    assert 16 * ties <= checked, ("choose another input", ties, checked)


@pytest.mark.parametrize("cells,k", PARAMS)
def test_the_report_after_every_limit(fx, scene, cells, k):
    """Check 4: the report's warm search starts from the reach and prev_m the loop left -- one step of up to metres behind the
    returned pose after CONVERGED / MAX_ITERATION, prev_m one pose behind reach[] after LARGER_ERROR / LARGER_SCALE."""
    checked, loose, failures, codes = 0, 0, [], set()
    for rec in _runs(fx, scene, cells, k):
        for m in IC.MAX_ITERS:
            what, r, (res, rep) = _name(cells, k, rec, m), rec["R"][m], rec["REP"][m]
            try:
                assert _same_bytes(res, r), (what, res, r)
                if m not in rec["want_report"]:
                    assert _all_zero(rep), what
                    continue
                checked += 1
                codes.add(r["code"])
                want = rec["want_report"][m]
                loose += int(want["near_threshold"])     # (the inlier counts are then a matter of rounding: not compared)
                _check(rep, want, what, inliers=not want["near_threshold"])
            except AssertionError as err:
                failures.append((what, str(err)[:400]))
    print("cells %g / %g, k = %d: %d reports checked after the codes %s, %d without their inlier counts" % (cells + (k, checked, sorted(codes), loose)))
    assert not failures, failures
    assert 16 * loose <= checked, ("choose another input", loose, checked)


@pytest.mark.parametrize("cells,k", PARAMS)
def test_ragged_batches_whose_scans_stop_at_different_iterations(fx, scene, cells, k):
    """Check 5."""
    records = [rec for rec in _runs(fx, scene, cells, k) if rec["case"]["maps"] == "scene"]
    cases, empty, no_plane = [rec["case"] for rec in records], IC.empty_case(), IC.no_plane_case(scene)
    half = len(cases) // 2
    maps, cmaps = _maps(fx, scene, cells, "scene"), _maps(fx, scene, cells, "coincident")
    for m in IC.MAX_ITERS:
        res, reps = _align(fx, maps, cases[:half] + [empty] + cases[half:], k, m, report=True)
        e = res.pop(half)
        assert (e["code"], e["iteration"]) == (EMPTY, 0) and e["pose"].tobytes() == empty["pose"].tobytes() and _all_zero(reps.pop(half)), (m, e)
        stops = {0}
        for rec, r, rep in zip(records, res, reps):
            what = _name(cells, k, rec, m)
            assert _same_bytes(r, rec["R"][m]), (what, r, rec["R"][m])
            assert rep["raw"] == rec["REP"][m][1]["raw"], what
            ends = [j for j in sorted(rec["want"]) if j <= m and (rec["want"][j]["code"] != MAX_ITERATION or j == m)]
            stops.add(rec["want"][ends[0]]["iteration"])  # (from the restated chain, not from the device)
        print("cells %g / %g, k = %d, m = %d: the scans of the batch stop at iterations" % (cells + (k, m)), sorted(stops))
        assert m < 3 or len(stops) >= 3, ("choose another input", m, stops)
        # against the map of coincident clusters: two scans that iterate, the empty one and the one without a plane between them
        mixed = [cases[0], empty, no_plane, cases[2]]
        got = _align(fx, cmaps, mixed, k, m)
        assert [(g["code"], g["iteration"]) for g in got[1:3]] == [(EMPTY, 0), (NO_PLANE, 0)], (m, got[1:3])
        assert got[2]["pose"].tobytes() == no_plane["pose"].tobytes()
        for c, g in zip(mixed, got):
            alone = _align(fx, cmaps, [c], k, m)[0]
            assert _same_bytes(g, alone), (cells, k, m, c["name"], g, alone)


def test_the_module_s_first_call_again(fx, scene):
    """Check 6: the 6 145-row call that ran before everything else in this context, after all the small calls: the same bytes."""
    res0, rep0 = _STATE["first"]
    res, rep = _first_call(fx, scene)
    assert _same_bytes(res[0], res0[0]), (res[0], res0[0])
    assert rep0[0]["valid"] and rep[0]["raw"] == rep0[0]["raw"]
