"""The one-iteration alignment cases (tests/align_step_cases.py) and their restatement (tests/align_step_restatement.py) against
the CPU oracle alone, without a GPU: what tests/test_align_step_gpu.py holds the device to is itself held to the functions
the reference's own vectors pin (tests/test_oracle_localization.py): orc_loc_scale, orc_loc_median, orc_loc_is_degenerate,
orc_loc_huber_derivative, orc_loc_optimize_pairs, orc_loc_edge_residuals, orc_loc_surface_residuals."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import align_step_cases as AC
from tests.align_step_restatement import median_sorted, restate_step, scale_sorted

PD = AC.PD


@pytest.mark.parametrize("kind", AC.KINDS)
def test_every_pair_case_against_the_oracle(kind):
    """Every family-A builder reproduces its residuals exactly (asserted by the builder); orc_loc_scale equals the sorted()
    restatement bit for bit; the error is the exact sum where every order gives one number; orc_loc_optimize_pairs with one
    iteration stays within B of the exact-sum restatement, with its code and iteration; nothing is excluded; every number
    is finite."""
    ratios, zero_scales = [], 0
    for arrangement in AC.ARRANGEMENTS:
        for case in AC.pair_cases(kind, arrangement):
            e = case["errors"]
            assert case["exact_sum"] or kind not in AC.EXACT_SUM_KINDS, case["name"]
            want = AC.expected(case)
            assert want["errors_sorted"].tobytes() == np.sort(e).tobytes(), case["name"]    # the restatement's rows give the same errors
            s = AC.oracle_scale(e)
            assert AC.bits(s) == AC.bits(scale_sorted(e)) == AC.bits(want["error_scale"]), (case["name"], s, want["error_scale"])
            if kind in AC.ZERO_SCALE_KINDS and case["n"] > 2:
                assert AC.bits(s) == AC.bits(0.0), case["name"]
                zero_scales += 1
            AC.check_result(case, AC.oracle_pairs(case), want, case["name"], ratios)
            if case["n"] >= 3:
                assert not want["degenerate"] and want["dx_norm"] > 0, (case["name"], want["min_eigenvalue_d"])
    assert (zero_scales > 0) == (kind in AC.ZERO_SCALE_KINDS)
    worst = max(ratios)
    print("%s: the oracle's worst |dP| / B over %d cases: %.3g (%s)" % (kind, len(ratios), worst[0], worst[1]))


def test_the_largest_the_degenerate_and_the_rotated_cases_against_the_oracle():
    """The 200 001-pair case (once); X = 0 and n = 1, 2: no step, CONVERGED at iteration 0, the pose untouched, error and
    scale still exact; the rotated poses to tolerance."""
    ratios = []
    big = AC.big_case()
    assert big["exact_sum"]
    AC.check_result(big, AC.oracle_pairs(big), AC.expected(big), big["name"], ratios)
    for case in AC.degenerate_cases():
        want, got = AC.expected(case), AC.oracle_pairs(case)
        assert want["degenerate"] and (want["code"], want["iteration"]) == (0, 0), case["name"]
        assert got["pose"].tobytes() == case["pose"].tobytes() == want["pose"].tobytes(), case["name"]
        AC.check_result(case, got, want, case["name"], ratios)
        assert AC.bits(got["error"]) == AC.bits(math.fsum(case["errors"].tolist())), case["name"]
    for case in AC.rotated_cases():
        AC.check_result(case, AC.oracle_pairs(case), AC.expected(case), case["name"], ratios)
    worst = max(ratios)
    print("the oracle's worst |dP| / B: %.3g (%s)" % worst)


def test_the_restatement_s_median_and_degenerate_branch_against_the_oracle():
    from oracle import binding as OB
    L = OB.lib()
    L.orc_loc_median.restype = C.c_double
    rng = np.random.default_rng(9)
    for n in (1, 2, 3, 4, 7, 8, 64, 65):
        for v in (rng.uniform(0, 1, n), rng.integers(0, 3, n).astype(np.float64), np.zeros(n)):
            v = np.ascontiguousarray(v)
            assert AC.bits(L.orc_loc_median(OB.ptr(v, PD), n)) == AC.bits(median_sorted(v)), (n, v)
    # IsDegenerate: the restatement's eigvalsh branch on the D of cases on both sides of the threshold
    seen = set()
    cases = AC.degenerate_cases() + [AC.pair_case("generic", n) for n in (3, 4, 5, 63)] + [AC.pair_case("wide-exponent", 3)]
    for case in cases:
        want = AC.expected(case)
        D = np.ascontiguousarray(want["D"])
        assert bool(L.orc_loc_is_degenerate(OB.ptr(D, PD), 7, C.c_double(0.1))) == want["degenerate"], (case["name"], want["min_eigenvalue_d"])
        seen.add(want["degenerate"])
    assert seen == {True, False}


def test_the_mixed_cases_on_the_oracle_s_rows():
    """Family B on the CPU: the restatement on the rows orc_loc_edge_residuals / orc_loc_surface_residuals give for the same
    clouds.  Every step and code is defined, at most 1 case in 16 is excluded, the 16 residues of (3 n3, 3 n3 + n1) mod 4
    take a real step, and the scan against the coincident map has a majority of zero rows and a scale of exactly 0."""
    scene = AC.mixed_scene()
    cases = AC.mixed_cases(scene)
    excluded, residues = 0, set()
    for case in cases:
        r3, J3 = AC.oracle_rows(scene["edge_map"], 0, case["pose"], case["edge"])
        r1, J1 = AC.oracle_rows(scene["surface_map"], 1, case["pose"], case["surface"])
        want = restate_step(case["pose"], r3, J3, r1, J1)
        assert np.isfinite(want["pose"]).all() and want["code"] in (0, 3, 4, 5), (case["name"], want)
        excluded += int(want["excluded"])
        if (case["n3"], case["n1"]) in AC.MIXED_COUNTS:
            assert not want["degenerate"] and want["dx_norm"] > 0, case["name"]
            residues.add((3 * case["n3"] % 4, (3 * case["n3"] + case["n1"]) % 4))
    print("family B on the oracle's rows: %d of %d cases excluded" % (excluded, len(cases)))
    assert len(residues) == 16
    assert 16 * excluded <= len(cases), excluded
    z = AC.zero_row_case(scene)
    r3, J3 = AC.oracle_rows(scene["edge_map"], 0, z["pose"], z["edge"])
    r1, J1 = AC.oracle_rows(scene["coincident_map"], 1, z["pose"], z["surface"])
    zero_rows = int((~J1[:, 4:7].any(axis=1)).sum())
    want = restate_step(z["pose"], r3, J3, r1, J1)
    print("zero rows: %d of %d surface rows, %d rows" % (zero_rows, len(r1), len(r1) + len(r3)))
    assert 2 * zero_rows > len(r1) + len(r3) and zero_rows < len(r1)
    assert AC.bits(want["error_scale"]) == AC.bits(0.0) and not want["excluded"] and np.isfinite(want["pose"]).all()
