"""The visibility cases hold what they say (CPU): the restatement (tests/visibility_restatement.py) gives every hand probe the
vote word written beside it, every condition a probe is named after occurs bit for bit, every group shows every outcome and
both decisions, the layout case has all three outcomes on both sides of its boundaries, and the scene meets the issue's
conditions -- so a device that equals the restatement byte for byte (tests/test_visibility_gpu.py) has passed something."""
import numpy as np
import pytest

from tests import keyframes_restatement as KR
from tests import visibility_cases as VC
from tests.visibility_restatement import AGREE, NEITHER, NO_VOTE, THROUGH, Rule, build_masked

OUTCOME = {"through": THROUGH, "agree": AGREE, "neither": NEITHER, "no vote": NO_VOTE}
GROUPS = VC.hand_groups()


def group(name):
    return next(g for g in GROUPS if g.name == name)


def record(g, name):
    kind, i = g.where(name)
    return g.store().records(kind)[i]


def seen(g, name):
    """the surface records of the first viewer of the probe's cluster"""
    return g.store().clouds[VC.SURFACE][g.probes[name]["viewer"]]


@pytest.mark.parametrize("g", GROUPS, ids=lambda g: g.name)
def test_every_probe_gets_the_word_written_beside_it(g):
    rule, s = Rule(**g.fields), g.store()
    first, count = g.window()
    votes, flags, res = rule.run(s, first, count)
    tally, _, _, images = rule.tally(s, first, count)
    for name, p in g.probes.items():
        kind, i = g.where(name)
        word = int(votes[kind][i])
        assert (word & 0xFFFF, word >> 16) == tuple(p["want"]), name
        if p["dynamic"] is not None:
            assert int(flags[kind][i]) == p["dynamic"], name
        if p["outcome"] is not None:
            o = rule.vote(s.pose[p["keyframe"]], s.clouds[kind][p["keyframe"]], s.pose[p["viewer"]], images[p["viewer"]])
            assert o[p["index"]] == OUTCOME[p["outcome"]], name
    # nothing vacuous: every outcome and both decisions occur in the group
    total = tally[0].sum(0) + tally[1].sum(0)
    assert total[THROUGH] > 0 and total[AGREE] > 0 and total[NEITHER] > 0
    dyn = np.concatenate(flags)
    assert dyn.any() and not dyn.all() and res["n_dynamic"][0] + res["n_dynamic"][1] == int(dyn.sum())
    assert all(a >= b for a, b in zip(res["n_records"], res["n_voted"])) and res["occupied_cells"] > 0


def test_column_probes_are_what_they_are_named_after():
    g = group("columns")
    rule = Rule(**g.fields)
    for name, col in g.marks.items():
        x, y, z, _ = record(g, name)
        row, c, r = rule.cell(np.float64([x]), np.float64([y]), np.float64([z]))
        assert (row[0], c[0]) == (2, col), name
        assert rule.cell(*(np.float64([v]) for v in seen(g, name)[0][:3]))[1][0] == col, name
    y = {n: record(g, n)[1] for n in g.marks}
    assert y["x>0 y=+0"] == 0 and not np.signbit(y["x>0 y=+0"]) and y["x>0 y=-0"] == 0 and np.signbit(y["x>0 y=-0"])
    assert y["x<0 y=+sub"] == VC.SUB and y["x<0 y=-sub"] == -VC.SUB and VC.SUB > 0 and VC.SUB / np.float32(2) == 0
    x, yy = record(g, "cross zero")[:2]
    cross = rule.col_cos[5] * np.float64(yy) - rule.col_sin[5] * np.float64(x)
    assert cross == 0.0 and rule.col_cos[5] != rule.col_sin[5] and x == yy
    dx, dy = record(g, "direction 5")[:2]
    assert (dx, dy) == (np.float32(rule.col_cos[5] * 4.0), np.float32(rule.col_sin[5] * 4.0))
    assert record(g, "direction 5 up")[1] == np.nextafter(dy, np.float32(9)) and record(g, "direction 5 down")[1] == np.nextafter(dy, np.float32(0))
    assert g.marks["direction 5 up"] != g.marks["direction 5 down"]


@pytest.mark.parametrize("name", ["rows first", "rows inner", "rows last"])
def test_row_probes_sit_on_the_boundary_bit_for_bit(name):
    g = group(name)
    rule, j = Rule(**g.fields), g.marks["j"]
    assert rule.row_tan[j] == 0.0 and (j == 0 or rule.row_tan[j - 1] < 0) and (j == 4 or rule.row_tan[j + 1] > 0)
    for pname, want_row in g.marks.items():
        if pname == "j":
            continue
        x, y, z, _ = record(g, pname)
        rho = np.sqrt(np.float64(x) * np.float64(x) + np.float64(y) * np.float64(y))
        assert rho == 5.0
        row = rule.cell(np.float64([x]), np.float64([y]), np.float64([z]))[0][0]
        assert row == (-1 if want_row is None else want_row), pname
        if pname.startswith("on"):
            assert np.float64(z) == rule.row_tan[j] * rho
    assert record(g, "below")[2] == np.nextafter(np.float32(0), np.float32(-1)) and record(g, "above")[2] == np.nextafter(np.float32(0), np.float32(1))
    if name == "rows inner":
        assert np.float64(record(g, "over the top row")[2]) >= rule.row_tan[4] * 5.0 and np.float64(record(g, "under the bottom row")[2]) < rule.row_tan[0] * 5.0


def rng_of(rec):
    x, y, z = (np.float64(v) for v in rec[:3])
    return np.sqrt((x * x + y * y) + z * z)


def test_range_probes_sit_on_the_gates():
    g = group("range")
    rule = Rule(**g.fields)
    s = seen(g, "image at min_range")
    assert rng_of(s[0]) == rule.min_range == 5.0 and rng_of(s[1]) == rule.max_range == 15.0 and rng_of(s[2]) < rule.max_range and s[2][1] == np.nextafter(np.float32(12), np.float32(0))
    assert rng_of(record(g, "target at min_range")) == rule.min_range and rng_of(record(g, "target at max_range")) == rule.max_range
    assert rng_of(record(g, "target under min_range")) < rule.min_range and record(g, "target under min_range")[1] == np.nextafter(np.float32(3), np.float32(0))
    assert rng_of(record(g, "target under max_range")) < rule.max_range and record(g, "target under max_range")[1] == np.nextafter(np.float32(9), np.float32(0))


def test_margin_probes_sit_on_the_margins():
    g = group("margins")
    rule = Rule(**g.fields)
    R = np.float64(np.float32(rng_of(seen(g, "R == r_q + m")[0])))
    assert R == 10.0 and rule.margin_abs == 1.25 and rule.margin_rel == 0.0
    assert rng_of(record(g, "R == r_q + m")) + rule.margin_abs == R and rng_of(record(g, "R == r_q - m")) - rule.margin_abs == R
    over, under = record(g, "R just over r_q + m"), record(g, "R just under r_q - m")
    assert over[0] == np.nextafter(np.float32(7), np.float32(0)) and rng_of(over) + rule.margin_abs < R
    assert under[1] == np.nextafter(np.float32(9), np.float32(99)) and rng_of(under) - rule.margin_abs > R
    g = group("margin selection")
    rule = Rule(**g.fields)
    rel = {n: rule.margin_rel * rng_of(record(g, n)) for n in ("rel larger", "abs larger", "equal")}
    assert rel["rel larger"] > rule.margin_abs and rel["abs larger"] < rule.margin_abs and rel["equal"] == rule.margin_abs
    cells = seen(g, "equal")
    for n, cell in (("rel larger", cells[0]), ("abs larger", cells[1]), ("equal", cells[2])):
        assert rng_of(record(g, n)) + max(rule.margin_abs, rel[n]) == np.float64(np.float32(rng_of(cell))), n


@pytest.mark.parametrize("guard", [0, 1, 2])
def test_window_probes_sit_where_the_window_ends(guard):
    g = group("window guard %d" % guard)
    rule = Rule(**g.fields)
    assert rule.guard == guard

    def cells(name):
        c = seen(g, name)
        row, col, r = rule.cell(*(c[:, a].astype(np.float64) for a in range(3)))
        return [(int(a), int(b)) for a, b in zip(row, col)], r
    for name in g.probes:
        if name.startswith("filler"):
            continue
        p = record(g, name)
        row, col, r = rule.cell(*(np.float64([v]) for v in p[:3]))
        centre = (int(row[0]), int(col[0]))
        got, ranges = cells(name)
        near = [c for c, rr in zip(got, ranges) if rr < r[0]]
        inside = [c for c in near if abs(c[0] - centre[0]) <= guard and min((c[1] - centre[1]) % 8, (centre[1] - c[1]) % 8) <= guard]
        if name.startswith("centre empty"):
            assert centre not in got and len(inside) == (0 if guard == 0 else 4)
            continue
        assert centre in got and centre not in near, name
        assert (g.probes[name]["want"] == (1, 0)) == (not inside), name
        if "corner only" in name:
            assert len(near) == 1 and abs(near[0][0] - centre[0]) == guard and (near[0][1] - centre[1]) % 8 in (guard, 8 - guard), name
        if "one past" in name:
            assert len(near) == 1 and max(abs(near[0][0] - centre[0]), (near[0][1] - centre[1]) % 8) == guard + 1, name
        if name.startswith("seam"):
            assert {centre[1], near[0][1]} == {0, 7}, name
        if name.startswith("rows clipped at 0"):
            assert centre[0] == 0
        if name.startswith("rows clipped at H"):
            assert centre[0] == 3


def test_pair_probes_sit_on_the_radius_and_outside_the_window():
    g = group("pairs")
    rule, s = Rule(**g.fields), g.store()
    first, count = g.window()
    for name, beyond in (("viewer at radius", False), ("viewer one double past the radius", True)):
        p = g.probes[name]
        d = s.pose[p["keyframe"]][:, 3] - s.pose[p["viewer"]][:, 3]
        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        assert (d2 > rule.radius2) if beyond else (d2 == rule.radius2 == 225.0), name
        assert abs(d[1]) == (np.nextafter(12.0, 13.0) if beyond else 12.0)
    for k in (g.marks["empty viewer"], g.marks["empty target"]):
        assert first <= k < first + count and len(s.clouds[0][k]) + len(s.clouds[1][k]) == 0
    lead, trail = g.marks["outside"]
    assert lead == 0 < first and trail == len(s) - 1 >= first + count
    for out, name in ((lead, "a viewer in front of the window"), (trail, "a viewer behind the window")):
        k = g.probes[name]["keyframe"]
        assert rule.qualifies(s.pose[k], s.pose[out]) and len(s.clouds[1][out]) > 0
        o = rule.vote(s.pose[k], s.clouds[0][k], s.pose[out], rule.image([s.clouds[0][out], s.clouds[1][out]]))
        assert o[g.probes[name]["index"]] == THROUGH       # it would have voted
    assert np.isnan(record(g, "nan x")[0]) and np.isnan(record(g, "nan z")[2]) and np.isinf(record(g, "inf y")[1])
    p = g.probes["behind max_range from the viewer"]
    o, det = rule.vote(s.pose[p["keyframe"]], s.clouds[0][p["keyframe"]], s.pose[p["viewer"]], rule.image([s.clouds[1][p["viewer"]]]), detail=True)
    i, j = p["index"], g.probes["in range from the viewer"]["index"]
    assert det["r"][i] >= rule.max_range > rng_of(record(g, "behind max_range from the viewer")) and o[i] == NO_VOTE
    assert det["r"][j] < rule.max_range and o[j] == AGREE
    # ... and would agree if the gate were missing
    R = np.float64(rule.image([s.clouds[1][p["viewer"]]]).max(initial=0, where=rule.image([s.clouds[1][p["viewer"]]]) != 0xFFFFFFFF).view(np.float32))
    assert det["r"][i] - rule.margin_abs <= R <= det["r"][i] + rule.margin_abs


def test_decision_groups_cover_the_thresholds():
    for weight in (1, 2, 0):
        g = group("decision weight %d" % weight)
        rule = Rule(**g.fields)
        assert rule.agree_weight == weight and rule.min_through == 2
        wants = {p["want"]: p["dynamic"] for n, p in g.probes.items() if not n.startswith("filler")}
        for (t, a), dyn in wants.items():
            assert dyn == int(t >= 2 and a * weight < t)
        if weight:
            assert any(t >= 2 and a * weight == t for t, a in wants) and any(t >= 2 and a * weight == t - 1 for t, a in wants)
    w1 = {p["want"] for p in group("decision weight 1").probes.values()}
    assert (2, 0) in w1 and (1, 0) in w1


@pytest.mark.parametrize("window", VC.LAYOUT_WINDOWS)
def test_layout_has_every_outcome_on_both_sides_of_its_boundaries(window):
    s, rule = VC.layout_case(), Rule(**VC.LAYOUT)
    first, count = window
    begin = s.begin(0).astype(np.int64)
    counts = np.diff(begin)
    n = len(s)
    assert any((counts[k:k + 300] == 1).all() for k in range(n - 300)) and any((counts[k:k + 40] == 0).all() for k in range(n - 40))
    assert counts.max() > 1024 and {int(b) % 64 for b in begin} >= {63, 0, 1}
    tally, pairs, viewers, _ = rule.tally(s, first, count)
    lo, hi = begin[first], begin[first + count]
    t = tally[0]
    assert ((t[lo:hi, 1:].sum(1) <= 1).all()) and t[:lo].sum() == 0 and t[hi:].sum() == 0
    outcome = np.where(t[:, THROUGH] > 0, THROUGH, np.where(t[:, AGREE] > 0, AGREE, np.where(t[:, NEITHER] > 0, NEITHER, NO_VOTE)))
    # a record's kind is its store index mod 3, wherever a partner looks
    voted = outcome[lo:hi] != NO_VOTE
    assert (outcome[lo:hi][voted] == np.array([THROUGH, AGREE, NEITHER])[np.arange(lo, hi) % 3][voted]).all() and voted.mean() > 0.5
    every = {THROUGH, AGREE, NEITHER}
    checked, seen_offsets = 0, set()
    bounds = sorted({int(b) for b in begin[first:first + count + 1] if lo < b < hi} | set(range(int(lo) + 64, int(hi), 64)))
    for b in bounds:
        left, right = outcome[max(lo, b - 3):b], outcome[b:min(hi, b + 3)]
        if len(left) == 3 and len(right) == 3 and NO_VOTE not in left and NO_VOTE not in right:
            assert set(left) == every and set(right) == every
            checked += 1
            seen_offsets.add((b - int(lo)) % 64)
    assert checked > 0.5 * len(bounds) and seen_offsets >= {63, 0, 1}
    inside = next(k for k in range(n) if counts[k] > 1024)
    if window != (0, n):
        assert first > 0 and first + count < n and first <= inside < first + count
    # the flags: one partner decides (min_through 1)
    _, flags, res = rule.run(s, first, count)
    assert (flags[0][lo:hi] == (outcome[lo:hi] == THROUGH)).all() and 0 < res["n_dynamic"][0] < res["n_voted"][0] < res["n_records"][0]


def test_scene_meets_the_conditions():
    """The one behavioural pin.  The restatement's own counts, guard 1: walls and fixed pillars 0 of 76 077 DYNAMIC, ground 0 of
    8 227, the moving pillar 1 990 of 2 096 (94.9 %); guard 0: ground 2 409 of 8 227, the moving pillar 1 992."""
    s, classes = VC.scene_case()
    assert len(s) == 6 and int(s.begin(0)[-1]) + int(s.begin(1)[-1]) == 6 * 16 * 900 and int(s.begin(1)[-1]) == 6 * 16 * 900 // 3
    dyn = {}
    for guard in (1, 0):
        _, flags, res = Rule(**dict(VC.SCENE, guard=guard)).run(s)
        dyn[guard] = {c: (sum(int(flags[k][classes[k] == c].sum()) for k in range(2)), sum(int((classes[k] == c).sum()) for k in range(2)))
                      for c in (VC.WALL, VC.GROUND, VC.MOVING)}
        print("guard %d: walls and fixed pillars %d of %d, ground %d of %d, moving pillar %d of %d DYNAMIC; %s" % (
            (guard,) + dyn[guard][VC.WALL] + dyn[guard][VC.GROUND] + dyn[guard][VC.MOVING] + (res,)))
    wall, ground, moving = dyn[1][VC.WALL], dyn[1][VC.GROUND], dyn[1][VC.MOVING]
    assert wall[0] == 0 and wall[1] > 20000
    assert ground[0] <= 0.005 * ground[1] and ground[1] > 2000
    assert moving[0] >= 0.9 * moving[1] and moving[1] > 500
    assert dyn[0][VC.GROUND][0] > ground[0]


def test_build_masked_restated_on_a_hand_store():
    s = KR.Store(4, (8, 8))
    clouds = [np.arange(4 * n, dtype=np.float32).reshape(n, 4) + 100 * k for k, n in enumerate((3, 0, 2, 1))]
    assert s.add(clouds, clouds, [KR.pose([0, 0, 0], [k, 0, 0]) for k in range(4)]) == 0
    flags = np.array([0, 1, 0, 1, 0, 0], np.uint8)
    cloud, begin = build_masked(s, 0, flags)
    assert begin.tolist() == [0, 2, 2, 3, 4] and (cloud == s.build(0)[[0, 2, 4, 5]]).all()
    cloud, begin = build_masked(s, 0, flags, 2, 2)
    assert begin.tolist() == [0, 1, 2] and (cloud == s.build(0)[[4, 5]]).all()
    assert len(build_masked(s, 0, np.ones(6, np.uint8))[0]) == 0 and (build_masked(s, 0, np.zeros(6, np.uint8))[0] == s.build(0)).all()


def test_tables_are_the_segmentation_columns_and_the_row_tangents():
    import lidar_feature_extraction_amd as lfx
    from lidar_feature_extraction_amd import binding as B
    for fields in (dict(), VC.BASE, VC.SCENE, dict(n_rows=128, n_columns=4096, elev_min=-1.5, elev_step=0.0234)):
        cfg = lfx.visibility_config(**fields)
        cs, sn, rt = lfx.visibility_tables(cfg)
        seg = lfx.segment_tables(dict(n_rows=1, n_columns=int(cfg.n_columns), ground_first_row=0, ground_last_row=0))
        assert cs.tobytes() == seg[0].tobytes() and sn.tobytes() == seg[1].tobytes() and len(rt) == cfg.n_rows + 1
        for j in range(cfg.n_rows + 1):
            want = np.tan(np.float64(np.float32(cfg.elev_min)) + np.float64(j) * np.float64(np.float32(cfg.elev_step)))
            assert abs(rt[j] - want) <= 2 * np.spacing(abs(want)) and (j == 0 or rt[j] > rt[j - 1])
    d = lfx.visibility_config()
    assert (d.n_rows, d.n_columns, d.guard, d.min_through, d.agree_weight, d.reserved) == (32, 360, 1, 2, 1, 0)
    assert (d.elev_min, d.elev_step, d.min_range, d.max_range, d.radius, d.margin_abs, d.margin_rel) == tuple(
        np.float32(v) for v in (-0.43633232, 0.027270770, 1.0, 100.0, 15.0, 0.3, 0.02))
    for bad in (dict(n_rows=0), dict(n_columns=6 + 1), dict(elev_min=-1.5707964), dict(elev_step=-0.1), dict(max_range=float("inf")), dict(guard=3),
                dict(min_through=0), dict(margin_abs=float("nan")), dict(radius=-0.0 - 1e-9), dict(reserved=7)):
        with pytest.raises(B.LfxError) as err:
            lfx.visibility_tables(lfx.visibility_config(**bad))
        assert err.value.code == B.ERR_INVALID_ARGUMENT, bad
    assert lfx.visibility_tables(lfx.visibility_config(agree_weight=0, radius=0.0, margin_abs=0.0, margin_rel=0.0, guard=0))[2][0] < 0
