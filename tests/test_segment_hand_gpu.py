"""The hand cases of tests/test_segment_expect.py through the device: lfx_segment_batch on records that sit on the edges of
the header's arithmetic -- the column boundaries (y = +0.0 / -0.0, 1e-30, the smallest subnormal, the table's own directions
and their float neighbours), the range gates, a tie in one cell, the ground test at equality, the join test one float on
either side of its threshold.  Every probe is a scan of its own, with 1 to 3 records, so that it can join or shadow nothing
but itself; a batch of 32 or more probes also runs the 8-workgroups-per-scan launch shape with nearly empty scans.  Class, id
and counts equal the restatement byte for byte, and what the header fixes is written out by hand."""
import numpy as np
import pytest

from tests import deskew_cases as K
from tests import segment_cases as S
from tests import segment_restatement as R

f32 = np.float32
SUB = f32(2.0 ** -149)                                          # the smallest subnormal
# where a record's column is to be read back: nothing joins (id = row * W + column), no ground, every node a cluster
ALONE = dict(segment_tan=1e30, ground_first_row=0, ground_last_row=0, small_min_points=1, small_min_rows=1)


def _up(v):
    return np.nextafter(f32(v), f32(np.inf))


def _down(v):
    return np.nextafter(f32(v), f32(-np.inf))


def _run(cfg, probes, what):
    """One call over the probes, each a scan of its own: the device's (class, id, counts) against the restatement's, and per
    probe (classes, ids) as lists."""
    assert all(1 <= len(p) <= 3 for p in probes)
    clouds = [R.cloud_of(p) for p in probes]
    fx = K.fx_for(16, 64, len(clouds))
    d = S.device_batch(fx, clouds)
    got = S.numpy_of(fx.segment(cfg, stream=K.stream()))
    fx.close()
    del d
    S.same(got, R.segment_batch(cfg, clouds), what)
    begin = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    return [(got[0][begin[k]:begin[k + 1]].tolist(), got[1][begin[k]:begin[k + 1]].tolist()) for k in range(len(clouds))]


# --- the column boundaries -----------------------------------------------------------------------------------------------------
def _four_column_cases():
    """((x, y), column) for W = 4: test_column_boundaries' 16 pairs and x = +-1 with the smallest subnormal of either sign
    as y -- a flushed y is +-0.0, which opens the upper half."""
    t = 1e-30
    cases = [((1, t), 2), ((1, -t), 1), ((1, 0.0), 2), ((1, -0.0), 2), ((-1, 0.0), 3), ((-1, -0.0), 3), ((-1, -t), 0), ((-1, t), 3),
             ((1e-3, 1), 2), ((-1e-3, 1), 3), ((1e-3, -1), 1), ((-1e-3, -1), 0), ((5, 5), 2), ((-5, 5), 3), ((-5, -5), 0), ((5, -5), 1)]
    cases += [((1, SUB), 2), ((1, -SUB), 1), ((-1, SUB), 3), ((-1, -SUB), 0)]
    return cases


def _boundary_columns(W):
    return [0, 1, W // 4, W // 2 - 1, W // 2, W // 2 + 1, 3 * W // 4, W - 1]


def _boundary_records(cfg):
    """{m: five (x, y)}: the record 10 m out along the table's direction m -- the lower edge of column m -- its two float
    neighbours in y and its two float neighbours in x."""
    cs, sn, _ = R.segment_tables(cfg)
    out = {}
    for m in _boundary_columns(int(cfg.n_columns)):
        x, y = f32(10.0 * cs[m]), f32(10.0 * sn[m])
        out[m] = [(x, y), (x, _down(y)), (x, _up(y)), (_down(x), y), (_up(x), y)]
    return out


def _zero_cross_records(cfg):
    """[(m, x, y)]: records on the four diagonal directions of the table whose cross with that direction is 0.0 exactly --
    just under 8 sqrt(2) m both products round to the same double -- so that `cross >= 0` and `cross > 0` part there."""
    cs, sn, _ = R.segment_tables(cfg)
    W = int(cfg.n_columns)
    out = []
    for m in (W // 8, 3 * W // 8, 5 * W // 8, 7 * W // 8):
        for v in (11.313756, 11.313758, 11.31376):
            x, y = f32(np.sign(cs[m]) * v), f32(np.sign(sn[m]) * v)
            assert cs[m] * float(y) - sn[m] * float(x) == 0.0 and abs(cs[m]) != abs(sn[m]), (m, x, y)
            out.append((m, x, y))
    return out


def _sign_records(W):
    """What decides between the columns W - 1 and 0: the bisection never asks for cross(0), the sign of y does."""
    return [(f32(-10.0), f32(0.0)), (f32(-10.0), f32(-0.0)), (f32(-10.0), SUB), (f32(-10.0), -SUB)]


@pytest.mark.parametrize("W", [64, 4096])
def test_the_probes_straddle_their_boundaries(W):
    """(no device) For every direction m of the table but 0 the five records do not all land in one column.  Direction 0 is
    the seam at -pi: between the columns W - 1 and 0 the header lets the sign of y decide (m0), and cross(0) is never
    evaluated, so the five records there, whose y is the float of 10 sin(-pi) = -1.2e-15, are all in column 0; the seam is
    straddled by the four records of _sign_records instead, y = +-0.0 and the subnormals."""
    cfg = R.config(n_rows=1, n_columns=W, min_range=0.5, **ALONE)
    for m, recs in _boundary_records(cfg).items():
        cols = R.columns(cfg, [r[0] for r in recs], [r[1] for r in recs]).tolist()
        print("W = %d, m = %d: columns %s" % (W, m, cols))
        assert set(cols) <= {(m - 1) % W, m}, (m, cols)
        if m == 0:
            assert recs[0][1] < 0 and set(cols) == {0}
        else:
            assert len(set(cols)) == 2, (m, cols)
    sign = _sign_records(W)
    assert R.columns(cfg, [r[0] for r in sign], [r[1] for r in sign]).tolist() == [W - 1, W - 1, W - 1, 0]
    zero = _zero_cross_records(cfg)
    assert R.columns(cfg, [r[1] for r in zero], [r[2] for r in zero]).tolist() == [r[0] for r in zero]


@pytest.mark.gpu
def test_column_boundaries_of_four_columns():
    """The 20 pairs, and the same 20 seven times as far out (another range, the same column): 40 probes of one record."""
    cfg = R.config(n_rows=1, n_columns=4, min_range=0.5, **ALONE)
    cases = _four_column_cases()
    want = [c[1] for c in cases] * 2
    probes = [[(f32(x), f32(y), f32(0.0), 0)] for (x, y), _ in cases]
    probes += [[(f32(7.0) * f32(x), f32(7.0) * f32(y), f32(0.0), 0)] for (x, y), _ in cases]
    assert probes[36][0][1] == f32(7.0) * SUB != 0.0
    xy = np.array([p[0][:2] for p in probes], np.float32)
    assert R.columns(cfg, xy[:, 0], xy[:, 1]).tolist() == want
    got = _run(cfg, probes, "W = 4")
    assert [g[0] for g in got] == [[R.SEGMENT]] * 40
    assert [g[1][0] for g in got] == want, [(k, g[1][0], w) for k, (g, w) in enumerate(zip(got, want)) if g[1][0] != w]


@pytest.mark.gpu
@pytest.mark.parametrize("W", [64, 4096])
def test_column_boundaries_of_the_tables_directions(W):
    """Eight directions of the table, each with its four float neighbours, the four records that the sign of y sorts at the
    seam, and twelve records whose cross with a diagonal direction is 0.0 exactly (they belong to that direction's column):
    56 probes of one record.  The id read back is the column."""
    cfg = R.config(n_rows=1, n_columns=W, min_range=0.5, **ALONE)
    zero = _zero_cross_records(cfg)
    records = [r for recs in _boundary_records(cfg).values() for r in recs] + _sign_records(W) + [r[1:] for r in zero]
    probes = [[(x, y, f32(0.0), 0)] for x, y in records]
    want = R.columns(cfg, [r[0] for r in records], [r[1] for r in records]).tolist()
    got = _run(cfg, probes, W)
    assert [g[0] for g in got] == [[R.SEGMENT]] * len(probes)
    assert [g[1][0] for g in got] == want
    assert want[40:44] == [W - 1, W - 1, W - 1, 0] and want[44:] == [r[0] for r in zero] and want[20:25].count(W // 2) >= 1 and want[20:25].count(W // 2 - 1) >= 1


# --- the range gates -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_range_gates():
    """y = z = 0: r is x exactly.  min_range is kept and the float below it is not; max_range is not kept and the float
    below it is; a record on the z axis has no azimuth.  The defaults' 1 and 100 m, on +x and on -x, padded to 32 probes."""
    lo, hi = 1.0, 100.0
    probes = [[(f32(lo), f32(0), f32(0), 0)], [(_down(lo), f32(0), f32(0), 0)], [(f32(hi), f32(0), f32(0), 0)], [(_down(hi), f32(0), f32(0), 0)],
              [(f32(0), f32(0), f32(5), 0)], [(f32(-lo), f32(0), f32(0), 0)], [(_up(-lo), f32(0), f32(0), 0)], [(f32(-hi), f32(0), f32(0), 0)],
              [(_up(-hi), f32(0), f32(0), 0)], [(f32(0), f32(-0.0), f32(-5), 0)]]
    want = [(R.SEGMENT, 2), (R.NONE, R.NO_ID), (R.NONE, R.NO_ID), (R.SEGMENT, 2), (R.NONE, R.NO_ID),
            (R.SEGMENT, 3), (R.NONE, R.NO_ID), (R.NONE, R.NO_ID), (R.SEGMENT, 3), (R.NONE, R.NO_ID)]
    # (three records to a probe: the gates with a kept record on either side of them, each in a column of its own)
    probes.append([(f32(1.0), f32(0), f32(0), 0), (f32(0), _down(1.0), f32(0), 0), (f32(0), f32(-100.0), f32(0), 0)])
    while len(probes) < 32:
        k = len(probes)
        probes.append([(f32(0), f32(1.0 + k), f32(0), 0), (f32(0), f32(0), f32(k), 0)])
    cfg = R.config(n_rows=1, n_columns=4, **ALONE)
    assert (float(cfg.min_range), float(cfg.max_range)) == (1.0, 100.0)
    got = _run(cfg, probes, "gates")
    assert [(g[0][0], g[1][0]) for g in got[:10]] == want
    assert got[10][0] == [R.SEGMENT, R.NONE, R.NONE]
    assert all(g[0] == [R.SEGMENT, R.NONE] for g in got[11:])


@pytest.mark.gpu
def test_range_gates_of_another_config():
    """The same gates at min_range 2.5 and max_range 40 (floats that are exact), with z carrying the range: (0, 1.5, 2) has
    r = 2.5 exactly."""
    cfg = R.config(n_rows=1, n_columns=4, min_range=2.5, max_range=40.0, **ALONE)
    probes = [[(f32(2.5), f32(0), f32(0), 0)], [(_down(2.5), f32(0), f32(0), 0)], [(f32(40), f32(0), f32(0), 0)], [(_down(40), f32(0), f32(0), 0)],
              [(f32(0), f32(1.5), f32(2), 0)], [(f32(0), f32(1.5), _down(2), 0)], [(f32(0), f32(24), f32(32), 0)], [(f32(0), f32(24), _down(32), 0)]]
    got = _run(cfg, probes, "gates 2.5 .. 40")
    assert [g[0][0] for g in got] == [R.SEGMENT, R.NONE, R.NONE, R.SEGMENT, R.SEGMENT, R.NONE, R.NONE, R.SEGMENT]


# --- two records in one cell ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_tie_in_one_cell_shows_in_the_classes():
    """H = 2, W = 4, ground_tan = 0.5.  A and B share cell (0, 2), 3 m out with z = +0.5 and -0.5: r is equal in double and
    in float, the lower index wins.  C is in (1, 2), 5 m out with z = 1.5.  A first: dz = 1, dx = 2, 1 <= 0.25 * 4 -- all
    three are ground.  B first: dz = 2 -- none is, and nothing joins: all three are clutter.  Then A at z = 0 and B at
    z = -1e-6, whose r differ in double and are equal in float, with C at z = 1: A first gives dz = 1 (ground), B first a
    dz above 1 (clutter) -- a key of the double's bits would let A win both times.  And test_two_records_in_one_cell's pair
    in both orders."""
    cfg = R.config(n_rows=2, n_columns=4, ground_tan=0.5, ground_first_row=0, ground_last_row=1)
    A, B, Cc = (f32(3), f32(0), f32(0.5), 0), (f32(3), f32(0), f32(-0.5), 0), (f32(5), f32(0), f32(1.5), 1)
    A2, B2, C2 = (f32(3), f32(0), f32(0), 0), (f32(3), f32(0), f32(-1e-6), 0), (f32(5), f32(0), f32(1), 1)
    c = R.cloud_of([A2, B2])
    keep, cell, r = R.project(cfg, c["x"], c["y"], c["z"], R.rows_of(c))
    assert keep.all() and cell[0] == cell[1] == 2 and r[0] < r[1] and f32(r[0]) == f32(r[1])
    probes = [[A, B, Cc], [B, A, Cc], [Cc, A, B], [Cc, B, A], [A2, B2, C2], [B2, A2, C2], [C2, A2, B2], [C2, B2, A2]]
    got = _run(cfg, probes, "tie")
    G, Cl = R.GROUND, R.CLUTTER
    assert [g[0] for g in got] == [[G] * 3, [Cl] * 3, [G] * 3, [Cl] * 3] * 2
    assert [g[1] for g in got[:2]] == [[R.NO_ID] * 3, [2, 2, 6]]
    one = R.config(n_rows=1, n_columns=64, ground_last_row=0, small_min_points=2, small_min_rows=1)
    a = R.centre_record(one, 0, 10, 10.0)
    b = (a[0], a[1], f32(1e-6), 0)
    side = R.centre_record(one, 0, 11, 10.2)
    got = _run(one, [[a, b], [b, a], [a, b, side], [b, a, side]], "equal floats of r")
    assert [g[0] for g in got] == [[Cl] * 2, [Cl] * 2, [R.SEGMENT] * 3, [R.SEGMENT] * 3] and got[2][1] == [10, 10, 10]


# --- the ground test at equality -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ground_at_equality():
    """test_ground_at_equality's cases: ground_tan = 0.5 (g2 = 0.25 exactly), dx = 2; dz = 1 passes, one float more does
    not, and the records may come in either order.  Also one float less, and the same with -dz."""
    cfg = R.config(n_rows=2, n_columns=4, ground_first_row=0, ground_last_row=1, ground_tan=0.5)
    low = lambda z=0.0: (f32(3), f32(0), f32(z), 0)
    high = lambda z: (f32(5), f32(0), f32(z), 1)
    probes = [[low(), high(1.0)], [low(), high(_up(1.0))], [high(1.0), low()], [high(_up(1.0)), low()], [low(), high(_down(1.0))],
              [low(), high(-1.0)], [low(), high(_down(-1.0))], [low(1.0), high(0.0)], [low(_up(1.0)), high(0.0)]]
    got = _run(cfg, probes, "ground")
    G, Cl = R.GROUND, R.CLUTTER
    assert [g[0] for g in got] == [[G, G], [Cl, Cl], [G, G], [Cl, Cl], [G, G], [G, G], [Cl, Cl], [G, G], [Cl, Cl]]


# --- the join test at its threshold ---------------------------------------------------------------------------------------------
JOIN = dict(n_rows=2, n_columns=64, ground_first_row=0, ground_last_row=0, small_min_points=2, small_min_rows=1)
PAIRS = {"columns": ((0, 10), (0, 11)), "rows": ((0, 10), (1, 10)), "seam": ((0, 63), (0, 0))}


def _joins(cfg, pair, rb):
    (ra_row, ra_col), (rb_row, rb_col) = pair
    cls = R.segment_cloud(cfg, R.cloud_of([R.centre_record(cfg, ra_row, ra_col, 10.0), R.centre_record(cfg, rb_row, rb_col, float(rb))]))[0].tolist()
    assert cls in ([R.SEGMENT] * 2, [R.CLUTTER] * 2), cls
    return cls[0] == R.SEGMENT


def _bracket(cfg, pair):
    """(rb, the float above it): float32 ranges of the second record, found by bisection on the restatement from 10 m (joins)
    to 11 m (does not); the first still joins the record at 10 m and the second no longer does."""
    lo, hi = int(f32(10.0).view(np.uint32)), int(f32(11.0).view(np.uint32))
    as_float = lambda bits: np.uint32(bits).view(np.float32)
    assert _joins(cfg, pair, as_float(lo)) and not _joins(cfg, pair, as_float(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _joins(cfg, pair, as_float(mid)):
            lo = mid
        else:
            hi = mid
    return as_float(lo), as_float(hi)


def test_the_join_brackets_differ():
    """(no device) One float of the second record's range apart, the restatement joins and does not join."""
    cfg = R.config(**JOIN)
    for name, pair in PAIRS.items():
        rb, above = _bracket(cfg, pair)
        print("%s: joins up to rb = %r (%.9g), not at %.9g" % (name, rb, rb, above))
        assert above == _up(rb) and _joins(cfg, pair, rb) and not _joins(cfg, pair, above)
        assert (1.015 < rb / 10.0 < 1.025) if name == "rows" else (1.045 < rb / 10.0 < 1.06)


@pytest.mark.gpu
def test_join_threshold():
    """W = 64, the default segment_tan: a column pair, a row pair and the seam pair (63, 0), the first record 10 m out and
    the second at the largest float32 range that still joins it and at the next float -- in both orders of the records."""
    cfg = R.config(**JOIN)
    probes, want = [], []
    for name, pair in PAIRS.items():
        a = R.centre_record(cfg, pair[0][0], pair[0][1], 10.0)
        least = min(pair[0][0] * 64 + pair[0][1], pair[1][0] * 64 + pair[1][1])
        for rb, joins in zip(_bracket(cfg, pair), (True, False)):
            b = R.centre_record(cfg, pair[1][0], pair[1][1], float(rb))
            probes += [[a, b], [b, a]]
            ids = [pair[0][0] * 64 + pair[0][1], pair[1][0] * 64 + pair[1][1]]
            want += [([R.SEGMENT] * 2, [least] * 2), ([R.SEGMENT] * 2, [least] * 2)] if joins else [([R.CLUTTER] * 2, ids), ([R.CLUTTER] * 2, ids[::-1])]
    got = _run(cfg, probes, "join")
    assert got == want, [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]


def _equality_config():
    """A config whose row pair meets the join test in powers of two: row_step = 2^-30 (sin = 2^-30 and cos = 1 in double),
    segment_tan = 2^-20.  With y = z = 0 a record's range is |x| exactly."""
    cfg = R.config(n_rows=2, n_columns=4, row_step=2.0 ** -30, segment_tan=2.0 ** -20, ground_first_row=0, ground_last_row=0,
                   small_min_points=2, small_min_rows=1)
    _, _, consts = R.segment_tables(cfg)
    assert consts[2] == 2.0 ** -30 and consts[3] == 1.0 and float(cfg.segment_tan) == 2.0 ** -20
    return cfg


def _equality_probes():
    """d2 = 8, d1 = 8 + 2^-7: d2 sin a = 2^-27 = segment_tan (d1 - d2 cos a), and `>` does not join; one float less of d1
    and it does; one more and it does not.  Either record may be the farther one and come first."""
    at = lambda x, row: (f32(x), f32(0), f32(0), row)
    d1 = f32(8.0078125)
    probes = [[at(8, 0), at(d1, 1)], [at(d1, 1), at(8, 0)], [at(d1, 0), at(8, 1)], [at(8, 0), at(_down(d1), 1)], [at(_down(d1), 0), at(8, 1)],
              [at(8, 0), at(_up(d1), 1)], [at(-8, 0), at(-d1, 1)], [at(-8, 0), at(_up(-d1), 1)]]
    Cl, Sg = [R.CLUTTER] * 2, [R.SEGMENT] * 2
    return probes, [Cl, Cl, Cl, Sg, Sg, Cl, Cl, Sg]


def test_the_join_test_at_equality_on_the_host():
    """(no device) Both sides of the join test are 2^-27, and the restatement says what the header's `>` says."""
    cfg = _equality_config()
    assert R.joined(cfg, np.float64(8.0), np.float64(8.0078125), 2.0 ** -30, 1.0) == False and 8.0 * 2.0 ** -30 == 2.0 ** -20 * (8.0078125 - 8.0)
    assert R.joined(cfg, np.float64(8.0), np.float64(_down(8.0078125)), 2.0 ** -30, 1.0) == True
    probes, want = _equality_probes()
    assert [R.segment_cloud(cfg, R.cloud_of(p))[0].tolist() for p in probes] == want


@pytest.mark.gpu
def test_join_at_equality():
    """The join test with both of its sides equal (2^-27): not joined, as the header's `>` has it."""
    probes, want = _equality_probes()
    got = _run(_equality_config(), probes, "join at equality")
    assert [g[0] for g in got] == want
    assert got[0][1] == [2, 6] and got[3][1] == [2, 2] and got[6][1] == [3, 7]
