"""lfx_place_db_query_gated on the device (include/lfx.h, the place recognition section) against the numpy restatement
(tests/loop_closer_restatement.py over tests/scan_context_restatement.py): every match byte for byte and n_eligible equal --
index sizes on both sides of the comparison kernel's pass (4 entries at S = 60), of a wave's ballot (64), of a round of the
gate kernel (256) and, in a case of its own at R = 2, S = 4, of its step (2 048 entries: the count carried from step to
step), with enough queries in one call for a workgroup of the gated comparison to take several tiles; gates that leave
none, one, a pass less one, a pass, a pass and one, every third, only the last and all entries eligible; limits 0, 1 and n; several queries with their own limits and poses in one call; k above the eligible
entries; duplicates; the other grids; the position test at equality; a query without a pose among gated ones; the ungated
query's bytes where nothing is gated; what the call refuses; and an add on one stream with the query on another."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import deskew_cases as K
from tests import loop_closer_cases as LC
from tests import loop_closer_restatement as LR
from tests import segment_cases as S
from tests.test_place_db_gpu import _pool

pytestmark = pytest.mark.gpu


def _tuples(raw, n):
    return [(int(m.entry), int(m.shift), float(m.distance), float(m.yaw)) for m in raw[:n]]


def _poses(translations):
    """[n][3][4] poses with the identity as rotation"""
    t = np.asarray(translations, np.float64).reshape(-1, 3)
    p = np.zeros((len(t), 3, 4))
    p[:, 0, 0] = p[:, 1, 1] = p[:, 2, 2] = 1.0
    p[:, :, 3] = t
    return p


def _near(n, chosen):
    """Poses of n entries and, as pose n, the query's at the origin: the chosen entries 1 m from it, the others 10 m."""
    t = np.zeros((n + 1, 3))
    t[:n, 0] = 10.0
    t[:n, 1] = np.arange(n) * 0.001                                     # (no two entries at one spot)
    t[list(chosen), 0] = 1.0
    return _poses(t)


def _check(db, d_q, which, best, gates, poses, radius, k):
    """The device's matches and counts of queries `which` (gates[i] for which[i]) equal the restatement's."""
    import torch
    d_poses = None if poses is None else torch.from_numpy(poses).to(K.dev())
    raw, n_eligible = db.query_gated_raw(d_q[which[0]:], gates, 0 if poses is None else d_poses, radius, k, K.stream())
    want, counts = LR.query_gated(None, np.zeros((len(db),) + db.shape, np.float32), gates, poses, radius, k, [best[q] for q in which])
    got = _tuples(raw, len(gates) * k)
    assert [int(c) for c in n_eligible] == counts, (gates, n_eligible, counts)
    for i in range(len(gates)):
        assert got[i * k:(i + 1) * k] == want[i], (gates[i], k, got[i * k:(i + 1) * k][:3], want[i][:3])
    return bytes(raw)[:C.sizeof(raw[0]) * len(gates) * k]


@pytest.mark.parametrize("entries", [1, 3, 4, 5, 63, 64, 65, 255, 256, 257])
def test_gated_matches_equal_the_restatement(entries):
    """R = 20, S = 60 against the first `entries` descriptors of test_place_db_gpu's pool (duplicates at 3, 10 and 100, an
    all-zero entry at 20)."""
    import torch
    pool, queries, best = _pool()
    n = entries
    fx = K.fx_for(16, 900, 1)
    db = fx.place_db(n)
    db.add(torch.from_numpy(pool[:n]).to(K.dev()), n, K.stream())
    d_q = torch.from_numpy(queries).to(K.dev())
    sets = {"none": [], "one": [n // 2], "three": range(min(3, n)), "four": range(max(n - 4, 0), n), "five": range(min(5, n)),
            "all": range(n), "third": range(0, n, 3), "last": [n - 1], "ties": [e for e in (3, 10, 100) if e < n]}
    for name, chosen in sets.items():
        poses = _near(n, chosen)
        for k in (1, 16):
            for q in range(3):
                _check(db, d_q, [q], best, [(n, n)], poses, 2.0, k)
    # limits without a position test, and with one that passes everything
    everywhere = _near(n, range(n))
    for limit in (0, 1, n):
        for k in (1, 16):
            _check(db, d_q, [0], best, [(limit, None)], None, math.inf, k)
            _check(db, d_q, [2], best, [(limit, n)], everywhere, math.inf, k)
    # 2 and 5 queries (the three queries, then the first two again: d_q is extended) with their own limits and poses
    d_q5 = torch.cat([d_q, d_q[:2]])
    best5 = best + best[:2]
    line = np.zeros((n + 5, 3))
    line[:n, 0] = np.arange(n)                                          # entry e at x = e; five query poses along the line
    line[n:, 0] = [0.0, n / 2.0, n - 1.0, n / 3.0, 2.0]
    poses = _poses(line)
    gates = [(n, n), (max(n - 1, 0), n + 1), (n, n + 2), (min(n, 7), n + 3), (n // 2, n + 4)]
    for k in (1, 16):
        alone = [_check(db, d_q5, [q], best5, [gates[q]], poses, 2.5, k) for q in range(5)]
        assert _check(db, d_q5, [0, 1], best5, gates[:2], poses, 2.5, k) == b"".join(alone[:2])
        assert _check(db, d_q5, [0, 1, 2, 3, 4], best5, gates, poses, 2.5, k) == b"".join(alone)
    if n > 100:
        top, _ = db.query_gated(d_q, [(n, n)], torch.from_numpy(_near(n, [100, 3, 10, 50])).to(K.dev()), 2.0, 4, K.stream())
        assert [m["entry"] for m in top[0][:3]] == [3, 10, 100] and top[0][0]["shift"] == 7   # the tie goes to the lower entry
    db.close()
    fx.close()


@pytest.mark.parametrize("shape,entries", [((1, 4), 70), ((40, 120), 5)], ids=["1x4", "40x120"])
def test_gated_other_grids(shape, entries):
    """R = 1 with S = 4 (64 entries to a pass) and R = 40 with S = 120 (two to a pass, the most LDS)."""
    import torch
    pool, queries, best = _pool(shape, entries)
    n = entries
    fx = K.fx_for(16, 900, 1)
    db = fx.place_db(n, dict(n_rings=shape[0], n_sectors=shape[1]))
    db.add(torch.from_numpy(pool).to(K.dev()), n, K.stream())
    d_q = torch.from_numpy(queries).to(K.dev())
    for chosen in ([], range(n), range(0, n, 3), [n - 1], range(min(3, n))):
        poses = _near(n, chosen)
        for k in (1, 16):
            _check(db, d_q, [0, 1, 2], best, [(n, n), (n - 1, n), (n, None)], poses, 2.0, k)
    db.close()
    fx.close()


@pytest.mark.parametrize("entries", [2047, 2048, 2049, 4100])
def test_gate_steps_and_comparison_trips(entries):
    """R = 2, S = 4 (64 entries to a pass; two rings, so that distances differ: with one ring every pair of occupied columns
    has the cosine 1), index sizes on both sides of the gate kernel's step of 2 048 entries and one of
    three steps, 300 queries in one call: with poses the comparison's grid is capped at 8192 / 300 = 27 workgroups a query,
    so a list of more than 27 x 64 = 1 728 slots gives workgroups two and three tiles each.  Entry e lies at x = e; every
    query has a limit and a pose of its own (every 11th none).  Dense: a radius that passes every entry (lists of up to 4 100
    slots).  Sparse: radius 100.5, lists of up to 201 entries that begin anywhere, many across a step's edge."""
    import torch
    n, n_queries, shape = entries, 300, (2, 4)
    rng = np.random.default_rng(n)
    pool = rng.uniform(0.5, 5.0, (n,) + shape).astype(np.float32)
    pool[rng.uniform(0, 1, pool.shape) < 0.1] = 0.0
    pool[7] = np.array([[1.0, 2.0, 3.0, 4.0], [4.0, 2.5, 1.0, 3.0]], np.float32)
    pool[n - 1] = pool[n // 2] = pool[7]                                # duplicates on both sides of a step
    queries = rng.uniform(0.5, 5.0, (n_queries,) + shape).astype(np.float32)
    queries[3] = np.roll(pool[7], -1, axis=1)
    best = [LR.best_of(q, pool) for q in queries]
    line = np.zeros((n + n_queries, 3))
    line[:n, 0] = np.arange(n)
    line[n:, 0] = rng.integers(0, n, n_queries)
    line[n + 3, 0] = 2048.0 if n > 2048 else n - 1.0
    poses = _poses(line)
    gates = [(n - (j % 7) * (n // 40), None if j % 11 == 10 else n + j) for j in range(n_queries)]
    fx = K.fx_for(16, 900, 1)
    db = fx.place_db(n, dict(n_rings=shape[0], n_sectors=shape[1]))
    db.add(torch.from_numpy(pool).to(K.dev()), n, K.stream())
    d_q, d_poses = torch.from_numpy(queries).to(K.dev()), torch.from_numpy(poses).to(K.dev())
    for radius, shortest, longest in ((1e9, n, n), (100.5, 101, 201)):
        for k in (1, 16):
            raw, n_eligible = db.query_gated_raw(d_q, gates, d_poses, radius, k, K.stream())
            want, counts = LR.query_gated(None, pool, gates, poses, radius, k, best)
            assert [int(c) for c in n_eligible] == counts
            assert shortest <= max(c for c, g in zip(counts, gates) if g[1] is not None) <= longest   # (the queries with a pose)
            got = _tuples(raw, n_queries * k)
            for j in range(n_queries):
                assert got[j * k:(j + 1) * k] == want[j], (radius, k, j, gates[j], got[j * k:(j + 1) * k][:2], want[j][:2])
    top, _ = db.query_gated(d_q[3:], [(n, n + 3)], d_poses, 1e9, 3, K.stream())
    assert [m["entry"] for m in top[0]] == [7, n // 2, n - 1] and top[0][0]["shift"] == 1
    db.close()
    fx.close()


def test_position_test_at_equality_and_without_a_pose():
    """Entries at (3, 4, 0) and (0, 3, 4) from the query's pose: radius 5.0 keeps them, the double below 5 drops them, +inf
    keeps every entry; a query without a pose in a call that gates the others takes every entry below its limit."""
    import torch
    pool, queries, best = _pool()
    n = 6
    fx = K.fx_for(16, 900, 1)
    db = fx.place_db(n)
    db.add(torch.from_numpy(pool[:n]).to(K.dev()), n, K.stream())
    d_q = torch.from_numpy(queries).to(K.dev())
    base = np.array([100.0, -50.0, 7.0])
    t = np.array([[3, 4, 0], [0, 3, 4], [30, 40, 0], [0, 0, 0], [3, 4, 1e-7], [-3, 0, -4], [0, 0, 0]], np.float64) + base
    poses = _poses(t)                                                   # (pose 6: the query's)
    d_poses = torch.from_numpy(poses).to(K.dev())
    for radius, want in ((5.0, [0, 1, 3, 5]), (float(np.nextafter(5.0, 0.0)), [3]), (math.inf, [0, 1, 2, 3, 4, 5]), (0.0, [3])):
        assert list(LR.eligible(n, n, 6, poses, radius)) == want
        got, counts = db.query_gated(d_q, [(n, 6)], d_poses, radius, 16, K.stream())
        assert counts == [len(want)] and sorted(m["entry"] for m in got[0] if m["entry"] is not None) == want, (radius, got[0], counts)
        _check(db, d_q, [0, 1, 2], best, [(n, 6), (n, None), (3, 6)], poses, radius, 16)
    db.close()
    fx.close()


def test_gate_hand_cases_on_the_device():
    """tests/loop_closer_cases.py's hand cases of the gate (a pose that is not finite among them): the eligible entries are the
    ones written down there."""
    import torch
    pool, queries, best = _pool()
    fx = K.fx_for(16, 900, 1)
    db = fx.place_db(4)
    db.add(torch.from_numpy(pool[:4]).to(K.dev()), 4, K.stream())
    d_q = torch.from_numpy(queries).to(K.dev())
    for translations, radius, want in LC.GATE_CASES:
        n = len(translations) - 1
        poses = _poses(translations)
        got, counts = db.query_gated(d_q, [(n, n)], torch.from_numpy(poses).to(K.dev()), radius, 16, K.stream())
        assert counts == [len(want)] and sorted(m["entry"] for m in got[0] if m["entry"] is not None) == want, (translations, radius, got[0])
        _check(db, d_q, [0], best, [(n, n)], poses, radius, 16)
    db.close()
    fx.close()


def test_ungated_bytes_refusals_and_the_other_stream():
    """With d_poses NULL and limit = n the bytes are lfx_place_db_query(first = 0, count = n)'s; every refusal of the header is
    returned with the index unchanged; an add on a held stream and the gated query on another: ordered behind the add."""
    import torch
    from lidar_feature_extraction_amd import binding as B
    pool, queries, best = _pool()
    n = 130
    fx = K.fx_for(16, 900, 1)
    db = fx.place_db(n + 4)
    d_pool = torch.from_numpy(pool[:n + 4]).to(K.dev())
    db.add(d_pool, n, K.stream())
    d_q = torch.from_numpy(queries).to(K.dev())
    size = C.sizeof(B.PlaceMatch)
    for k in (1, 16):
        plain = bytes(db.query_raw(d_q, 3, k, 0, n, K.stream()))[:size * 3 * k]
        gated, counts = db.query_gated_raw(d_q, [(n, None)] * 3, 0, math.inf, k, K.stream())
        assert bytes(gated)[:size * 3 * k] == plain and list(counts) == [n] * 3
    before = bytes(db.query_raw(d_q, 3, 16, 0, n, K.stream()))
    d_poses = torch.from_numpy(_near(n, range(n))).to(K.dev())
    L = B.load()
    res, gates, elig = (B.PlaceMatch * 64)(), (B.PlaceGate * 4)(*[B.PlaceGate(n, n)] * 4), (C.c_uint32 * 4)()
    vp = C.c_void_p

    def call(ctx=fx._ctx, handle=db.handle, desc=d_q.data_ptr(), n_queries=1, g=gates, radius=2.0, k=1, matches=res):
        return L.lfx_place_db_query_gated(ctx, handle, vp(desc), n_queries, g, vp(d_poses.data_ptr()), radius, k, matches, elig, vp(K.stream()))

    assert call() == 0
    for refused in (dict(ctx=None), dict(handle=None), dict(desc=None), dict(g=None), dict(matches=None), dict(n_queries=0), dict(n_queries=65536),
                    dict(k=0), dict(k=17), dict(radius=math.nan), dict(radius=-1.0), dict(radius=-math.inf),
                    dict(g=(B.PlaceGate * 1)(B.PlaceGate(n + 1, n))), dict(n_queries=2, g=(B.PlaceGate * 2)(B.PlaceGate(n, n), B.PlaceGate(n + 1, n)))):
        assert call(**refused) == B.ERR_INVALID_ARGUMENT, refused
    assert len(db) == n and bytes(db.query_raw(d_q, 3, 16, 0, n, K.stream())) == before
    # 4 entries added on held A, the gated query at once on B
    hold = S.Hold()
    a, b = S.two_streams()
    poses = _near(n + 4, [n, n + 2, 5])
    d_poses4 = torch.from_numpy(poses).to(K.dev())
    K.sync()
    hold(a)
    db.add(d_pool[n:], 4, a.cuda_stream)
    e = S.event_behind(a)
    hold.still_held(e, "place index: add on A, gated query on B")
    raw, counts = db.query_gated_raw(d_q, [(n + 4, n + 4)] * 3, d_poses4, 2.0, 4, b.cuda_stream)
    want, _ = LR.query_gated(None, pool[:n + 4], [(n + 4, n + 4)] * 3, poses, 2.0, 4, best)
    assert list(counts) == [3] * 3 and _tuples(raw, 12) == [m for w in want for m in w]
    K.sync()
    db.close()
    fx.close()
