"""lfx_place_db on the device (include/lfx.h, the place recognition section) against the numpy restatement
(tests/scan_context_restatement.py): distances, shifts, yaws and the order of the matches byte-equal, on both sides of the
comparison kernel's pass (floor(256 / S) entries: 4 at S = 60, and the tile of a small index) and of its largest tile (64
entries), with duplicates, all-zero descriptors and empty columns; ranges, k above the range's size, adds in parts, the capacity, download."""
import ctypes as C

import numpy as np
import pytest

from tests import deskew_cases as K
from tests import scan_context_restatement as R

pytestmark = pytest.mark.gpu

_POOL = {}


def _descriptors(rng, n, shape):
    """n descriptors: heights in [0, 5), a tenth of the cells and two runs of columns empty."""
    d = rng.uniform(0.0, 5.0, (n,) + shape).astype(np.float32)
    d[rng.uniform(0, 1, d.shape) < 0.1] = 0.0
    S = shape[1]
    for e in range(n):
        a, b = rng.integers(0, S, 2)
        d[e, :, a:a + max(1, S // 15)] = 0.0
        d[e, :, b:b + 1] = 0.0
    return d


def _pool(shape=(20, 60), n=257):
    """The entries, three queries, and the restatement's (distance, shift) of every pair -- made once per shape."""
    if shape not in _POOL:
        rng = np.random.default_rng(shape[0] * 1000 + shape[1])
        pool = _descriptors(rng, n, shape)
        pool[min(10, n - 1)] = pool[3]                                  # duplicates
        pool[min(100, n - 2)] = pool[3]
        pool[min(20, n - 3)] = 0.0                                      # an all-zero entry: distance 1 to everything
        queries = np.stack([np.roll(pool[3], -7 % shape[1], axis=1), np.zeros(shape, np.float32), _descriptors(rng, 1, shape)[0]])
        best = []
        for q in queries:
            d = R.shift_distances(q, pool)
            shift = np.argmin(d, axis=1)
            best.append((d[np.arange(n), shift], shift))
        _POOL[shape] = (pool, queries, best)
    return _POOL[shape]


def _want(best, S, k, first, count):
    """The restatement's matches of one query for entries [first, first + count)."""
    dist, shift = best[0][first:first + count], best[1][first:first + count]
    out = [(first + int(e), int(shift[e]), float(dist[e]), R.yaw_of_shift(int(shift[e]), S)) for e in np.lexsort((np.arange(count), dist))[:k]]
    return out + [(0xFFFFFFFF, 0, float("inf"), 0.0)] * (k - len(out))


def _tuples(raw, n):
    return [(int(m.entry), int(m.shift), float(m.distance), float(m.yaw)) for m in raw[:n]]


def _check(db, d_queries, which, best, k, first=0, count=None):
    """The device's matches of queries `which` equal the restatement's, bit for bit (floats compared as floats: no NaN here)."""
    S = db.shape[1]
    count = len(db) - first if count is None else count
    raw = db.query_raw(d_queries[which[0]:], len(which), k, first, count, K.stream())
    got = _tuples(raw, len(which) * k)
    for i, q in enumerate(which):
        want = _want(best[q], S, k, first, count)
        assert got[i * k:(i + 1) * k] == want, (q, k, first, count, got[i * k:(i + 1) * k][:3], want[:3])
    return bytes(raw)[:C.sizeof(raw[0]) * len(which) * k]


@pytest.mark.parametrize("entries", [1, 3, 4, 5, 63, 64, 65, 257])
def test_matches_equal_the_restatement(entries):
    """1 and 3 queries with k = 1, 4, 16 against the first `entries` descriptors of the pool: the duplicate entries come by
    the lower index, the all-zero entry and the all-zero query have distance 1, a rolled copy of an entry finds it with the
    roll as shift and a distance within rounding of 0."""
    import torch
    pool, queries, best = _pool()
    fx = K.fx_for(16, 900, 1)
    db = fx.place_db(entries)
    db.add(torch.from_numpy(pool[:entries]).to(K.dev()), entries, K.stream())
    assert len(db) == entries
    d_q = torch.from_numpy(queries).to(K.dev())
    for k in (1, 4, 16):
        alone = [_check(db, d_q, [q], best, k) for q in range(3)]
        together = _check(db, d_q, [0, 1, 2], best, k)
        assert together == b"".join(alone)                              # a query is the same bytes alone and in a batch
    top = db.query(d_q, 3, 4, stream=K.stream())
    if entries > 3:
        assert top[0][0]["entry"] == 3 and top[0][0]["shift"] == 7 and abs(top[0][0]["distance"]) < 1e-15
        assert top[0][0]["yaw"] == pytest.approx(np.deg2rad(42.0), abs=1e-12)
    if entries > 100:
        assert [m["entry"] for m in top[0][:3]] == [3, 10, 100]
    assert all(m["distance"] == 1.0 and m["shift"] == 0 for m in top[1] if m["entry"] is not None)
    assert [m["entry"] for m in top[1]] == [e if e < entries else None for e in range(4)]
    if entries > 20:
        far = db.query(d_q, 3, 16, first=20, count=1, stream=K.stream())
        assert all(f[0]["entry"] == 20 and f[0]["distance"] == 1.0 and f[1]["entry"] is None for f in far)
    db.close()
    fx.close()


@pytest.mark.parametrize("shape,entries", [((1, 4), 70), ((40, 120), 5), ((7, 18), 40)], ids=["1x4", "40x120", "7x18"])
def test_other_grids(shape, entries):
    """The smallest grid (64 entries to a pass), the largest (two to a pass, the most LDS) and an odd one."""
    import torch
    pool, queries, best = _pool(shape, entries)
    fx = K.fx_for(16, 900, 1)
    db = fx.place_db(entries, dict(n_rings=shape[0], n_sectors=shape[1]))
    db.add(torch.from_numpy(pool).to(K.dev()), entries, K.stream())
    d_q = torch.from_numpy(queries).to(K.dev())
    for k in (1, 16):
        _check(db, d_q, [0, 1, 2], best, k)
    db.close()
    fx.close()


def test_tiles_of_several_passes():
    """An index large enough for the comparison kernel to give a workgroup two and four passes of entries (7 x 18: 14 entries
    to a pass; 16 and 32 queries against 3 600 entries are 57 600 and 115 200 pairs): every query's 16 best as the restatement
    has them, and the same bytes whichever the tile."""
    import torch
    shape, entries = (7, 18), 3600
    rng = np.random.default_rng(77)
    pool, queries = _descriptors(rng, entries, shape), _descriptors(rng, 32, shape)
    pool[1234] = pool[17]
    queries[5] = np.roll(pool[17], -3, axis=1)
    fx = K.fx_for(16, 900, 1)
    db = fx.place_db(entries, dict(n_rings=shape[0], n_sectors=shape[1]))
    db.add_host(pool, K.stream())
    d_q = torch.from_numpy(queries).to(K.dev())
    want = [[(0xFFFFFFFF if e is None else e, s, d, y) for e, s, d, y in R.query(q, pool, 16)] for q in queries]
    got = {}
    for n in (1, 16, 32):
        got[n] = _tuples(db.query_raw(d_q, n, 16, 0, entries, K.stream()), n * 16)
        assert got[n] == [m for w in want[:n] for m in w], n
    assert [m[0] for m in got[32][5 * 16:5 * 16 + 2]] == [17, 1234] and got[32][5 * 16][1] == 3
    db.close()
    fx.close()


def test_ranges_parts_capacity_and_download():
    """first / count ranges (an empty one, one entry, one across a tile's edge), k above the range's size; an add in two
    parts and from the host equals an add in one; an add past the capacity is LFX_ERR_CAPACITY and leaves size and answers as
    they were; download returns what was added; what the calls refuse."""
    import torch
    from lidar_feature_extraction_amd import binding as B
    pool, queries, best = _pool()
    n = 130
    fx = K.fx_for(16, 900, 1)
    d_pool = torch.from_numpy(pool[:n]).to(K.dev())
    d_q = torch.from_numpy(queries).to(K.dev())
    whole, parts = fx.place_db(n), fx.place_db(n + 2)
    whole.add(d_pool, n, K.stream())
    parts.add(d_pool, 50, K.stream())
    parts.add_host(pool[50:97], K.stream())
    parts.add(d_pool[97:], n - 97, K.stream())
    parts.add(d_pool, 0, K.stream())                                    # (nothing: fine)
    assert len(parts) == n == len(whole)
    assert parts.download(0, n, K.stream()).tobytes() == pool[:n].tobytes() == whole.download(stream=K.stream()).tobytes()
    assert parts.download(60, 3, K.stream()).tobytes() == pool[60:63].tobytes() and parts.download(n, 0).shape == (0, 20, 60)
    for first, count in ((0, 0), (n, 0), (5, 1), (60, 10), (1, n - 1), (0, n)):
        for k in (1, 16):
            a = _check(whole, d_q, [0, 1, 2], best, k, first, count)
            assert a == _check(parts, d_q, [0, 1, 2], best, k, first, count)
    before = _check(parts, d_q, [0, 1, 2], best, 16)
    with pytest.raises(B.LfxError) as e:
        parts.add(d_pool, 3, K.stream())                                # two places left
    assert e.value.code == B.ERR_CAPACITY
    with pytest.raises(B.LfxError) as e:
        parts.add_host(pool[:3], K.stream())
    assert e.value.code == B.ERR_CAPACITY
    assert len(parts) == n and _check(parts, d_q, [0, 1, 2], best, 16) == before
    parts.add(d_pool, 2, K.stream())                                    # ... which can still be taken
    assert len(parts) == n + 2 and parts.download(n, 2, K.stream()).tobytes() == pool[:2].tobytes()

    def refused(call):
        with pytest.raises(B.LfxError) as err:
            call()
        assert err.value.code == B.ERR_INVALID_ARGUMENT, err.value

    refused(lambda: whole.query(d_q, 1, 0))                             # k outside 1 .. 16
    refused(lambda: whole.query(d_q, 1, 17))
    refused(lambda: whole.query(d_q, 0, 1))                             # no query
    refused(lambda: whole.query(d_q, 1, 1, first=n + 1, count=0))       # a range past the size
    refused(lambda: whole.query(d_q, 1, 1, first=n - 1, count=2))
    refused(lambda: whole.query(d_q, 1, 1, first=1, count=0xFFFFFFFF))
    refused(lambda: whole.download(n - 1, 2))
    refused(lambda: fx.place_db(0))
    refused(lambda: fx.place_db(4, dict(n_sectors=61)))
    refused(lambda: fx.place_db(4, dict(n_rings=41)))
    L = B.load()
    res = (B.PlaceMatch * 16)()
    assert L.lfx_place_db_query(fx._ctx, whole.handle, None, 1, 0, n, 1, res, None) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_place_db_query(fx._ctx, whole.handle, C.c_void_p(d_q.data_ptr()), 1, 0, n, 1, None, None) == B.ERR_INVALID_ARGUMENT
    assert L.lfx_place_db_add(fx._ctx, whole.handle, None, 1, None) == B.ERR_INVALID_ARGUMENT
    assert _check(whole, d_q, [0, 1, 2], best, 16, 0, n)
    whole.close()
    parts.close()
    fx.close()
