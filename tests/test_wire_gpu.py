"""The four packed payloads (lfx_pack_features, lfx_pack_xyz, lfx_pack_xyz12, lfx_pack_colored) on the device against the
numpy restatement of tests/wire_cases.py, bit for bit: the offsets tables around the one-workgroup prefix's chunk
boundaries, a capacity shorter than the payload, and colored_scan on every route a scan can take."""
import numpy as np
import pytest

from tests import wire_cases as W

pytestmark = pytest.mark.gpu

from lidar_feature_extraction_amd import FeatureExtraction, make_scan  # noqa: E402
from lidar_feature_extraction_amd import binding as LB  # noqa: E402

SIZES = [769, 1, 513, 2, 257, 256, 255, 512, 511]


def test_offsets_at_the_chunk_boundaries():
    """feature_offsets_kernel and colored_offsets_kernel are one workgroup of 256 threads that takes ceil(batch / 256) scans
    per thread: batches of 769 (four per thread, the last thread's chunk ragged and most threads past 193 idle), 513, 512,
    511 (two or three per thread), 257, 256, 255 and 1, 2, growing and shrinking on one context.  Every batch starts with
    an empty scan, some end with one or with a scan without a feature (tests/test_wire_expect.py); all four payloads and
    their tables against the restatement after every batch."""
    import torch
    pool = W.pool()
    fx = FeatureExtraction(device=0, max_points_per_scan=W.POOL_RINGS * W.POOL_COLS, max_batch=max(SIZES),
                           max_points_per_ring=W.POOL_COLS, max_rings=W.POOL_RINGS)
    d_content = [torch.from_numpy(c.view(np.uint8).reshape(-1).copy()).to(W.dev()) for _, c, _, _ in pool]
    pad = torch.zeros(32, dtype=torch.uint8, device=W.dev())                  # (a batch of one empty scan still needs an address)
    for n in SIZES:
        ids = W.contents_for(n)
        assert ids[0] == W.EMPTY and (n < 3 or (W.EMPTY in ids[1:-1] and W.FEATURELESS in ids[1:-1]))
        d = torch.cat([d_content[k] for k in ids] + [pad])
        fx.extract_batch_device(d.data_ptr(), np.array([len(pool[k][1]) for k in ids], np.uint32), W.stream())
        fx.batch_status(W.stream())
        exp = W.batch_expect([pool[k][3] for k in ids])
        assert exp.offsets[n] != exp.offsets[2 * n + 1] or n == 1
        for call in W.CALLS:
            W.check_call(fx, exp, call, what="batch of %d" % n)
    fx.close()


def _boundary(table):
    """An interior scan boundary of an offsets table: an entry strictly between 0 and the total, from the middle on."""
    n = len(table) - 1
    for k in list(range(n // 2, n)) + list(range(1, n // 2)):
        if 0 < table[k] < table[n]:
            return int(table[k])
    raise AssertionError("no interior boundary in %s" % table.tolist())


def test_a_capacity_shorter_than_the_payload():
    """capacity_points below the payload: records at or past it are not written (the `< capacity` guards of
    feature_pack_kernel, the 12-byte store among them, and colored_pack_kernel's break), the offsets table is the full one,
    and a size_t capacity above 2^32 is clamped, not truncated (2^32 + 5 would otherwise keep five records).  The edge and
    the surface cloud have their own totals and boundaries: each call runs against both."""
    pool = W.pool()
    ids = W.contents_for(9)
    assert ids[0] == ids[-1] == W.EMPTY and W.FEATURELESS in ids
    fx = FeatureExtraction(device=0, max_points_per_scan=W.POOL_RINGS * W.POOL_COLS, max_batch=len(ids),
                           max_points_per_ring=W.POOL_COLS, max_rings=W.POOL_RINGS)
    d = W.upload([pool[k][1] for k in ids])
    fx.extract_batch_device(d.data_ptr(), np.array([len(pool[k][1]) for k in ids], np.uint32), W.stream())
    fx.batch_status(W.stream())
    exp = W.batch_expect([pool[k][3] for k in ids])
    b = exp.batch
    for call in W.CALLS:
        tables = [exp.colored_offsets] if call == "pack_colored" else [exp.offsets[:b + 1], exp.offsets[b + 1:]]
        capacities = {0, 1, 2 ** 32 + 5}
        for t in tables:
            o, total = _boundary(t), int(t[b])
            assert 1 < o < total - 1
            capacities |= {o - 1, o, o + 1, total - 1, total, total + 3}
        assert len(tables) == 1 or tables[0][b] != tables[1][b]
        for capacity in sorted(capacities):
            W.check_call(fx, exp, call, capacity)
    fx.close()


# ------------------------------------------------------------------------------------------ colored_scan on every route
R, C = 16, 900


def _fx(n, **kw):
    return FeatureExtraction(device=0, max_points_per_scan=R * C, max_batch=n, max_points_per_ring=C, max_rings=R, **kw)


def _piece(cloud, zero=None):
    """The restatement's share of a scan; with the zero filter on, of the scan without its (0, 0, 0) records."""
    kept = cloud if zero is None else np.ascontiguousarray(cloud[~zero])
    return W.scan_piece(kept, W.oracle_of(kept))


def _colored_and_xyz(fx, clouds, pieces, what):
    """The batch through the device path: its routes; colored_scan (all 32 bytes of every record of every scan, and the table)
    and the pcl::PointXYZ payloads beside it against the restatement."""
    d = W.upload(clouds)
    fx.extract_batch_device(d.data_ptr(), np.array([len(c) for c in clouds], np.uint32), W.stream())
    routes = fx.scan_routes(len(clouds), W.stream()).tolist()
    fx.batch_status(W.stream())
    exp = W.batch_expect(pieces)
    assert all(exp.colored_offsets[k + 1] > exp.colored_offsets[k] for k in range(len(clouds)))
    W.check_call(fx, exp, "pack_colored", what="%s routes %s" % (what, routes))
    W.check_call(fx, exp, "pack_xyz", what="%s routes %s" % (what, routes))
    return routes


def _zeroed(c, fraction, seed, rings=None):
    c = c.copy()
    zero = np.random.default_rng(seed).uniform(0, 1, len(c)) < fraction
    if rings is not None:
        zero |= np.isin(c["ring"], rings)
    for f in ("x", "y", "z"):
        c[f][zero] = 0.0
    return c, zero


def test_colored_scan_read_in_place_bucketed_and_both_in_one_batch():
    """Route 1 (an organised scan: every field from the record, the index from the position), route 0 (staged x, y and
    sorted_index, z from the record) and a batch that holds both; then the same batch once the stream has moved to the
    bucketing route for every scan."""
    plain = [make_scan(R, C, seed=4100 + i) for i in range(3)]
    odd = [make_scan(R, C, seed=4110, shuffle=True), make_scan(R, C, seed=4111, drop_fraction=0.07)]
    f = _fx(4)
    assert _colored_and_xyz(f, plain, [_piece(c) for c in plain], "organised") == [1, 1, 1]
    f.close()
    f = _fx(4)
    mixed = [plain[0], odd[0], plain[1], odd[1]]
    pieces = [_piece(c) for c in mixed]
    assert _colored_and_xyz(f, mixed, pieces, "mixed") == [1, 0, 1, 0]
    # (half of that batch fell back: the next one is bucketed whole)
    assert _colored_and_xyz(f, mixed, pieces, "mixed, second batch") == [0, 0, 0, 0]
    f.close()


@pytest.mark.parametrize("kind", ["rotated", "reversed", "reversed_rotated"])
def test_colored_scan_of_turned_rings(kind):
    """Route 2: position k of a ring is column ring_column(xform, k, n) -- (start + k) mod n, or (start - k) mod n for a
    clockwise sensor -- with rings of one scan starting at different columns.  The first batch is bucketed, the later
    ones are read in place through the transforms; the payloads are the same on both."""
    kw = {"rotated": dict(start_col=517), "reversed": dict(reverse=True), "reversed_rotated": dict(reverse=True, start_col=333)}[kind]
    nb = 4
    turned = [make_scan(R, C, seed=4200 + i, **kw) for i in range(nb)]
    for c in turned:
        grid = c.reshape(C, R)
        for r, shift in ((3, 1), (7, 2), (12, 5)):
            grid[:, r] = np.roll(grid[:, r], shift)
    pieces = [_piece(c) for c in turned]
    f = _fx(nb)
    seen = [_colored_and_xyz(f, turned, pieces, "%s batch %d" % (kind, rep)) for rep in range(4)]
    assert seen[0] == [0] * nb and seen[-1] == [2] * nb, seen
    f.close()


def test_colored_scan_of_a_grid_with_holes_and_its_odd_scans_out():
    """Route 3 (x, y, z from the record, the index from sorted_index) for a batch of grids with (0, 0, 0) records, one of
    them without holes; then a batch that mixes such scans with what the holes form hands to the bucketing route: a ring
    left too short, a record with another ring's id, a scan that is no grid."""
    base = [make_scan(R, C, seed=4300 + i) for i in range(5)]
    holes = [_zeroed(c, frac, 60 + i) for i, (c, frac) in enumerate(zip(base[:4], (0.05, 0.0, 0.12, 0.02)))]
    f = _fx(5, drop_zero_points=True, stream_hint=LB.STREAM_GRID_WITH_HOLES)
    clouds, pieces = [c for c, _ in holes], [_piece(c, z) for c, z in holes]
    for rep in range(2):
        assert _colored_and_xyz(f, clouds, pieces, "holes batch %d" % rep) == [3] * 4
    f.close()
    mixed = [_zeroed(base[0], 0.04, 71), _zeroed(base[1], 0.04, 72, rings=[5])]
    c, z = _zeroed(base[2], 0.02, 73)
    short = np.nonzero((c["ring"] == 7) & ~z)[0][8:]                  # ring 7 keeps 8 points: a skip condition
    for fld in ("x", "y", "z"):
        c[fld][short] = 0.0
    z[short] = True
    mixed.append((c, z))
    c, z = _zeroed(base[3], 0.03, 74)
    c["ring"][1234] = (c["ring"][1234] + 3) % R                       # a record with a ring id that is not its place's
    mixed.append((c, z))
    c, z = _zeroed(base[4], 0.03, 75)
    mixed.append((np.ascontiguousarray(c[:-5]), z[:-5]))              # not R x C
    f = _fx(5, drop_zero_points=True, stream_hint=LB.STREAM_GRID_WITH_HOLES)
    clouds, pieces = [c for c, _ in mixed], [_piece(c, z) for c, z in mixed]
    assert _colored_and_xyz(f, clouds, pieces, "holes and odd scans out") == [3, 3, 0, 0, 0]
    _colored_and_xyz(f, clouds, pieces, "holes and odd scans out, second batch")
    f.close()


def test_colored_scan_of_a_scan_the_organised_kernel_gave_up():
    """Two neighbouring records of one ring change places in a late block: the organised-scan kernel has labelled the
    scan's earlier units by then, gives the scan up, and the bucketing route redoes it whole inside the call.  Its
    colored_scan is the staged form's, beside three scans that stay read in place."""
    clouds = [make_scan(R, C, seed=4400 + i) for i in range(4)]
    clouds[2] = clouds[2].copy()
    a, b = R * 600 + 5, R * 601 + 5
    clouds[2][[a, b]] = clouds[2][[b, a]]
    pieces = [_piece(c) for c in clouds]
    f = _fx(4)
    for rep in range(2):
        assert _colored_and_xyz(f, clouds, pieces, "given up, batch %d" % rep) == [1, 1, 0, 1]
    f.close()
