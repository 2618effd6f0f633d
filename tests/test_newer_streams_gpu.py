"""The ordering include/lfx.h promises across streams for the three newer subsystems -- "calls on different streams are
ordered one behind the other: they share the workspace" (segmentation), "a query on another stream is ordered behind the last
add" (the place index), "calls on one map are ordered behind its last insert whichever streams they use" (the rolling map)
-- with two streams, A and B, and every result compared with the restatements byte for byte.

Every case first warms the workspaces it uses with one call of the largest size, so that the part that counts neither
allocates nor frees.  A *held* case queues a busy kernel of torch's on the producer's stream (tests/segment_cases.py Hold:
sized for 50 ms from a measurement on the device), then the producer, then records an event E behind it, and asserts
`not E.query()` at the moment the dependent call is issued on the other stream: the dependent call was issued while the
producer had not run, so only the library's own wait can have put it behind.  The value chosen on an MI355X: 1.10 - 1.14
x 10^8 units of torch.cuda._sleep (0.44 - 0.46 ms per 10^6), a hold of 50 ms; the dependent calls were issued 0.04 - 0.5 ms
after their hold was queued, the first one of the process 5.5 - 6.8 ms after (the sleep kernel's first launch on that stream).
The module's fixture prints both for every held case.

The waits the cases rest on (none of them is ever taken out on a device: without it a kernel can leave its buffers):
  (a) hipStreamWaitEvent(st, db->added) in lfx_place_db_query and lfx_place_db_download, and in add_device for the second add;
  (b) hipEventSynchronize(slot->used) in take_slot: a slot's table and keys are rewritten only after the call that used them;
  (c) hipStreamWaitEvent(st, w.used) in take_workspace, which also puts a cache hit behind the upload of the table it hits,
      and hipEventSynchronize(w.used) in put_tables before a slot's pinned block is refilled;
  (d) the same wait in take_workspace and the one in lfx_pack_features_segmented for the context's own counts;
  (e) order_behind's hipStreamWaitEvent(st, rm->tail) in the extraction, the view and the save;
  (f) the same in lfx_rolling_map_insert and in the update loop's cuts, and settle's hipEventSynchronize(rm->tail)."""
import ctypes as C

import numpy as np
import pytest

from tests import deskew_cases as K
from tests import rolling_map_restatement as RM
from tests import scan_context_restatement as SC
from tests import segment_cases as S
from tests import segment_restatement as R


@pytest.fixture(scope="module")
def hold():
    h = S.Hold()
    print("a hold: %d units of %s, %.3f ms per %d measured" % (h.amount, "torch.cuda._sleep" if h.sleep else "matmuls", h.ms_per_unit, h.unit))
    yield h
    for what, ms in h.issue_ms:
        print("held %.0f ms; issued %.3f ms after the hold was queued: %s" % (S.HOLD_MS, ms, what))


# --- (a) the place index ------------------------------------------------------------------------------------------------------
def _descriptors(rng, n, shape=(20, 60)):
    d = rng.uniform(0.0, 5.0, (n,) + shape).astype(np.float32)
    d[rng.uniform(0, 1, d.shape) < 0.1] = 0.0
    return d


def _matches(raw, n):
    return [(None if m.entry == 0xFFFFFFFF else int(m.entry), int(m.shift), float(m.distance), float(m.yaw)) for m in raw[:n]]


@pytest.mark.gpu
def test_place_index_queries_and_downloads_behind_adds_on_the_other_stream(hold):
    """8 entries and a query of the largest size first (the query's workspace).  Then 4 entries added on held A and at once
    queried on B: the restatement over those 4.  4 more added on held B and queried on A: over the 8 (the second add waits
    for the first one's event, the query for the second's).  4 more on held A and at once downloaded on B."""
    import torch
    rng = np.random.default_rng(91)
    pool, queries = _descriptors(rng, 20), _descriptors(rng, 3)
    queries[0] = np.roll(pool[9], -7, axis=1)
    queries[2] = np.roll(pool[14], -11, axis=1)
    k = 4
    want = lambda first, count: [(None if e is None else e + first, s, d, y) for q in queries for e, s, d, y in SC.query(q, pool[first:first + count], k)]
    fx = K.fx_for(16, 900, 1)
    db = fx.place_db(20)
    d_pool, d_q = torch.from_numpy(pool).to(K.dev()), torch.from_numpy(queries).to(K.dev())
    a, b = S.two_streams()
    db.add(d_pool[:8], 8, K.stream())
    assert _matches(db.query_raw(d_q, 3, k, 0, 8, K.stream()), 3 * k) == want(0, 8)
    K.sync()
    # 4 entries on held A, queried on B
    hold(a)
    db.add(d_pool[8:12], 4, a.cuda_stream)
    e = S.event_behind(a)
    hold.still_held(e, "place index: add on A, query on B")
    got = _matches(db.query_raw(d_q, 3, k, 8, 4, b.cuda_stream), 3 * k)
    assert got == want(8, 4), (got[:2], want(8, 4)[:2])
    assert got[0][:2] == (9, 7) and abs(got[0][2]) < 1e-15
    # 4 more on held B, all 8 queried on A
    K.sync()
    hold(b)
    db.add(d_pool[12:16], 4, b.cuda_stream)
    e = S.event_behind(b)
    hold.still_held(e, "place index: add on B, query on A")
    got = _matches(db.query_raw(d_q, 3, k, 8, 8, a.cuda_stream), 3 * k)
    assert got == want(8, 8)
    assert got[2 * k][:2] == (14, 11)
    # 4 more on held A, downloaded on B
    K.sync()
    hold(a)
    db.add(d_pool[16:20], 4, a.cuda_stream)
    e = S.event_behind(a)
    hold.still_held(e, "place index: add on A, download on B")
    assert db.download(16, 4, b.cuda_stream).tobytes() == pool[16:20].tobytes()
    K.sync()
    assert len(db) == 20 and db.download(stream=K.stream()).tobytes() == pool.tobytes()
    assert _matches(db.query_raw(d_q, 3, k, 0, 20, K.stream()), 3 * k) == want(0, 20)
    db.close()
    fx.close()


# --- (b) the scan-context ring ------------------------------------------------------------------------------------------------
GRIDS = [dict(n_rings=1, n_sectors=4), dict(), dict(n_rings=40, n_sectors=120)]


@pytest.mark.gpu
def test_scan_context_calls_take_the_ring_of_slots_round_on_two_streams():
    """Four calls of the largest grid first: every slot of the ring (lfx_ctx::kPlaceSlots = 4) has its room.  Then 10 calls
    over one batch of 3 scans, alternating A / B, the grids cycling through 1 x 4, 20 x 60 and 40 x 120: slot i % 4 serves the
    calls i, i + 4, i + 8 with the grids i % 3, (i + 1) % 3, (i + 2) % 3 -- each slot is reused twice with a table and a key
    block of another size.  Every call has its own output; one synchronise at the end."""
    import torch
    clouds = S.scans33()[:3]
    fx = K.fx_for(S.RINGS, S.COLS, 3)
    d = S.device_batch(fx, clouds)
    fx.batch_status(K.stream())
    shape = lambda f: (3, f.get("n_rings", 20), f.get("n_sectors", 60))
    for _ in range(4):
        fx.scan_context(SC.config(**GRIDS[2]), None, K.stream())
    plan = [GRIDS[i % 3] for i in range(10)]
    assert all(plan[i] != plan[i + 4] for i in range(6))
    outs = [torch.full(shape(f), float("nan"), dtype=torch.float32, device=K.dev()) for f in plan]
    a, b = S.two_streams()
    K.sync()
    for i, (f, out) in enumerate(zip(plan, outs)):
        fx.scan_context(SC.config(**f), out.data_ptr(), (a, b)[i % 2].cuda_stream)
    K.sync()
    for i, (f, out) in enumerate(zip(plan, outs)):
        S.same_floats(out.cpu().numpy(), S.descriptors_want(3, **f), ("call", i, f))
    del d
    fx.close()


# --- (c) segmentation's table cache ------------------------------------------------------------------------------------------
# (n_columns, row_step) of c0 .. c5 -- c0 and c1 differ in row_step only, c0 and c2 in n_columns only -- and c6, c0 but for
# segment_min_points: the key of c0 with other kernel arguments
CACHE = [dict(n_columns=900), dict(n_columns=900, row_step=0.005), dict(n_columns=360), dict(n_columns=450), dict(n_columns=600, row_step=0.02),
         dict(n_columns=300), dict(n_columns=900, segment_min_points=2)]
CACHE_ORDER = [0, 1, 2, 3, 4, 5, 0, 5, 6, 1]
SEG_TABLES = 4                                # lfx_ctx::SegmentWork::kSegTables


def _cache_walk(order, configs, occupied):
    """What put_tables does with the calls: 'fill' (an empty slot), 'refill' (a slot that holds a table) or 'hit'."""
    key = lambda f: (f["n_columns"], f.get("row_step"))
    slots, at, out = list(occupied), len(occupied) % SEG_TABLES, []
    for i in order:
        k = key(configs[i])
        if k in slots:
            out.append("hit")
            continue
        if len(slots) < SEG_TABLES:
            slots.append(k)
            out.append("fill")
        else:
            slots[at] = k
            out.append("refill")
        at = (at + 1) % SEG_TABLES
    return out


def test_the_cache_plan_refills_and_hits():
    """(no device) After the four warming configs the order c0 .. c5, c0, c5, c6, c1 is six refills, then c0 evicted and
    refilled, c5 and c6 hits, c1 refilled; the pair that differs in row_step only and the pair that differs in n_columns only
    have different results, as have c0 and c6."""
    warm = [(900, 0.011 + 0.001 * j) for j in range(SEG_TABLES)]
    assert _cache_walk(CACHE_ORDER, CACHE, warm) == ["refill"] * 7 + ["hit", "hit", "refill"]
    clouds = S.scans33()[:3]
    want = [R.segment_batch(R.config(n_rows=S.RINGS, **f), clouds) for f in (CACHE[0], CACHE[1], CACHE[2], CACHE[6])]
    for other in want[1:]:
        assert other[0].tobytes() != want[0][0].tobytes() or other[1].tobytes() != want[0][1].tobytes()
    assert (want[1][0] != want[0][0]).sum() + (want[1][1] != want[0][1]).sum() > 100


@pytest.mark.gpu
def test_segmentation_configs_go_through_the_table_cache_on_two_streams(hold):
    """Four configs of the largest table first (every slot of the cache has its room, and the workspace its size).  Then the
    ten calls of CACHE_ORDER alternating A / B, each into outputs of its own, one synchronise at the end.  Then a config never
    seen before on held A and at once the same config on B into other outputs: B's call is a cache hit whose table has not
    gone up yet."""
    clouds = S.scans33()[:3]
    total = sum(len(c) for c in clouds)
    fx = K.fx_for(S.RINGS, S.COLS, 3)
    d = S.device_batch(fx, clouds)
    fx.batch_status(K.stream())
    for j in range(SEG_TABLES):
        fx.segment(R.config(n_rows=S.RINGS, n_columns=900, row_step=0.011 + 0.001 * j), stream=K.stream())
    outs = [S.seg_outputs(total, 3) for _ in range(len(CACHE_ORDER) + 2)]
    a, b = S.two_streams()
    K.sync()
    for i, c in enumerate(CACHE_ORDER):
        fx.segment(R.config(n_rows=S.RINGS, **CACHE[c]), *outs[i], (a, b)[i % 2].cuda_stream)
    K.sync()
    for i, c in enumerate(CACHE_ORDER):
        S.same(S.numpy_of(outs[i]), R.segment_batch(R.config(n_rows=S.RINGS, **CACHE[c]), clouds), ("call", i, CACHE[c]))
    # the held case
    new = R.config(n_rows=S.RINGS, n_columns=720, row_step=0.03)
    want = R.segment_batch(new, clouds)
    hold(a)
    fx.segment(new, *outs[-2], a.cuda_stream)
    e = S.event_behind(a)
    hold.still_held(e, "segmentation: a new config on A, the same on B")
    fx.segment(new, *outs[-1], b.cuda_stream)
    print("the producer had %s when B's call had been issued" % ("not run" if not e.query() else "run"))
    K.sync()
    S.same(S.numpy_of(outs[-2]), want, "held A")
    S.same(S.numpy_of(outs[-1]), want, "B behind held A")
    del d
    fx.close()


# --- (d) segmentation's shared workspace ---------------------------------------------------------------------------------------
MASKS = [(4, 6), (15, 15), (2, 1), (8, 4), (6, 9), (1, 14)]


@pytest.mark.gpu
def test_segmentation_calls_share_the_workspace_across_streams(hold):
    """The 33 scans; 128 x 4096 (two chunks: the largest workspace), 16 x 900 and one filtered pack first.  Then 128 x 4096
    on held A and at once 16 x 900 on B, which takes the images, the cells and the union-find's parents the first call is
    still to use.  Then six lfx_pack_features_segmented calls with d_counts_out = NULL and six different mask pairs,
    alternating A / B: all of them count into the context's own block."""
    import torch
    from lidar_feature_extraction_amd import binding as B
    clouds = S.scans33()
    n, total = len(clouds), sum(len(c) for c in clouds)
    begin = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    fx = S.fx33()
    d = S.device_batch(fx, clouds)
    fx.batch_status(K.stream())
    features = []
    for s in range(n):
        g = fx.download(s, K.stream())
        features.append((g.edge_points, g.edge_index, g.surface_points, g.surface_index))
    big, small = dict(n_rows=128, n_columns=4096), dict(n_rows=S.RINGS, n_columns=S.COLS)
    outs = [S.seg_outputs(total, n) for _ in range(3)]
    fx.segment(R.config(**big), *outs[2], K.stream())
    fx.segment(R.config(**small), *outs[2], K.stream())
    L = B.load()

    def pack(classes, masks, buffers, stream):
        edge, surface, offsets = buffers
        B.check(fx._ctx, L.lfx_pack_features_segmented(fx._ctx, C.c_void_p(classes.data_ptr()), masks[0], masks[1], C.c_void_p(edge.data_ptr()),
                                                       C.c_void_p(surface.data_ptr()), C.c_void_p(offsets.data_ptr()), None, total, C.c_void_p(stream)))

    buffers = [(torch.full((total, 4), 1234.5, dtype=torch.float32, device=K.dev()), torch.full((total, 4), 1234.5, dtype=torch.float32, device=K.dev()),
                torch.full((2, n + 1), -1, dtype=torch.int32, device=K.dev())) for _ in MASKS]
    pack(outs[2][0], MASKS[0], buffers[0], K.stream())
    a, b = S.two_streams()
    K.sync()
    hold(a)
    fx.segment(R.config(**big), *outs[0], a.cuda_stream)
    e = S.event_behind(a)
    hold.still_held(e, "segmentation: 128 x 4096 x 33 on A, 16 x 900 x 33 on B")
    fx.segment(R.config(**small), *outs[1], b.cuda_stream)
    K.sync()
    S.same(S.numpy_of(outs[0]), S.segment_want(n, **big), "A: 128 x 4096")
    got = S.numpy_of(outs[1])
    S.same(got, S.segment_want(n, **small), "B: 16 x 900")
    for i, masks in enumerate(MASKS):
        pack(outs[1][0], masks, buffers[i], (a, b)[i % 2].cuda_stream)
    K.sync()
    kept = []
    for i, masks in enumerate(MASKS):
        we, ws, woff, _ = R.filtered_pack(got[0], begin, features, masks[0], masks[1])
        edge, surface, offsets = (t.cpu().numpy() for t in buffers[i])
        assert offsets.view(np.uint32).tobytes() == woff.tobytes(), (i, masks)
        assert edge[:len(we)].tobytes() == we.tobytes() and surface[:len(ws)].tobytes() == ws.tobytes(), (i, masks)
        assert (edge[len(we):] == np.float32(1234.5)).all() and (surface[len(ws):] == np.float32(1234.5)).all(), (i, masks)
        kept.append((len(we), len(ws)))
    assert len(set(kept)) >= len(MASKS) - 1 and kept[1] == (sum(len(f[1]) for f in features), sum(len(f[3]) for f in features)), kept
    del d
    fx.close()


# --- (e) the rolling map: insert, then read on the other stream ---------------------------------------------------------------
class FastStore(RM.Store):
    """tests/rolling_map_restatement.py Store with the insert rule over arrays: the voxels of a window have slots of their
    own, so of the records that reach a slot the first in (cloud, index) order is stored unless the slot holds that voxel
    already, and the others find it live.  test_the_fast_store_is_the_store holds it to Store."""

    def insert(self, clouds, poses):
        o, n = np.array(self.o, np.int64), np.array(self.n, np.int64)
        for cloud, pose in zip(clouds, poses):
            c = np.asarray(cloud, np.float32).reshape(-1, 4)
            if len(c) == 0:
                continue
            q = RM.transform(pose, c)
            v, ok = RM.voxels(q, self.inv)
            inside = ok & ((v >= o) & (v < o + n)).all(axis=1)
            self.counts["nonfinite"] += int((~ok).sum())
            self.counts["outside"] += int((ok & ~inside).sum())
            idx = np.flatnonzero(inside)
            vi = v[idx]
            slot = ((vi[:, 2] % n[2]) * n[1] + vi[:, 1] % n[1]) * n[0] + vi[:, 0] % n[0]
            slots, first = np.unique(slot, return_index=True)
            inserted = 0
            for s, f in zip(slots.tolist(), first.tolist()):
                k = RM.key(vi[f])
                if self.keys.get(s, 0) != k:
                    self.keys[s], self.points[s] = k, q[idx[f]]
                    inserted += 1
            self.counts["inserted"] += inserted
            self.counts["merged"] += len(idx) - inserted


def _roll_cloud(rng, n, spread, centre=(0.0, 0.0, 0.0)):
    c = np.empty((n, 4), np.float32)
    c[:, :3] = rng.normal(0, 1, (n, 3)) * spread + np.asarray(centre)
    c[:, 3] = rng.normal(0, 1, n)
    for value in (np.nan, np.inf, 1e30):
        c[rng.random(n) < 0.002, rng.integers(0, 3)] = value
    return c


def _roll_pose(rng):
    from tests.mapping_restatement import pose
    w = rng.normal(0, 0.4, 3)
    th = np.linalg.norm(w)
    u = w / th
    Kx = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return pose(np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx, rng.normal(0, 0.3, 3))


def test_the_fast_store_is_the_store():
    """(no device) Three inserts of 3 000 records with a move of the window between them: keys, points and counters."""
    rng = np.random.default_rng(8300)
    slow, fast = RM.Store(0.5, (8, 6, 4)), FastStore(0.5, (8, 6, 4))
    for r in range(3):
        clouds = [_roll_cloud(rng, 3000, 1.2, (0.6 * r, 0, 0)), _roll_cloud(rng, 10, 1.0)]
        poses = [_roll_pose(rng), _roll_pose(rng)]
        for s in (slow, fast):
            s.insert(clouds, poses)
            s.recenter([0.6 * (r + 1), 0.1, 0.0])
        assert slow.counts == fast.counts and slow.keys == fast.keys and slow.o == fast.o
        assert all(slow.points[k].tobytes() == fast.points[k].tobytes() for k in slow.keys)
        assert slow.extract_all().tobytes() == fast.extract_all().tobytes() and len(slow.extract_all()) > 50
    assert min(slow.counts.values()) > 0


ROLL = dict(edge_leaf=0.5, surface_leaf=0.7, edge_dims=(64, 64, 32), surface_dims=(48, 40, 24))
ROLL_RECORDS = 200000


@pytest.mark.gpu
def test_rolling_map_reads_behind_an_insert_on_the_other_stream(tmp_path):
    """Six rounds, the inserting stream alternating, the kind too, the window moved once (no device work).  A round is one
    insert of 200 000 records -- 782 workgroups of claims and commits behind the call's table -- and at once, on the other
    stream, the extraction of the whole window and the view; after the last round the save.  All equal the restatement
    after that insert."""
    import torch
    from lidar_feature_extraction_amd import RollingMap, read_pcd
    rng = np.random.default_rng(8301)
    fx = K.fx_for(16, 64, 1)
    rm = RollingMap(fx, **ROLL)
    ref = dict(edge=FastStore(ROLL["edge_leaf"], ROLL["edge_dims"]), surface=FastStore(ROLL["surface_leaf"], ROLL["surface_dims"]))
    kinds = ["edge", "surface", "edge", "surface", "edge", "edge"]
    centre = lambda r: (2.0, -1.0, 0.5) if r >= 3 else (0.0, 0.0, 0.0)
    clouds = [_roll_cloud(rng, ROLL_RECORDS, 0.3 * float(ref[kinds[r]].leaf) * 64, centre(r)) for r in range(6)]
    for c in clouds:
        c[:, 3] = 1.0                                                   # (a PCD file holds x, y, z)
    poses = [_roll_pose(rng) for _ in range(6)]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(K.dev())
    d_clouds = [up(c) for c in clouds]
    d_begin, d_count = up(np.zeros(1, np.uint32).view(np.int32)), up(np.array([ROLL_RECORDS], np.uint32).view(np.int32))
    most = max(int(np.prod(ROLL["edge_dims"])), int(np.prod(ROLL["surface_dims"])))
    out = torch.zeros((most, 4), dtype=torch.float32, device=K.dev())
    # (another map first: the kernels are loaded.  The map under test takes its pinned block in round 0 and frees nothing.)
    warm = RollingMap(fx, **ROLL)
    warm.insert("edge", d_clouds[0].data_ptr(), d_begin.data_ptr(), d_count.data_ptr(), 1, 1, ROLL_RECORDS, poses[0][None], K.stream())
    warm.view(K.stream())
    warm.close()
    a, b = S.two_streams()
    K.sync()
    for r in range(6):
        kind = kinds[r]
        writer, reader = ((a, b), (b, a))[r % 2]
        if r == 3:
            rm.recenter(centre(r))
            for s in ref.values():
                s.recenter(centre(r))
        rm.insert(kind, d_clouds[r].data_ptr(), d_begin.data_ptr(), d_count.data_ptr(), 1, 1, ROLL_RECORDS, poses[r][None], writer.cuda_stream)
        lo, hi = ref[kind].window()
        n = rm.extract_device(kind, lo, hi, out.data_ptr(), most, reader.cuda_stream)
        view = rm.view(reader.cuda_stream)
        got = out[:n].cpu().numpy()
        ref[kind].insert([clouds[r]], [poses[r]])
        want = ref[kind].extract_all()
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (r, kind, got.shape, want.shape)
        for k in ("edge", "surface"):
            assert {c: view[k][c] for c in ref[k].counts} == ref[k].counts, (r, k)
            assert view[k]["live"] == len(ref[k].extract_all()) and view[k]["origin"] == ref[k].o, (r, k)
        assert len(want) > 20000 and ref[kind].counts["merged"] > 20000
    rm.insert("surface", d_clouds[5].data_ptr(), d_begin.data_ptr(), d_count.data_ptr(), 1, 1, ROLL_RECORDS, poses[4][None], a.cuda_stream)
    assert rm.save(str(tmp_path), b.cuda_stream) == (True, True)
    ref["surface"].insert([clouds[5]], [poses[4]])
    for kind in ("edge", "surface"):
        assert read_pcd(str(tmp_path / (kind + ".pcd"))).tobytes() == ref[kind].extract_all().tobytes(), kind
    K.sync()
    rm.close()
    fx.close()


# --- (f) the rolling map: a chain of updates ------------------------------------------------------------------------------------
def _bits(r):
    return (r["pose"].tobytes(), r["initial_pose"].tobytes(), r["error"], r["error_scale"], r["iteration"], r["code"], r["aligned"],
            r["inserted"], r["recentered"], r["n_edge_map"], r["n_surface_map"])


def _whole(rm, kind):
    v = rm.view(K.stream())[kind]
    leaf = float(v["leaf"])
    lo = [(v["origin"][a] + 0.5) * leaf for a in range(3)]
    hi = [(v["origin"][a] + v["dims"][a] - 0.5) * leaf for a in range(3)]
    return rm.extract(kind, lo, hi, K.stream())


@pytest.mark.gpu
def test_rolling_map_update_chain_over_two_streams():
    """4 scans of a moving 16 x 900 sensor through lfx_rolling_map_update_batch in 4 calls on one map, alternating A / B:
    every call's boxes are cut behind the insert the call before queued on the other stream.  Results, the final whole
    windows and the view equal the same 4 calls on one stream on a fresh map, byte for byte."""
    from lidar_feature_extraction_amd import make_sequence
    clouds, _ = make_sequence(4, S.RINGS, S.COLS, seed=8100)
    a, b = S.two_streams()
    dims = dict(edge_dims=(256, 256, 64), surface_dims=(128, 128, 32))

    def chain(streams):
        fx = K.fx_for(S.RINGS, S.COLS, 1)
        rm = fx.rolling_map(**dims)
        out = []
        for k, c in enumerate(clouds):
            d, _ = K.extract(fx, [c])
            K.sync()
            out += rm.update_batch(None, 1, streams[k])
        K.sync()
        state = (_whole(rm, "edge"), _whole(rm, "surface"), rm.view(K.stream()), rm.pose())
        rm.close()
        fx.close()
        return out, state

    two, state2 = chain([a.cuda_stream, b.cuda_stream, a.cuda_stream, b.cuda_stream])
    one, state1 = chain([K.stream()] * 4)
    assert [_bits(r) for r in two] == [_bits(r) for r in one]
    assert sum(r["aligned"] for r in one) >= 2 and all(r["inserted"] for r in one), [(r["aligned"], r["inserted"], r["code"]) for r in one]
    assert state2[0].tobytes() == state1[0].tobytes() and state2[1].tobytes() == state1[1].tobytes() and len(state1[0]) > 500 and len(state1[1]) > 500
    assert state2[2]["edge"] == state1[2]["edge"] and state2[2]["surface"] == state1[2]["surface"] and state2[3].tobytes() == state1[3].tobytes()


@pytest.mark.gpu
def test_rolling_map_host_inserts_then_an_update_over_two_streams():
    """lfx_rolling_map_insert_host of two scans' clouds on A, B, A -- each call rewrites the staged cloud and the pinned
    table the call before it, on the other stream, read -- then lfx_rolling_map_update_batch of a third scan on B, whose
    boxes are cut behind the last insert on A.  The result, the whole windows, the view and the pose equal the same four
    calls on one stream on a fresh map, byte for byte."""
    from lidar_feature_extraction_amd import make_sequence
    clouds, _ = make_sequence(3, S.RINGS, S.COLS, seed=8102)
    a, b = S.two_streams()
    fx = K.fx_for(S.RINGS, S.COLS, 2)
    _, got = K.extract(fx, clouds[:2])
    host = [(np.ascontiguousarray(g.edge_points, np.float32).reshape(-1, 4).copy(), np.ascontiguousarray(g.surface_points, np.float32).reshape(-1, 4).copy())
            for g in got]
    d, _ = K.extract(fx, clouds[2:])
    K.sync()

    def chain(streams):
        rm = fx.rolling_map(edge_dims=(256, 256, 64), surface_dims=(128, 128, 32))
        rm.insert_host("edge", host[0][0], None, streams[0])
        rm.insert_host("surface", host[0][1], None, streams[1])
        rm.insert_host("edge", host[1][0], None, streams[2])
        out = rm.update_batch(None, 1, streams[3])
        K.sync()
        state = (_whole(rm, "edge"), _whole(rm, "surface"), rm.view(K.stream()), rm.pose())
        rm.close()
        return out, state

    one, state1 = chain([K.stream()] * 4)
    two, state2 = chain([a.cuda_stream, b.cuda_stream, a.cuda_stream, b.cuda_stream])
    fx.close()
    assert [_bits(r) for r in two] == [_bits(r) for r in one]
    assert one[0]["aligned"] and one[0]["inserted"], (one[0]["aligned"], one[0]["inserted"], one[0]["code"])
    assert state2[0].tobytes() == state1[0].tobytes() and state2[1].tobytes() == state1[1].tobytes() and len(state1[0]) > 500 and len(state1[1]) > 500
    assert state2[2]["edge"] == state1[2]["edge"] and state2[2]["surface"] == state1[2]["surface"] and state2[3].tobytes() == state1[3].tobytes()
