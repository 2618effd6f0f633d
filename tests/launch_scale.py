"""Whole-batch comparison of the device-resident results with the CPU oracle, for batches of launch scale
(tests/test_launch_scale_gpu.py): every position of a batch, whole arrays, few copies.

A batch is an arrangement `pick` of a few distinct scans: position s holds distinct scan pick[s].  The oracle runs once per
distinct scan; expected_ring_major() lays its result out as lfx_device_view lays one scan out (include/lfx.h); the compare_*
functions take plain numpy arrays (tests/test_launch_scale_expect.py drives them without a device) and are vectorised over the
positions of a slice; assert_batch_equal() is the thin wrapper that copies the view's arrays to the host in slices.

Nothing is left out on any ground: the inputs are chosen free of angle and curvature ties (require_tie_free), so that every
ring position of every scan has one right answer."""
import ctypes as C

import numpy as np

K_RINGS = 256                      # ring_count / ring_status rows of lfx_device_view: [batch][256]
ROUTE_MASK, ORGANISED = 0x300, 0x100        # LFX_SCAN_ROUTE_MASK, LFX_SCAN_ORGANISED
SLICE_BYTES = 1 << 30              # the most that is copied to the host at a time


def require_tie_free(want, what):
    """The oracle result of a distinct scan must carry no tie: a tie would have to be compared in canonical mode."""
    assert want["angle_ties"] == 0 and want["curvature_ties"] == 0, "%s: %d angle ties, %d curvature ties -- choose another seed" % (
        what, want["angle_ties"], want["curvature_ties"])


def expected_ring_major(want, max_rings, cap, keep=None):
    """One oracle result as lfx_device_view lays one scan out: ring r owns [r][0 .. ring_count[r]) of labels_sorted,
    curvature_sorted and sorted_index ([max_rings][cap]; `valid` marks those positions), ring_count / ring_skipped by ring slot
    (the ring id), and the dense clouds with their index lists.  keep: the scan is the oracle's on a filtered cloud; indices into
    the cloud the device was given go through it (tests/parity.py assert_filtered_equal)."""
    rid = np.asarray(want["ring_id"], np.int64)
    cnt = np.asarray(want["ring_count"], np.int64)
    assert rid.size == 0 or (rid.max() < max_rings and cnt.max() <= cap), "the oracle's rings do not fit the layout"
    off = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    n = int(cnt.sum())
    assert n == len(want["sorted_index"]), "ring counts and sorted_index disagree"
    ring_of = np.repeat(rid, cnt)                              # per sorted position: its ring slot ...
    k_of = np.arange(n) - np.repeat(off, cnt)                  # ... and its place in the ring
    sidx = np.asarray(want["sorted_index"], np.int64)
    orig = sidx if keep is None else np.asarray(keep, np.int64)[sidx]
    out = {
        "valid": np.zeros((max_rings, cap), bool),
        "labels_sorted": np.zeros((max_rings, cap), np.uint8),
        "curvature_sorted": np.zeros((max_rings, cap), np.float64),
        "sorted_index": np.zeros((max_rings, cap), np.uint32),
        "ring_count": np.zeros(K_RINGS, np.uint32),
        "ring_skipped": np.zeros(K_RINGS, bool),
    }
    out["valid"][ring_of, k_of] = True
    out["labels_sorted"][ring_of, k_of] = want["labels"][sidx]
    out["curvature_sorted"][ring_of, k_of] = want["curvature"][sidx]
    out["sorted_index"][ring_of, k_of] = orig.astype(np.uint32)
    out["ring_count"][rid] = cnt.astype(np.uint32)
    out["ring_skipped"][rid] = np.asarray(want["ring_status"]) != 0
    for kind in ("edge", "surface"):
        idx = np.asarray(want[kind + "_index"], np.int64)
        out["n_" + kind] = len(idx)
        out[kind + "_points"] = np.ascontiguousarray(want[kind + "_points"], np.float32).reshape(-1, 4)
        out[kind + "_index"] = (idx if keep is None else np.asarray(keep, np.int64)[idx]).astype(np.uint32)
    return out


def invert_ring_major(exp, n_points):
    """(labels, curvature, seen) per original point from the ring-major arrays through their own sorted_index."""
    labels, curv, seen = np.zeros(n_points, np.uint8), np.zeros(n_points, np.float64), np.zeros(n_points, bool)
    at = exp["sorted_index"][exp["valid"]]
    labels[at] = exp["labels_sorted"][exp["valid"]]
    curv[at] = exp["curvature_sorted"][exp["valid"]]
    seen[at] = True
    return labels, curv, seen


class Expected:
    """The expectations of the distinct scans, stacked: one row per distinct scan."""

    def __init__(self, per_scan, n_points):
        self.n = len(per_scan)
        self.n_points = np.asarray(n_points, np.int64)         # records of each distinct scan as the device is given it
        self.per_scan = per_scan
        for k in ("valid", "labels_sorted", "curvature_sorted", "sorted_index", "ring_count", "ring_skipped"):
            setattr(self, k, np.stack([e[k] for e in per_scan]))
        self.n_edge = np.array([e["n_edge"] for e in per_scan], np.int64)
        self.n_surface = np.array([e["n_surface"] for e in per_scan], np.int64)

    def payload(self, pick, kind, what):
        """The batch's clouds (or index lists) back to back, and their offsets table (exclusive prefix, [batch + 1])."""
        counts = getattr(self, "n_" + kind)[pick]
        offs = np.concatenate([[0], np.cumsum(counts)])
        parts = [self.per_scan[u][kind + "_" + what] for u in pick]
        width = (0, 4) if what == "points" else (0,)
        dtype = np.float32 if what == "points" else np.uint32
        return (np.concatenate(parts) if parts else np.zeros(width, dtype)), offs


def _fail(ctx, pick, s, array, detail):
    raise AssertionError("%s: position %d (distinct scan %d): %s: %s" % (ctx, s, int(pick[s]), array, detail))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def compare_tables(got, pick, exp, max_rings, ctx):
    """scan_info[s][2:4], scan_begin, ring_count and ring_status (zero / non-zero where ring_count > 0) of every position."""
    pick = np.asarray(pick, np.int64)
    B = len(pick)
    info = np.asarray(got["scan_info"]).reshape(-1, 4)[:B]
    for col, name, want in ((2, "n_edge", exp.n_edge[pick]), (3, "n_surface", exp.n_surface[pick])):
        bad = np.nonzero(info[:, col] != want)[0]
        if bad.size:
            _fail(ctx, pick, bad[0], "scan_info[%d] (%s)" % (col, name), "got %d want %d (%d positions differ)" % (
                info[bad[0], col], want[bad[0]], bad.size))
    begin = np.concatenate([[0], np.cumsum(exp.n_points[pick])])
    gb = np.asarray(got["scan_begin"])[:B + 1]
    bad = np.nonzero(gb != begin)[0]
    if bad.size:
        _fail(ctx, pick, min(bad[0], B - 1), "scan_begin[%d]" % bad[0], "got %d want %d" % (gb[bad[0]], begin[bad[0]]))
    rc = np.asarray(got["ring_count"]).reshape(-1, K_RINGS)[:B, :max_rings]
    want_rc = exp.ring_count[pick][:, :max_rings]
    bad = np.argwhere(rc != want_rc)
    if bad.size:
        s, r = bad[0]
        _fail(ctx, pick, s, "ring_count", "ring %d: got %d want %d (%d rings differ)" % (r, rc[s, r], want_rc[s, r], len(bad)))
    rs = np.asarray(got["ring_status"]).reshape(-1, K_RINGS)[:B, :max_rings] != 0
    want_rs = exp.ring_skipped[pick][:, :max_rings]
    bad = np.argwhere((rs != want_rs) & (want_rc > 0))
    if bad.size:
        s, r = bad[0]
        _fail(ctx, pick, s, "ring_status", "ring %d: got %s want %s" % (r, "skipped" if rs[s, r] else "ok", "skipped" if want_rs[s, r] else "ok"))
    return B


def compare_ring_major(name, got, first, pick, exp, ctx, only=None):
    """One ring-major array (`got`: [k][max_rings][cap], the scans first .. first + k of the batch) by bits over each ring's
    valid positions.  only: bool [k], the scans of the slice to compare (sorted_index: those that were not read in place as
    organised scans).  Returns the number of positions compared."""
    pick = np.asarray(pick, np.int64)
    k = len(got)
    rows = np.arange(k) if only is None else np.nonzero(only)[0]
    if rows.size == 0:
        return 0
    u = pick[first + rows]
    want = _bits(getattr(exp, name))[u]
    g = _bits(got)[rows]
    bad = (g != want) & exp.valid[u]
    if bad.any():
        i, r, p = np.argwhere(bad)[0]
        s = first + int(rows[i])
        gv, wv = np.asarray(got)[rows[i], r, p], getattr(exp, name)[u[i], r, p]
        _fail(ctx, pick, s, name, "ring %d position %d: got %r want %r (%d elements differ in the slice)" % (r, p, gv, wv, int(bad.sum())))
    return int(rows.size)


def compare_payload(name, got, want, offs, pick, ctx):
    """A batch's dense records back to back (`got`, `want`: [total] or [total][4]) by bits; offs: [batch + 1]."""
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, "%s: %s: %s records, want %s" % (ctx, name, g.shape, w.shape)
    if len(g) == 0:
        return
    bad =np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
    if bad.size:
        s = int(np.searchsorted(offs, bad[0], side="right") - 1)
        _fail(ctx, pick, s, name, "record %d of the scan: got %r want %r (%d records differ)" % (
            bad[0] - offs[s], np.asarray(got)[bad[0]].tolist(), np.asarray(want)[bad[0]].tolist(), bad.size))


def compare_batch(got, pick, exp, max_rings, ctx):
    """The comparison core on plain numpy arrays.  got: scan_info [B][4], scan_begin [B + 1], ring_count / ring_status
    [B][256], labels_sorted / curvature_sorted (or None) / sorted_index [B][max_rings][cap], and the clouds with their
    index lists as the view holds them (scan s: from record scan_begin[s]).  Returns the number of positions compared."""
    pick = np.asarray(pick, np.int64)
    B = compare_tables(got, pick, exp, max_rings, ctx)
    n = compare_ring_major("labels_sorted", got["labels_sorted"], 0, pick, exp, ctx)
    assert n == B
    if got.get("curvature_sorted") is not None:
        assert compare_ring_major("curvature_sorted", got["curvature_sorted"], 0, pick, exp, ctx) == B
    info = np.asarray(got["scan_info"]).reshape(-1, 4)[:B]
    indexed = (info[:, 1] & ROUTE_MASK) != ORGANISED
    compare_ring_major("sorted_index", got["sorted_index"], 0, pick, exp, ctx, only=indexed)
    begin = np.asarray(got["scan_begin"], np.int64)
    for kind in ("edge", "surface"):
        counts = getattr(exp, "n_" + kind)[pick]
        for what in ("points", "index"):
            want, offs = exp.payload(pick, kind, what)
            src = np.asarray(got[kind + "_" + what])
            rows = np.concatenate([begin[s] + np.arange(counts[s]) for s in range(B)]) if B else np.zeros(0, np.int64)
            compare_payload(kind + "_" + what, src[rows.astype(np.int64)], want, offs, pick, ctx)
    return B


# ------------------------------------------------------------------------------------------------- the device wrapper
_hip = None


def _copy(dst, src, nbytes):
    """nbytes from device address src into the numpy array dst (hipMemcpy, device to host)."""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemcpy.restype = C.c_int
    if nbytes:
        assert nbytes <= dst.nbytes
        rc = _hip.hipMemcpy(dst.ctypes.data, int(src), int(nbytes), 2)
        assert rc == 0, "hipMemcpy failed with %d" % rc


def _table(ptr, shape, dtype):
    out = np.zeros(shape, dtype)
    _copy(out, ptr, out.nbytes)
    return out


def assert_batch_equal(fx, pick, exp, ctx, curvature=True):
    """The device-resident results of the context's last batch against the expectations, for EVERY position: the view's arrays
    are copied to the host in slices of at most SLICE_BYTES and compared with the core above.  Returns the number of positions
    compared, after asserting that it is the batch."""
    import torch
    torch.cuda.synchronize()
    pick = np.asarray(pick, np.int64)
    B = len(pick)
    v = fx.device_view()
    R, cap = int(v.max_rings), int(v.ring_capacity)
    assert v.batch == B, "%s: the view is of %d scans, the batch of %d" % (ctx, v.batch, B)
    assert exp.valid.shape[1:] == (R, cap), "%s: expectations laid out for %s, the view is %d x %d" % (ctx, exp.valid.shape[1:], R, cap)
    got = {"scan_info": _table(v.scan_info, (B, 4), np.uint32), "scan_begin": _table(v.scan_begin, B + 1, np.uint32),
           "ring_count": _table(v.ring_count, (B, K_RINGS), np.uint32), "ring_status": _table(v.ring_status, (B, K_RINGS), np.uint8)}
    seen = {"tables": compare_tables(got, pick, exp, R, ctx)}
    assert bool(v.curvature_sorted) == bool(curvature), "%s: curvature_sorted is %s" % (ctx, "there" if v.curvature_sorted else "NULL")
    indexed = (got["scan_info"][:, 1] & ROUTE_MASK) != ORGANISED
    for name, ptr, dtype in (("labels_sorted", v.labels_sorted, np.uint8), ("curvature_sorted", v.curvature_sorted, np.float64),
                             ("sorted_index", v.sorted_index, np.uint32)):
        if not ptr:
            continue
        per_scan = R * cap * np.dtype(dtype).itemsize
        step = max(1, min(B, SLICE_BYTES // (4 * per_scan)))       # (the copy, the expectation, the mask and their difference)
        buf = np.zeros((step, R, cap), dtype)
        seen[name] = 0
        for first in range(0, B, step):
            k = min(step, B - first)
            if name == "sorted_index" and not indexed[first:first + k].any():
                continue
            _copy(buf, int(ptr) + first * per_scan, k * per_scan)
            seen[name] += compare_ring_major(name, buf[:k], first, pick, exp, ctx, only=indexed[first:first + k] if name == "sorted_index" else None)
        assert seen[name] == (int(indexed.sum()) if name == "sorted_index" else B), "%s: %s: %d positions compared" % (ctx, name, seen[name])
    begin = got["scan_begin"].astype(np.int64)
    for kind in ("edge", "surface"):
        counts = getattr(exp, "n_" + kind)[pick]                   # (= scan_info[s][2], [3]: compare_tables has passed)
        for what, ptr, dtype, rec in (("points", getattr(v, kind + "_points"), np.float32, 16), ("index", getattr(v, kind + "_index"), np.uint32, 4)):
            want, offs = exp.payload(pick, kind, what)
            have = np.zeros(want.shape, dtype)
            flat = have.reshape(-1).view(np.uint8)
            for s in range(B):                                     # scan s: its first n records from record scan_begin[s]
                if counts[s]:
                    _copy(flat[offs[s] * rec:], int(ptr) + int(begin[s]) * rec, int(counts[s]) * rec)
            compare_payload(kind + "_" + what, have, want, offs, pick, ctx)
    n = min(seen["tables"], seen["labels_sorted"], seen.get("curvature_sorted", B))
    assert n == B, "%s: %d positions compared, the batch has %d" % (ctx, n, B)
    return n


def assert_packed_equal(fx, pick, exp, ctx):
    """pack_features and pack_xyz12 of the whole batch: offset tables = prefix sums of the oracle's counts, payload = the
    oracle's clouds back to back."""
    import torch
    pick = np.asarray(pick, np.int64)
    B = len(pick)
    we, oe = exp.payload(pick, "edge", "points")
    ws, osf = exp.payload(pick, "surface", "points")
    capacity = int(max(oe[-1], osf[-1], 1))
    st = torch.cuda.current_stream().cuda_stream
    for name, width, call in (("pack_features", 4, fx.pack_features), ("pack_xyz12", 3, fx.pack_xyz12)):
        e = torch.zeros((capacity, width), dtype=torch.float32, device="cuda:0")
        s = torch.zeros((capacity, width), dtype=torch.float32, device="cuda:0")
        offs = torch.zeros(2 * (B + 1), dtype=torch.int32, device="cuda:0")
        call(e.data_ptr(), s.data_ptr(), offs.data_ptr(), capacity, st)
        torch.cuda.synchronize()
        offs = offs.cpu().numpy().view(np.uint32).reshape(2, B + 1)
        for row, o, kind in ((0, oe, "edge"), (1, osf, "surface")):
            bad = np.nonzero(offs[row] != o)[0]
            if bad.size:
                _fail(ctx, pick, min(bad[0], B - 1), "%s offsets (%s)" % (name, kind), "entry %d: got %d want %d" % (bad[0], offs[row][bad[0]], o[bad[0]]))
        compare_payload(name + " edge", e.cpu().numpy()[:oe[-1]], we[:, :width], oe, pick, ctx)
        compare_payload(name + " surface", s.cpu().numpy()[:osf[-1]], ws[:, :width], osf, pick, ctx)
