"""The edge and surface rows of lfx_scan_to_map_residuals (row_from_neighbours, lfx_kernels_localize.hpp) against the 50-digit
reference of tests/golden/row_reference.json: every row of every case, none left out, an ill-posed row under its wider
bound.  The fixture only: no mpmath and no oracle here.  What each row is held to (tests/row_cases.py has the arithmetic):

  direction   u_dev from J[:, 4:7] = Hat(2 u), which must be antisymmetric with a zero diagonal exactly;
              |sin(u_dev, u_ref)| <= 2^-53 (8 kappa + 4 kappa^2), kappa = l1 / (l1 - l2); an isotropic neighbourhood
              (k = 1, +-e_i, the cube's corners) gives (0, 0, 1) exactly
  edge sign   | |u_dev| - 1 | <= 4 x 2^-53; the sign is free, and the residual and all 21 Jacobian entries follow the same one
  edge rest   the row evaluated exactly with u := u_dev: every entry within C x 2^-53 x the sum of its absolute terms
  surface     u, J[0:4] and the residual against the 50-digit least-squares solution, within
              C x 2^-53 x (kappa_X + kappa_X^2 |X w + 1| / (|X| |w|)) x the entry's scale; | |u| - 1 | <= 4 x 2^-53;
              a zero row is zero in every bit
  C           8 x the CPU oracle's worst in the same units on the same cases (tests/test_row_reference_expect.py measures
              it: edge 3.51, surface 0.78), so C = 28.08 for an edge row and 6.24 for a surface row
  bytes       cell_size 0 and cell_size 1.0 give the same bytes for every row, ties included; lfx_edge_residuals equals
              lfx_scan_to_map_residuals over the same edge clouds; launch shapes that cross the 128-thread tile, an empty
              cloud, count_stride 4 and maps of 127, 128 and 129 points give the bytes of the single-row calls

Measured on an MI355X, the device's worst over its bound, per family: see DESIGN.md section 7 (the rows)."""
import numpy as np
import pytest

from tests import row_cases as K

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
CELLS = (0.0, 1.0)
NAMES = {K.EDGE: "edge", K.SURFACE: "surface"}


def _groups(data):
    """rows that one call can make: the same kind, map, pose and k"""
    groups = {}
    for row in data["rows"]:
        groups.setdefault((row["kind"], row["group"], row["pose"], row["k"]), []).append(row)
    for row in data["ties"]:
        groups[(row["kind"], row["name"], row["pose"], row["k"])] = [row]
    return groups


class Device:
    """one context, maps kept by (points, cell size), and a call of lfx_scan_to_map_residuals over host arrays"""

    def __init__(self):
        import torch
        from lidar_feature_extraction_amd import FeatureExtraction
        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.fx = FeatureExtraction(device=0, max_points_per_scan=1024, max_batch=1)
        self.maps = {}

    def map(self, points, cell):
        key = (points.tobytes(), cell)
        if key not in self.maps:
            d = self.torch.from_numpy(np.ascontiguousarray(points, np.float32)).to(self.dev)
            self.maps[key] = (self.fx.make_map(d.data_ptr(), len(points), cell), d)
        return self.maps[key][0]

    def rows(self, kind, points, cell, pose, k, pts, begin, count, count_stride, longest, n_rows):
        """-> residual [n_rows][dim], jacobian [n_rows][7 dim], both filled with SENTINEL before the call"""
        t, dim = self.torch, 3 if kind == K.EDGE else 1
        d_pts = t.from_numpy(np.ascontiguousarray(pts, np.float32)).to(self.dev)
        d_b = t.from_numpy(np.asarray(begin, np.uint32).view(np.int32)).to(self.dev)
        d_n = t.from_numpy(np.asarray(count, np.uint32).view(np.int32)).to(self.dev)
        d_res = t.full((n_rows, dim), SENTINEL, dtype=t.float64, device=self.dev)
        d_jac = t.full((n_rows, 7 * dim), SENTINEL, dtype=t.float64, device=self.dev)
        self.fx.scan_to_map_residuals(kind, self.map(points, cell), pose.reshape(3, 4), k, d_pts.data_ptr(), d_b.data_ptr(), d_n.data_ptr(),
                                      count_stride, len(begin), longest, d_res.data_ptr(), d_jac.data_ptr(), 0)
        t.cuda.synchronize()
        return d_res.cpu().numpy(), d_jac.cpu().numpy()

    def nearest(self, points, cell, queries, k):
        t = self.torch
        d_q = t.from_numpy(np.ascontiguousarray(queries, np.float64)).to(self.dev)
        d_i = t.full((len(queries), k), -1, dtype=t.int32, device=self.dev)
        self.map(points, cell).nearest(d_q.data_ptr(), len(queries), k, 0, 0, d_i.data_ptr(), 0)
        t.cuda.synchronize()
        return d_i.cpu().numpy()

    def close(self):
        for m, _ in self.maps.values():
            m.close()
        self.fx.close()


def _map_of(row, data):
    return row["map"] if "map" in row else data["maps"][(row["kind"], row["group"])]


@pytest.fixture(scope="module")
def run():
    """every row of the fixture through the device, once per search route: {(kind, name, pose): {cell: (res, jac, nearest)}}"""
    data = K.load()
    dev = Device()
    got = {}
    for (kind, _, pose_name, k), rows in _groups(data).items():
        m, pose = _map_of(rows[0], data), data["poses"][pose_name][0]
        pts = np.array([list(r["p0"]) + [1.0] for r in rows], np.float32)
        queries = np.array([[float(v) for v in K.query_of(pose, r["p0"])[0]] for r in rows])
        for cell in CELLS:
            res, jac = dev.rows(kind, m, cell, pose, k, pts, [0], [len(rows)], 1, len(rows), len(rows) + 2)
            assert np.all(res[len(rows):] == SENTINEL) and np.all(jac[len(rows):] == SENTINEL)
            near = dev.nearest(m, cell, queries, k)
            for i, r in enumerate(rows):
                got.setdefault((kind, r["name"], r["pose"]), {})[cell] = (res[i], jac[i], near[i])
    yield dict(data=data, dev=dev, got=got)
    dev.close()


def _each(run, kind):
    for row in run["data"]["rows"] + run["data"]["ties"]:
        if row["kind"] == kind:
            yield row, run["got"][(kind, row["name"], row["pose"])]


def _report(what, worst):
    for family, v in sorted(worst.items()):
        print("device, %-34s %-14s worst %.3f of its bound" % (what, family, v))


def test_the_neighbours_are_the_clusters_on_both_routes(run):
    """lfx_map_nearest at the rounded query: the cluster's points (every order of them is the same set), in the order of the
    exact distances wherever those differ by more than rounding -- and at a tie the lower index of the map as it was given."""
    data = run["data"]
    for kind in (K.EDGE, K.SURFACE):
        for row, got in _each(run, kind):
            for cell in CELLS:
                near = got[cell][2].tolist()
                if row["family"] == "tie":
                    assert near == row["neighbours"], (row["name"], cell, near)
                else:
                    assert sorted(near) == list(range(row["first"], row["first"] + row["k"])), (row["name"], row["pose"], cell, near)
    assert len(run["got"]) == len(data["rows"]) + len(data["ties"])


def test_both_search_routes_give_the_same_bytes(run):
    for kind in (K.EDGE, K.SURFACE):
        for row, got in _each(run, kind):
            for part in (0, 1):
                assert got[0.0][part].tobytes() == got[1.0][part].tobytes(), (NAMES[kind], row["name"], row["pose"], part)
            assert not np.any(got[0.0][0] == SENTINEL) and not np.any(got[0.0][1] == SENTINEL)


def test_edge_direction_follows_the_curve(run):
    failed, worst = [], {}
    for row, got in _each(run, K.EDGE):
        m = K.edge_row_units(row, got[0.0][0], got[0.0][1], run["data"])
        print("edge %-28s %-9s kappa %-12.6g |sin| %.3e  %.3f of 2^-53 (8 kappa + 4 kappa^2)" % (row["name"], row["pose"], row["kappa"], m["sin"], m["direction"]))
        worst[row["family"]] = max(worst.get(row["family"], 0.0), m["direction"])
        if not (m["hat_exact"] and m["direction"] <= 1.0):
            failed.append((row["name"], row["pose"], m["direction"], m["hat_exact"]))
        if row["fallback"]:
            assert np.array_equal(m["u"], [0.0, 0.0, 1.0]), (row["name"], m["u"])           # J[:, 4:7] = Hat((0, 0, 2))
            assert np.array_equal(np.asarray(got[0.0][1]).reshape(3, 7)[:, 4:], [[0, -2, 0], [2, 0, 0], [0, 0, 0]])
    _report("direction", worst)
    assert not failed, failed


def test_edge_direction_is_a_unit_vector_with_one_sign(run):
    """| |u| - 1 | <= 4 x 2^-53.  One sign: the row evaluated with u_dev (test_edge_rest...) fixes the residual and the 12
    quaternion entries to the sign of the Hat block; here the row with -u_dev is shown to be far outside the bound, so the
    comparison does tell the two signs apart."""
    failed, worst = [], {}
    for row, got in _each(run, K.EDGE):
        m = K.edge_row_units(row, got[0.0][0], got[0.0][1], run["data"])
        worst[row["family"]] = max(worst.get(row["family"], 0.0), m["norm"] / 4.0)
        if not m["norm"] <= 4.0:
            failed.append((row["name"], row["pose"], m["norm"]))
        flipped = np.asarray(got[0.0][1]).reshape(3, 7).copy()
        flipped[:, 4:] = -flipped[:, 4:]
        assert K.edge_row_units(row, got[0.0][0], flipped.reshape(21), run["data"])["rest"] > 1e6, (row["name"], row["pose"])
    _report("| |u| - 1 | (bound 4 x 2^-53)", worst)
    assert not failed, failed


def test_edge_rest_of_the_row_with_the_devices_direction(run):
    failed, worst = [], {}
    for row, got in _each(run, K.EDGE):
        m = K.edge_row_units(row, got[0.0][0], got[0.0][1], run["data"])
        print("edge %-28s %-9s rest %.3f x 2^-53 of the entry's terms (allowed %.2f)" % (row["name"], row["pose"], m["rest"], K.C_BOUND[K.EDGE]))
        worst[row["family"]] = max(worst.get(row["family"], 0.0), m["rest"] / K.C_BOUND[K.EDGE])
        if not m["rest"] <= K.C_BOUND[K.EDGE]:
            failed.append((row["name"], row["pose"], m["rest"]))
    _report("edge rest (C = %.2f)" % K.C_BOUND[K.EDGE], worst)
    assert not failed, failed


def test_surface_rows_against_the_least_squares_solution(run):
    failed, worst, norms = [], {}, {}
    for row, got in _each(run, K.SURFACE):
        res, jac = got[0.0][0][0], got[0.0][1]
        m = K.surface_row_units(row, res, jac, run["data"])
        if row["zero"]:
            assert m["zero_ok"], (row["name"], res, jac)
            continue
        assert jac[4:].any(), row["name"]
        print("surface %-22s %-9s condition factor %-10.4g worst %.4f (allowed %.2f)  | |u| - 1 | %.2f x 2^-53" % (
            row["name"], row["pose"], row["condition"], m["worst"], K.C_BOUND[K.SURFACE], m["norm"]))
        worst[row["family"]] = max(worst.get(row["family"], 0.0), m["worst"] / K.C_BOUND[K.SURFACE])
        norms[row["family"]] = max(norms.get(row["family"], 0.0), m["norm"] / 4.0)
        if not (m["worst"] <= K.C_BOUND[K.SURFACE] and m["norm"] <= 4.0):
            failed.append((row["name"], row["pose"], m["worst"], m["norm"]))
    _report("surface row (C = %.2f)" % K.C_BOUND[K.SURFACE], worst)
    _report("surface | |u| - 1 | (4 x 2^-53)", norms)
    assert not failed, failed


def test_a_tie_takes_the_lower_index_of_the_map_as_given(run):
    """The two maps hold the same six points in opposite orders, so the mirrored pair's lower index is another point: the rows
    of the two orders differ (both are held to the reference of their own neighbours above), on each route alike."""
    for kind in (K.EDGE, K.SURFACE):
        a, b = [got for row, got in _each(run, kind) if row["family"] == "tie"]
        for cell in CELLS:
            assert a[cell][1].tobytes() != b[cell][1].tobytes()
            assert a[cell][2][-1] == 4 and b[cell][2][-1] == 0


def _filled_map(clusters, n):
    """n points: far filler first, the clusters last (so the last of them lies across index 127 | 128)"""
    filler = np.array([[-50.0 - 3.0 * j, -50.0, 0.0, 1.0] for j in range(n - len(clusters))], np.float32)
    return np.ascontiguousarray(np.concatenate([filler, clusters]))


def test_launch_shapes_give_the_bytes_of_the_single_calls(run):
    """Three clouds of 127, 0 and 129 points in one call (max_points_per_cloud 129: two workgroups of the whole-map route,
    the second with one valid thread), count_stride 4 with sentinels in the unused words, gaps between the clouds' rows;
    against the shared map and against maps of 127, 128 and 129 points, on both routes.  Every row equals the row of the
    single call of its query; rows beyond a cloud's count and the empty cloud's keep what was written before."""
    data, dev = run["data"], run["dev"]
    for kind, group_k in ((K.EDGE, 5), (K.SURFACE, 6)):
        rows = [r for r in data["rows"] if r["kind"] == kind and r["group"] == "near" and r["pose"] == K.BASE and r["k"] == group_k]
        assert len(rows) >= 5
        pose = data["poses"][K.BASE][0]
        near = data["maps"][(kind, "near")]
        clusters = np.concatenate([near[r["first"]:r["first"] + r["k"]] for r in rows])
        begin, count = [0, 130, 135], [127, 0, 129]
        words = np.full(12, 0xFFFFFFFF, np.uint32)
        words[::4] = count
        pts = np.zeros((264, 4), np.float32)
        want_r, want_j, written = {}, {}, np.zeros(268, bool)
        for s in range(3):
            for i in range(count[s]):
                r = rows[(i + s) % len(rows)]
                pts[begin[s] + i] = list(r["p0"]) + [1.0]
                want_r[begin[s] + i], want_j[begin[s] + i] = run["got"][(kind, r["name"], r["pose"])][0.0][:2]
                written[begin[s] + i] = True
        for m in [near] + [_filled_map(clusters, n) for n in (127, 128, 129)]:
            for cell in CELLS:
                res, jac = dev.rows(kind, m, cell, pose, group_k, pts, begin, words, 4, 129, 268)
                assert np.all(res[~written] == SENTINEL) and np.all(jac[~written] == SENTINEL), (NAMES[kind], len(m), cell)
                for at in np.flatnonzero(written):
                    assert res[at].tobytes() == want_r[at].tobytes() and jac[at].tobytes() == want_j[at].tobytes(), (NAMES[kind], len(m), cell, at)


def test_edge_residuals_is_scan_to_map_residuals_over_the_edge_clouds(run):
    """lfx_edge_residuals on an extracted batch of two scans and lfx_scan_to_map_residuals over the same edge clouds (the
    context's own, count_stride 4): the same bytes."""
    import torch
    from lidar_feature_extraction_amd import FeatureExtraction, make_scan, concat
    data = run["data"]
    dev = torch.device("cuda", 0)
    rings, cols, batch, k = 16, 900, 2, 5
    clouds = [make_scan(rings, cols, seed=7300 + s) for s in range(batch)]
    fx = FeatureExtraction(device=0, max_points_per_scan=rings * cols, max_batch=batch, max_points_per_ring=1024, max_rings=rings)
    d = torch.from_numpy(concat(clouds).view(np.uint8).copy()).to(dev)
    fx.extract_batch_device(d.data_ptr(), [len(c) for c in clouds], 0)
    total = sum(len(c) for c in clouds)
    d_map = torch.from_numpy(data["maps"][(K.EDGE, "near")]).to(dev)
    pose = data["poses"][K.BASE][0].reshape(3, 4)
    out = []
    for cell in CELLS:
        m = fx.make_map(d_map.data_ptr(), len(d_map), cell)
        view = fx.device_view()
        bufs = [[torch.full((total, 3), SENTINEL, dtype=torch.float64, device=dev), torch.full((total, 21), SENTINEL, dtype=torch.float64, device=dev)] for _ in range(2)]
        fx.edge_residuals(m, pose, k, bufs[0][0].data_ptr(), bufs[0][1].data_ptr(), 0)
        fx.scan_to_map_residuals(K.EDGE, m, pose, k, view.edge_points, view.scan_begin, view.scan_info + 4 * 2, 4, batch, rings * cols,
                                 bufs[1][0].data_ptr(), bufs[1][1].data_ptr(), 0)
        torch.cuda.synchronize()
        a, b = [[x.cpu().numpy() for x in pair] for pair in bufs]
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        assert (a[0][:, 0] != SENTINEL).sum() > 100 and (a[0][:, 0] == SENTINEL).sum() > 100
        out.append(a)
        m.close()
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    fx.close()
