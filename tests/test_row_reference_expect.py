"""(CPU) The 50-digit reference of the scan-to-map rows (tools/row_reference.py, tests/golden/row_reference.json) held from
four sides, and the CPU oracle measured against it -- the measurement that fixes what tests/test_rows_gpu.py allows the
device.  No device here.

  * the fixture is what the tool writes (where mpmath is importable; else the file is taken as it is), its clusters are the
    k nearest map points of their queries by exact distances, and no surface case lies near the no-plane threshold;
  * the analytic 3 x 7 and 1 x 7 rows equal the derivative of the residual with respect to (q, t) at 50 digits
    (mpmath.diff; p1, p2 and w held fixed): a statement that shares no formula with the kernel;
  * the rational evaluation of tests/row_cases.py (what the device test uses in mpmath's place) equals the tool's;
  * the oracle's rows in the device test's units.  Measured here (orc_loc_edge_residuals with the oracle's own u;
    orc_loc_surface_residuals), worst per kind: the figures of row_cases.ORACLE_WORST, asserted below; the device is allowed
    8 times that (row_cases.C_BOUND).
  * a double-precision port of the device's closed-form principal_direction against the 50-digit eigenvector, over the
    bound 2^-53 (8 kappa + 4 kappa^2): a PORT's figures (numpy, this machine's libm), not a bound on the device -- the
    device is measured in tests/test_rows_gpu.py."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np

from tests import row_cases as K

PD, PF = C.POINTER(C.c_double), C.POINTER(C.c_float)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    try:
        import mpmath  # noqa: F401
    except ImportError:
        return None
    spec = importlib.util.spec_from_file_location("row_reference", os.path.join(ROOT, "tools", "row_reference.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _all_rows(data):
    return data["rows"] + data["ties"]


def _map_of(row, data):
    return row["map"] if "map" in row else data["maps"][(row["kind"], row["group"])]


def test_the_fixture_is_current_and_its_clusters_are_the_neighbours():
    tool = _tool()
    if tool is None:
        print("mpmath is not here: the file is taken as it is")
    else:
        with open(K.PATH) as f:
            assert f.read() == tool.text(), "tests/golden/row_reference.json is not what tools/row_reference.py writes"
    largest = max(os.path.getsize(os.path.join(ROOT, "tests", "golden", n)) for n in os.listdir(os.path.join(ROOT, "tests", "golden")))
    assert os.path.getsize(K.PATH) < largest
    data = K.load()
    names = set()
    for row in _all_rows(data):
        pose, _ = data["poses"][row["pose"]]
        q, _ = K.query_of(pose, row["p0"])
        m = _map_of(row, data)
        assert len(m) >= row["k"]
        got, kth, nxt = K.nearest_exact(m[:, :3], q, row["k"])
        if row["family"] == "tie":
            assert got == row["neighbours"] and kth == nxt and got[-1] == (0 if row["reversed"] else 4)
        else:
            assert sorted(got) == list(range(row["first"], row["first"] + row["k"])), row["name"]
            assert nxt is None or kth == 0 or nxt > 16 * kth                  # the next map point is 4 times as far as the k-th
        names.add((row["kind"], row["name"], row["pose"]))
    assert len(names) == len(_all_rows(data))
    # every case the rows are there for
    edge = {r["name"] for r in data["rows"] if r["kind"] == K.EDGE}
    surf = {r["name"] for r in data["rows"] if r["kind"] == K.SURFACE}
    assert {"k1", "k2", "k3", "k5", "k15", "k16", "iso_axes", "iso_cube", "axis_x", "axis_y", "axis_z", "l2_equals_l3"} <= edge
    assert {"k3", "k5", "k15", "k16", "first_x_zero", "first_x_negative", "column_zero_below", "column_all_zero", "coincident",
            "exact_line", "line_thick_1e-11", "line_thick_1e-6", "plane_d1000_0"} <= surf
    for kind in (K.EDGE, K.SURFACE):
        assert {r["pose"] for r in data["rows"] if r["kind"] == kind} == set(K.POSES)
    fallback = {r["name"] for r in data["rows"] if r["kind"] == K.EDGE and r["fallback"]}
    assert fallback == {"k1", "iso_axes", "iso_cube"}
    zero = {r["name"] for r in data["rows"] if r["kind"] == K.SURFACE and r["zero"]}
    assert zero == {"column_all_zero", "coincident", "exact_line", "line_thick_1e-11"}
    # the pivots the cases are there for
    first = {r["name"]: K.neighbours_of(r, data) for r in data["rows"] if r["kind"] == K.SURFACE and r["pose"] == K.BASE}
    for name, sign in (("first_x_zero", 0.0), ("first_x_negative", -1.0), ("column_zero_below", 1.0)):
        row = [r for r in data["rows"] if r["kind"] == K.SURFACE and r["name"] == name][0]
        q, _ = K.query_of(data["poses"][row["pose"]][0], row["p0"])
        order = K.nearest_exact(_map_of(row, data)[:, :3], q, row["k"])[0]
        assert order[0] == row["first"] and np.sign(first[name][0, 0]) == sign
    assert not first["column_zero_below"][1:, 0].any() and not first["column_all_zero"][:, 0].any()
    # the branches of the quaternion: the trace of each pose
    tr = {n: p[0] + p[5] + p[10] for n, (p, _) in data["poses"].items()}
    assert tr["identity"] > 0 and tr["rot005"] > 0 and tr["turn_111"] == 0.0 and all(tr[n] < 0 for n in ("x179", "y179", "z179", "turn_1m10", "general"))
    for n, i in (("x179", 1), ("y179", 2), ("z179", 3), ("turn_111", 1)):
        quat = data["poses"][n][1]
        assert quat[i] > 0 and abs(quat[i]) == np.abs(quat).max() or n == "turn_111" and np.all(quat == 0.5), (n, quat)
    p, quat = data["poses"]["turn_1m10"]
    assert p[0] == p[5] == 0.0 > p[10] and quat[0] == 0.0 and quat[1] > 0 > quat[2] and quat[1] == -quat[2] and quat[3] == 0.0


def test_the_rows_are_the_derivative_of_the_residual():
    """d residual / d (q, t) by mpmath.diff at 50 digits, the residual as a function of a free (not normalised) quaternion:
    x = q p q* + t, edge (x - p1) x (x - p2), surface (w . x + 1) / |w|; p1, p2, w held.  Agreement to 1e-25 of the entry's
    scale (the differences are of order 1e-30)."""
    tool = _tool()
    if tool is None:
        print("mpmath is not here: nothing to differentiate with")
        return
    mp = tool._mp()
    data = K.load()

    def moved(qt, p):
        w, v, t = qt[0], list(qt[1:4]), list(qt[4:7])
        vp, vv, vxp = sum(v[i] * p[i] for i in range(3)), sum(x * x for x in v), tool.cross(v, p)
        return [(w * w - vv) * p[i] + 2 * vp * v[i] + 2 * w * vxp[i] + t[i] for i in range(3)]
    worst = 0.0
    picked = [r for r in _all_rows(data) if r["name"] in ("k5", "disc_thick_0.5", "plane_d1_tilt", "line_noise_1e-3_off5000", "plane_d1000_1")]
    assert len(picked) >= 8 * 3 + 2
    for row in picked:
        pose, _ = data["poses"][row["pose"]]
        nb, p = K.neighbours_of(row, data), [mp.mpf(float(v)) for v in row["p0"]]
        at = tool.quaternion(mp, pose) + [mp.mpf(pose[4 * r + 3]) for r in range(3)]
        if row["kind"] == K.EDGE:
            r = tool.edge_row(mp, nb, row["p0"], pose)
            p1, p2 = [r["mean"][i] - r["u"][i] for i in range(3)], [r["mean"][i] + r["u"][i] for i in range(3)]
            fs = [lambda *qt, i=i: tool.cross([a - b for a, b in zip(moved(qt, p), p1)], [a - b for a, b in zip(moved(qt, p), p2)])[i] for i in range(3)]
        else:
            r = tool.surface_row(mp, nb, row["p0"], pose)
            nw = mp.sqrt(sum(v * v for v in r["w"]))
            fs = [lambda *qt: (sum(r["w"][i] * moved(qt, p)[i] for i in range(3)) + 1) / nw]
        for i, f in enumerate(fs):
            for c in range(7):
                got = mp.diff(f, tuple(at), tuple(int(j == c) for j in range(7)))
                want, scale = r["jacobian"][7 * i + c], r["jacobian_scale"][7 * i + c] + 1
                worst = max(worst, float(abs(got - want) / scale))
    print("analytic rows against mpmath.diff: worst %.2e of the entry's scale" % worst)
    assert worst < 1e-25


def test_the_rational_evaluation_is_the_tools():
    """tests/row_cases.py's Fraction arithmetic against the tool's 50 digits, with the reference u in both: the only
    difference is the quaternion's rounding to doubles in the fixture (2^-53 of each component), so 4 x 2^-53 of an entry's
    scale is allowed; the scales themselves agree to 1e-15."""
    tool = _tool()
    if tool is None:
        print("mpmath is not here: the rational evaluation is not compared")
        return
    mp = tool._mp()
    data = K.load()
    worst = 0.0
    for row in _all_rows(data):
        pose, quat = data["poses"][row["pose"]]
        nb = K.neighbours_of(row, data)
        if row["kind"] == K.EDGE:
            r = tool.edge_row(mp, nb, row["p0"], pose, u=row["u"])
            res, rs, J, Js = K.edge_row_exact(nb, row["p0"], pose, quat, row["u"])
            pairs = [(res, r["residual"], rs, r["residual_scale"]), (J, r["jacobian"], Js, r["jacobian_scale"])]
        else:
            r = tool.surface_row(mp, nb, row["p0"], pose)
            assert r["zero"] == row["zero"]
            if row["zero"]:
                continue
            J, Js, rs = K.surface_row_exact(row["p0"], pose, quat, row["u"], row["inv_norm_w"])
            pairs = [(J, r["jacobian"][:4], Js[:4], r["jacobian_scale"][:4]), ([row["residual"]], [r["residual"]], [rs], [r["residual_scale"]])]
        for got, want, scale, wscale in pairs:
            for g, w, s, ws in zip(got, want, scale, wscale):
                assert abs(s - float(ws)) <= 1e-6 * float(ws) + 0.0, (row["name"], s, float(ws))
                if ws == 0:
                    assert g == float(w)
                else:
                    worst = max(worst, float(abs(mp.mpf(float(g)) - w) / ws) / K.EPS)
    print("rational evaluation against 50 digits: worst %.2f x 2^-53 of the entry's scale" % worst)
    assert worst <= 4.0


def _groups(data):
    """rows that one call can make: the same kind, map, pose and k"""
    groups = {}
    for row in data["rows"]:
        groups.setdefault((row["kind"], row["group"], row["pose"], row["k"]), []).append(row)
    for row in data["ties"]:
        groups[(row["kind"], row["name"], row["pose"], row["k"])] = [row]
    return groups


def oracle_rows(data):
    """[(row, residual, jacobian)] from the CPU oracle, every row of the fixture"""
    from oracle import binding as OB
    L = OB.lib()
    out = []
    for (kind, _, pose_name, k), rows in _groups(data).items():
        m = np.ascontiguousarray(_map_of(rows[0], data), np.float32)
        pose = np.ascontiguousarray(data["poses"][pose_name][0])
        pts = np.ascontiguousarray(np.array([list(r["p0"]) + [1.0] for r in rows], np.float32))
        n, dim = len(rows), 3 if kind == K.EDGE else 1
        res, jac = np.zeros((n, dim)), np.zeros((n, 7 * dim))
        fn = L.orc_loc_edge_residuals if kind == K.EDGE else L.orc_loc_surface_residuals
        fn(OB.ptr(m, PF), len(m), OB.ptr(pose, PD), k, OB.ptr(pts, PF), n, OB.ptr(res, PD), OB.ptr(jac, PD))
        out += [(r, res[i], jac[i]) for i, r in enumerate(rows)]
    return out


def test_the_oracle_in_the_device_tests_units():
    """The measurement that fixes C.  Zero rows: the oracle's are the reference's (asserted, before any device run)."""
    data = K.load()
    worst, by_family = {K.EDGE: 0.0, K.SURFACE: 0.0}, {}
    for row, res, jac in oracle_rows(data):
        if row["kind"] == K.EDGE:
            got = K.edge_row_units(row, res, jac, data)
            # (the oracle's Hat(p2 - p1) is made of the rounded p1 and p2: its u is what that block says, its length is not held)
            assert got["hat_exact"] and np.isfinite(got["rest"])
            v = got["rest"]
            line = "rest %.2f, direction %.3f of its bound (Jacobi)" % (v, got["direction"] if not row["fallback"] else 0.0)
        else:
            got = K.surface_row_units(row, res[0], jac, data)
            if row["zero"]:
                assert got["zero_ok"], row["name"]
                continue
            assert res[0] != 0.0 or jac.any()
            v = got["worst"]
            line = "worst %.3f (condition factor %.3g)" % (v, row["condition"])
        print("%-8s %-28s %-9s %s" % ("edge" if row["kind"] == K.EDGE else "surface", row["name"], row["pose"], line))
        worst[row["kind"]] = max(worst[row["kind"]], v)
        key = (row["kind"], row["family"])
        by_family[key] = max(by_family.get(key, 0.0), v)
    for (kind, family), v in sorted(by_family.items()):
        print("oracle, %-7s %-14s worst %.3f" % ("edge" if kind == K.EDGE else "surface", family, v))
    print("oracle's worst: edge %.3f, surface %.3f; recorded %s; C = %s" % (worst[K.EDGE], worst[K.SURFACE], K.ORACLE_WORST, K.C_BOUND))
    for kind in (K.EDGE, K.SURFACE):
        assert worst[kind] <= K.ORACLE_WORST[kind] and K.C_BOUND[kind] == 8.0 * K.ORACLE_WORST[kind]
        assert worst[kind] > 0.5 * K.ORACLE_WORST[kind]                    # (the recorded figure is the measured one, not a loose cap)


def principal_direction_port(c):
    """lfx_kernels_localize.hpp's principal_direction, statement for statement, in numpy doubles (xx xy xz yy yz zz)"""
    shift = (c[0] + c[3] + c[5]) / 3.
    a00, a11, a22, a01, a02, a12 = c[0] - shift, c[3] - shift, c[5] - shift, c[1], c[2], c[4]
    scale = max(abs(a00), abs(a11), abs(a22), abs(a01), abs(a02), abs(a12))
    if not scale > 0.:
        return np.array([0., 0., 1.])
    inv = 1. / scale
    a00, a11, a22, a01, a02, a12 = a00 * inv, a11 * inv, a22 * inv, a01 * inv, a02 * inv, a12 * inv
    c0 = a00 * a11 * a22 + 2. * a01 * a02 * a12 - a00 * a12 * a12 - a11 * a02 * a02 - a22 * a01 * a01
    c1 = a00 * a11 - a01 * a01 + a00 * a22 - a02 * a02 + a11 * a22 - a12 * a12
    a3 = max(-c1 / 3., 0.)
    half_b = 0.5 * c0
    qd = max(a3 * a3 * a3 - half_b * half_b, 0.)
    rho, theta = math.sqrt(a3), math.atan2(math.sqrt(qd), half_b) / 3.
    lam = 2. * rho * math.cos(theta)
    lo = -rho * (math.cos(theta) + 1.7320508075688772 * math.sin(theta))
    if not lam - lo > 1e-14:
        return np.array([0., 0., 1.])
    m00, m11, m22 = a00 - lam, a11 - lam, a22 - lam
    col0, col1, col2 = np.array([m00, a01, a02]), np.array([a01, m11, a12]), np.array([a02, a12, m22])
    d0, d1, d2 = abs(m00), abs(m11), abs(m22)
    rep, o1, o2 = col0, col1, col2
    if d1 > d0 and d1 >= d2:
        rep, o1, o2 = col1, col2, col0
    elif d2 > d0 and d2 > d1:
        rep, o1, o2 = col2, col0, col1
    cr = lambda a, b: np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])  # noqa: E731
    x1, x2 = cr(rep, o1), cr(rep, o2)
    n1, n2 = x1[0] * x1[0] + x1[1] * x1[1] + x1[2] * x1[2], x2[0] * x2[0] + x2[1] * x2[1] + x2[2] * x2[2]
    v, nn = (x1, n1) if n1 > n2 else (x2, n2)
    if not nn > 0.:
        return np.array([0., 0., 1.])
    return v * (1. / math.sqrt(nn))


def test_the_port_of_the_closed_form_follows_the_curve():
    """A PORT of principal_direction (mean and covariance summed as the kernel sums them, in the fixture's order of the
    map), not the device: |sin(u_port, u_ref)| over 2^-53 (8 kappa + 4 kappa^2), per family."""
    data = K.load()
    by_family = {}
    for row in _all_rows(data):
        if row["kind"] != K.EDGE:
            continue
        nb = K.neighbours_of(row, data).astype(np.float64)
        k = len(nb)
        mean = np.zeros(3)
        for p in nb:
            mean = mean + p
        mean = mean / k
        c = np.zeros(6)
        for p in nb:
            e = p - mean
            c = c + np.array([e[0] * e[0], e[0] * e[1], e[0] * e[2], e[1] * e[1], e[1] * e[2], e[2] * e[2]])
        u = principal_direction_port(c / k)
        if row["fallback"]:
            assert np.array_equal(u, [0., 0., 1.]), row["name"]
            continue
        ratio = float(np.linalg.norm(np.cross(u, row["u"]))) / K.direction_bound(row["kappa"])
        by_family[row["family"]] = max(by_family.get(row["family"], 0.0), ratio)
        assert ratio <= 1.0, (row["name"], row["pose"], ratio, row["kappa"])
    for family, v in sorted(by_family.items()):
        print("port, %-14s worst |sin| %.3f of 2^-53 (8 kappa + 4 kappa^2)" % (family, v))
