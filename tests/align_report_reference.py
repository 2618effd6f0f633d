"""lfx_align_report twice over, for tests/test_align_report_expect.py (host) and tests/test_align_report_edges_gpu.py (device):

reference(pose, r3, J3, r1, J1): the DEFINITION (include/lfx.h) from a scan's rows at 50 digits in mpmath -- e_i, the median
and the MAD as sorted() gives them, the weights, D, A, H = M^T A M, mpmath.eigsy of H and of D, sigma2, the floored
covariance, the rank -- and the margins that say how far the inputs sit from every decision the record takes: each
eigenvalue's gap to its neighbours, each normalised error's distance from 1.345^2, each eigenvalue's distance from the floor.
The constants (1.482602218505602, 1.345, 1e-16, 1e-9) are the doubles the device's code holds.  M is built from
report_restatement.quaternion_of in float64, as the host hands the device the quaternion in doubles.

algorithm(H, sigma2) / algorithm_d(D): the second half of report_finish_h / report_finish_d (lfx_kernels_report.hpp) in plain
Python floats, operation by operation, nothing fused: jacobi_eigen (cyclic order p < q, the 2^-100 stopping test on the
squared norms, at most 30 sweeps, apq == 0 skipped, a <- a J and then a <- J^T a), the five-pass bubble sort with its strict
<, the sign rule (first largest fabs, strict >), the floor, the rank and the covariance summed in k order; for D the minimum
of the diagonal.  The device is held to these bit for bit, these to reference() within measured constants
(tests/align_report_cases.py)."""
import math

import mpmath as mp
import numpy as np

from tests.report_restatement import make_m, quaternion_of

DIGITS = 50
HUBER_K = 1.345
MAD_TO_SIGMA = 1.482602218505602
FLOOR = 1e-9
SWEEPS = 30
STOP = 7.888609052210118e-31           # 2^-100
CLUSTER_GAP = 1e-6                     # eigenvalues closer than this (relative to the largest) are compared as one span
NAN = float("nan")


def _median(values):
    v = sorted(values)
    n = len(v)
    return v[(n - 1) // 2] if n & 1 else (v[n // 2 - 1] + v[n // 2]) / 2


def _to_array(m, rows, cols):
    return np.array([[float(m[i, j]) for j in range(cols)] for i in range(rows)], np.float64)


def sign_rule(rows):
    """every row's first component of largest magnitude made positive"""
    out = np.array(rows, np.float64)
    for k in range(len(out)):
        if out[k][int(np.argmax(np.abs(out[k])))] < 0:
            out[k] = -out[k]
    return out


def clusters(lam):
    """runs of eigenvalues (ascending) whose neighbours lie within CLUSTER_GAP * the largest: [(first, last + 1), ...]"""
    top = max(abs(float(lam[-1])), abs(float(lam[0])))
    out, first = [], 0
    for k in range(1, len(lam) + 1):
        if k == len(lam) or float(lam[k] - lam[k - 1]) > CLUSTER_GAP * top:
            out.append((first, k))
            first = k
    return out


def reference(pose, r3, J3, r1, J1):
    """The record of one scan from its rows (as lfx_scan_to_map_residuals returns them: r3 [n3][3], J3 [n3][21], r1 [n1],
    J1 [n1][7]) at 50 digits, rounded to float64 at the end.  Needs at least one row."""
    r3 = np.asarray(r3, np.float64).reshape(-1, 3)
    J3 = np.asarray(J3, np.float64).reshape(-1, 7)
    r1 = np.asarray(r1, np.float64).reshape(-1)
    J1 = np.asarray(J1, np.float64).reshape(-1, 7)
    n3, n1 = len(r3), len(r1)
    assert n3 + n1 > 0
    with mp.workdps(DIGITS):
        f = mp.mpf
        e = [f(a) * f(a) + f(b) * f(b) + f(c) * f(c) for a, b, c in r3.tolist()] + [f(a) * f(a) for a in r1.tolist()]
        median = _median(e)
        scale = f(MAD_TO_SIGMA) * _median([abs(x - median) for x in e])
        k, k2 = f(HUBER_K), f(HUBER_K) * f(HUBER_K)
        en = [x / (scale + f(1e-16)) for x in e]
        w = [f(1) if x < k2 else k / mp.sqrt(x) for x in en]
        inlier = [x < k2 for x in en]
        huber_margin = min(abs(x - k2) / k2 for x in en)
        w_rows = [w[i // 3] for i in range(3 * n3)] + w[n3:]
        J = np.vstack([J3, J1])
        cols = [[f(x) for x in J[:, a].tolist()] for a in range(7)]
        wcols = [[wi * x for wi, x in zip(w_rows, col)] for col in cols]
        D, A = mp.zeros(7, 7), mp.zeros(7, 7)
        for a in range(7):
            for b in range(a, 7):
                D[a, b] = D[b, a] = mp.fdot(cols[a], cols[b])
                A[a, b] = A[b, a] = mp.fdot(wcols[a], cols[b])
        Mf = make_m(quaternion_of(np.asarray(pose, np.float64).reshape(3, 4)[:, :3]))
        M = mp.matrix(Mf.tolist())
        H = M.T * A * M
        H = (H + H.T) / 2
        lam_m, Q = mp.eigsy(H)
        order = sorted(range(6), key=lambda i: lam_m[i])
        lam = [lam_m[i] for i in order]
        vec = [[Q[c, i] for c in range(6)] for i in order]
        lam_d = sorted(mp.eigsy(D, eigvals_only=True))
        floor = f(FLOOR) * lam[5]
        dim = 3 * mp.fsum(w[:n3]) + mp.fsum(w[n3:]) - 6
        sigma2 = mp.fdot(w, e) / dim if dim > 0 else None
        cov = None
        if sigma2 is not None:
            cov = mp.zeros(6, 6)
            for i in range(6):
                s = sigma2 / max(lam[i], floor)
                for r in range(6):
                    for c in range(6):
                        cov[r, c] += s * vec[i][r] * vec[i][c]
        e3, e1 = mp.fsum(e[:n3]), mp.fsum(e[n3:])
        gaps = []
        for i in range(6):
            near = [abs(lam[i] - lam[j]) for j in (i - 1, i + 1) if 0 <= j < 6]
            gaps.append(float(min(near) / lam[5]) if lam[5] > 0 else 0.0)
        floor_margin = [float(abs(x - floor) / floor) if floor > 0 else 0.0 for x in lam]
        # the largest terms of the sums, for the bounds of tests/align_report_cases.py
        row_norm2 = [mp.fsum(x * x for x in row) for row in [[cols[a][i] for a in range(7)] for i in range(len(w_rows))]]
        out = dict(
            information=_to_array(H, 6, 6), eigenvalues=np.array([float(x) for x in lam]),
            eigenvectors=sign_rule([[float(x) for x in v] for v in vec]),
            covariance=_to_array(cov, 6, 6) if cov is not None else np.full((6, 6), NAN),
            rank=sum(1 for x in lam if x > floor), sigma2=float(sigma2) if sigma2 is not None else NAN, dim=float(dim),
            D=_to_array(D, 7, 7), A=_to_array(A, 7, 7), eigenvalues_d=np.array([float(x) for x in lam_d]),
            min_eigenvalue_d=float(lam_d[0]), error=float(e3 + e1), error_scale=float(scale),
            rms_edge=float(mp.sqrt(e3 / n3)) if n3 else 0.0, rms_surface=float(mp.sqrt(e1 / n1)) if n1 else 0.0,
            n_edge=n3, n_surface=n1, n_edge_inliers=sum(inlier[:n3]), n_surface_inliers=sum(inlier[n3:]),
            n_surface_no_plane=int((~J1[:, 4:7].any(axis=1)).sum()) if n1 else 0,
            gaps=np.array(gaps), huber_margin=float(huber_margin), floor_margin=np.array(floor_margin),
            cond=float(lam[5] / max(lam[0], floor)), norm_h=float(max(abs(lam[0]), abs(lam[5]))),
            norm_d=float(max(abs(lam_d[0]), abs(lam_d[6]))), norm_m2=float(np.linalg.norm(Mf, 2) ** 2),
            sum_w_j2=float(mp.fdot(w_rows, row_norm2)), sum_w_dim=float(dim + 6), sum_w_e=float(mp.fdot(w, e)),
            weights=np.array([float(x) for x in w]))
    return out


# ---- the device's algorithm in plain floats ---------------------------------------------------------------------------------

def _div(a, b):
    """a / b as IEEE has it where b is 0 (Python raises there)"""
    if b == 0.0:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def jacobi_eigen(a, n, vectors):
    """jacobi_eigen<n, vectors> on the row-major list a (changed in place): (settled, v); column k of v belongs to a[k][k]"""
    v = [1.0 if i // n == i % n else 0.0 for i in range(n * n)] if vectors else None
    for sweep in range(SWEEPS + 1):
        off, diag = 0.0, 0.0
        for p in range(n):
            diag += a[n * p + p] * a[n * p + p]
            for q in range(p + 1, n):
                off += a[n * p + q] * a[n * p + q]
        if 2.0 * off <= STOP * diag:
            return True, v
        if sweep == SWEEPS:
            break
        for p in range(n):
            for q in range(p + 1, n):
                apq = a[n * p + q]
                if apq != 0.0:
                    theta = _div(a[n * q + q] - a[n * p + p], 2.0 * apq)
                    t = _div(-1.0 if theta < 0.0 else 1.0, abs(theta) + math.sqrt(theta * theta + 1.0))
                    c = 1.0 / math.sqrt(t * t + 1.0)
                    sn = t * c
                    for k in range(n):                                   # a <- a J
                        akp, akq = a[n * k + p], a[n * k + q]
                        a[n * k + p] = c * akp - sn * akq
                        a[n * k + q] = sn * akp + c * akq
                    for k in range(n):                                   # a <- J^T a
                        apk, aqk = a[n * p + k], a[n * q + k]
                        a[n * p + k] = c * apk - sn * aqk
                        a[n * q + k] = sn * apk + c * aqk
                    a[n * p + q] = 0.0
                    a[n * q + p] = 0.0
                    if vectors:
                        for k in range(n):
                            vkp, vkq = v[n * k + p], v[n * k + q]
                            v[n * k + p] = c * vkp - sn * vkq
                            v[n * k + q] = sn * vkp + c * vkq
    return False, v


def algorithm(H, sigma2):
    """report_finish_h from `information` on: dict(eigenvalues, eigenvectors (rows), covariance, rank, settled)"""
    a = [float(x) for x in np.asarray(H, np.float64).reshape(36)]
    settled, V = jacobi_eigen(a, 6, True)
    lam = [a[7 * k] for k in range(6)]
    vec = [[V[6 * c + k] for c in range(6)] for k in range(6)]
    for sweep in range(5):
        for k in range(5 - sweep):
            if lam[k + 1] < lam[k]:
                lam[k], lam[k + 1] = lam[k + 1], lam[k]
                vec[k], vec[k + 1] = vec[k + 1], vec[k]
    for k in range(6):
        big = vec[k][0]
        for c in range(1, 6):
            if abs(vec[k][c]) > abs(big):
                big = vec[k][c]
        sign = -1.0 if big < 0.0 else 1.0
        vec[k] = [x * sign for x in vec[k]]
    sigma2 = float(sigma2)
    floor = FLOOR * lam[5]
    rank = sum(1 for x in lam if x > floor)
    inv = [_div(sigma2, x if x > floor else floor) for x in lam]
    cov = np.zeros((6, 6))
    for r in range(6):
        for c in range(r, 6):
            s = 0.0
            for k in range(6):
                s += inv[k] * (vec[k][r] * vec[k][c])
            cov[r, c] = cov[c, r] = s
    return dict(eigenvalues=np.array(lam), eigenvectors=np.array(vec), covariance=cov, rank=rank, settled=settled)


def algorithm_d(D):
    """report_finish_d's number: the smallest diagonal entry after jacobi_eigen<7, false> on D's upper triangle mirrored"""
    D = np.asarray(D, np.float64).reshape(7, 7)
    a = [0.0] * 49
    for i in range(7):
        for j in range(i, 7):
            a[7 * i + j] = a[7 * j + i] = float(D[i, j])
    settled, _ = jacobi_eigen(a, 7, False)
    dmin = a[0]
    for i in range(1, 7):
        if a[8 * i] < dmin:
            dmin = a[8 * i]
    return dmin, settled


def same_bits(a, b):
    return np.ascontiguousarray(a, np.float64).tobytes() == np.ascontiguousarray(b, np.float64).tobytes()


def mismatches(rep):
    """The fields of a device record (a dict as FeatureExtraction hands it out) that are not algorithm()'s bytes on the record's
    own information and sigma2; where sigma2 is NaN the covariance has to be NaN in every entry (a NaN's payload is not compared)"""
    alg = algorithm(rep["information"], rep["sigma2"])
    bad = [k for k in ("eigenvalues", "eigenvectors") if not same_bits(rep[k], alg[k])]
    if math.isnan(rep["sigma2"]):
        bad += [] if np.isnan(rep["covariance"]).all() else ["covariance"]
    elif not same_bits(rep["covariance"], alg["covariance"]):
        bad.append("covariance")
    if rep["rank"] != alg["rank"]:
        bad.append("rank")
    if bool(rep["valid"]) != alg["settled"]:
        bad.append("valid")
    return bad
