#!/usr/bin/env python3
"""tools/make_ref_pieces_hashes.py -- writes tests/golden/reference_pieces_hashes.json: SHA-256 of what the reference's own
math.cpp / convolution.cpp / index_range.cpp (oracle/_ref, built by `make -C oracle ref` where the reference's sources
are) return on the seeded inputs of tests/test_oracle_reference_vectors.py::test_ref_pieces_bit_exact.  That test needs
the compiled pieces; with these hashes tests/test_oracle_reference_vectors.py::test_ref_pieces_stored_hashes pins the
oracle to the same outputs bit for bit on any checkout.  The inputs are hashed too (another numpy may draw other numbers,
and then the outputs say nothing).  Re-run only where oracle/_ref is built."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import binding as B      # noqa: E402

PD, PI = C.POINTER(C.c_double), C.POINTER(C.c_int)
PATH = os.path.join(ROOT, "tests", "golden", "reference_pieces_hashes.json")


def sha(parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


def pieces(R=None):
    """The hashes of the oracle's outputs (R None) or of the compiled reference pieces' (R = B.ref_pieces()), inputs drawn
    as test_ref_pieces_bit_exact draws them; an output is hashed only where its call returned 0, as the test compares it."""
    L = B.lib()
    rng = np.random.default_rng(1)
    ins, out = [], {k: [] for k in ("xy_norm", "calc_radian", "convolution1d", "curvature", "padded_index_range")}
    # XYNorm / CalcRadian on float-valued inputs, including degenerate ones
    v = rng.normal(0, 30, size=(20000, 4)).astype(np.float32).astype(np.float64)
    v[:50, :2] = 0.0
    v[50:100, 2:] = 0.0
    v[100:150] = 0.0
    v[150:200, 2:] = v[150:200, :2] * 3.0
    ins.append(v)
    for a in v:
        out["xy_norm"].append(np.float64(R.ref_xy_norm(a[0], a[1]) if R else L.orc_xy_norm(a[0], a[1])))
        o = C.c_double(0)
        rc = R.ref_calc_radian(*a, C.byref(o)) if R else L.orc_calc_radian(*a, C.byref(o))
        out["calc_radian"] += [np.int64(rc), np.float64(o.value if rc == 0 else 0.0)]
    # Convolution1D with curvature weights; the curvature is the convolution squared
    for pad in (1, 2, 3, 5, 8):
        w = np.zeros(2 * pad + 1)
        L.orc_make_weight(pad, B.ptr(w, PD))
        ins.append(w)
        for n in (2 * pad, 2 * pad + 1, 64, 257):
            r = np.abs(rng.normal(20, 15, n))
            ins.append(r)
            o = np.zeros(n)
            conv = R.ref_convolution1d if R else L.orc_convolution1d
            rc = conv(B.ptr(r, PD), n, B.ptr(w, PD), len(w), B.ptr(o, PD))
            out["convolution1d"] += [np.int64(rc), o if rc == 0 else np.zeros(0)]
            if rc == 0:
                c = o * o
                if not R:
                    c = np.zeros(n)
                    assert L.orc_calc_curvature(B.ptr(r, PD), n, pad, B.ptr(c, PD)) == 0
                out["curvature"].append(c)
    # PaddedIndexRange boundaries over a sweep of sizes
    for pad in (1, 2, 5):
        for nb in (1, 3, 6, 7):
            for size in list(range(2 * pad, 2 * pad + 40)) + [900, 1800, 2048, 4001]:
                b = np.zeros(nb + 1, np.int32)
                rc = (R.ref_padded_index_range if R else L.orc_padded_index_range)(size, nb, pad, B.ptr(b, PI))
                out["padded_index_range"] += [np.int64(rc), b if rc == 0 else np.zeros(0, np.int32)]
    return dict(input=sha(ins), **{k: sha(p) for k, p in out.items()})


if __name__ == "__main__":
    R = B.ref_pieces()
    if R is None:
        sys.exit("oracle/_ref is not built: `make -C oracle ref` where the reference's sources are")
    want = pieces(R)
    assert pieces() == want, "the oracle does not match the reference pieces: fix the oracle before freezing their outputs"
    json.dump({"note": "tools/make_ref_pieces_hashes.py: SHA-256 of the reference pieces' outputs (oracle/_ref) on the seeded inputs of "
                       "test_ref_pieces_bit_exact", "hashes": want}, open(PATH, "w"), indent=1)
    print("wrote", PATH)
