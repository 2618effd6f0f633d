"""Times of lfx_pose_graph_optimize on a two-lap circle with N nodes and L loop closures: per call (wall clock, profiling off)
and per kernel (lfx_kernel_times: HIP events around every launch, profiling on), one JSON line per size.

    python tools/pose_graph_bench.py [--sizes 1000x10,10000x100,10000x512] [--runs 3] [--out FILE]
                                     [--priors P [--pose [--anchored]]] [--marginals]

The graph: radius 20 m, chained odometry with noise 0.002 rad / 0.01 m, the start its composition, loop closures from the first
lap to the second.  Every run starts from the same chained poses (set_poses), so the iterations are the same each time.
share_chain_factor: the sequential block factorisation's part of the kernels' time.
--priors P: P robust position fixes (sigma 0.05 m) spread evenly over the nodes, of an antenna at the lever (0.8, -0.2, 1.5);
with --pose, P robust pose fixes instead (0.01 rad, 0.05 m).  --anchored (with --pose): the same fixes as the graph had to
take them before priors existed -- an extra fixed node at the identity first, every id shifted by one, every fix an edge
from that node: P - 1 more loop edges.  (A position fix has no anchored form: its Omega = blkdiag(0, Omega_t) is singular,
and a loop edge's information must have a Cholesky factor.)
--marginals: beside every timed optimise, the covariances that follow it (wall clock): marginals_first_ms, the first
lfx_pose_graph_marginals call, which does the whole graph's work and copies every block; marginals_again_ms, the same call
once more (a copy); joint_64_ms, 64 pairs half a trajectory apart (i, i + N / 2), the longest products there are."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lidar_feature_extraction_amd import FeatureExtraction, pose_graph_edges, pose_graph_priors  # noqa: E402

LEVER = np.array([0.8, -0.2, 1.5])
SIGMA_FIX, SIGMA_FIX_ROT = 0.05, 0.01


def planar(yaw, x, y):
    T = np.zeros((len(yaw), 3, 4))
    T[:, 0, 0], T[:, 0, 1], T[:, 1, 0], T[:, 1, 1], T[:, 2, 2] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw), 1.0
    T[:, 0, 3], T[:, 1, 3] = x, y
    return T


def between(A, B):
    Z = np.zeros_like(A)
    Z[:, :, :3] = np.einsum("kji,kjl->kil", A[:, :, :3], B[:, :, :3])
    Z[:, :, 3] = np.einsum("kji,kj->ki", A[:, :, :3], B[:, :, 3] - A[:, :, 3])
    return Z


def circle(n, loops, seed=1, radius=20.0, sigma=(0.002, 0.01)):
    rng = np.random.default_rng(seed)
    ang = 4.0 * np.pi * np.arange(n) / n
    truth = planar(ang + np.pi / 2, radius * np.cos(ang), radius * np.sin(ang))
    half = n // 2
    li = (np.floor((np.arange(loops) + 0.5) * half / loops).astype(np.int64)) % half
    i = np.concatenate([np.arange(n - 1), li])
    j = np.concatenate([np.arange(1, n), li + half])
    Z = between(truth[i], truth[j])
    jitter = planar(sigma[0] * rng.standard_normal(len(i)), sigma[1] * rng.standard_normal(len(i)), sigma[1] * rng.standard_normal(len(i)))
    Zn = np.zeros_like(Z)
    Zn[:, :, :3] = Z[:, :, :3] @ jitter[:, :, :3]
    Zn[:, :, 3] = np.einsum("kij,kj->ki", Z[:, :, :3], jitter[:, :, 3]) + Z[:, :, 3]
    om = np.diag([1.0 / sigma[0] ** 2] * 3 + [1.0 / sigma[1] ** 2] * 3)
    start = np.zeros_like(truth)
    start[0] = truth[0]
    for k in range(n - 1):
        start[k + 1, :, :3] = start[k, :, :3] @ Zn[k, :, :3]
        start[k + 1, :, 3] = start[k, :, :3] @ Zn[k, :, 3] + start[k, :, 3]
    return start, truth, pose_graph_edges(i, j, Zn, np.broadcast_to(om, (len(i), 6, 6)))


def fixes(truth, count, lever, seed=2):
    """(nodes [count], the antenna's measured places [count][3]): spread evenly over the trajectory"""
    rng = np.random.default_rng(seed)
    nodes = (np.arange(count) * len(truth)) // count
    at = truth[nodes, :, 3] + truth[nodes, :, :3] @ lever
    return nodes, at + SIGMA_FIX * rng.standard_normal((count, 3))


def pose_fixes(truth, count, seed=2):
    """(nodes [count], measured poses [count][3][4], information [count][6][6]): the true poses, the yaw and the place with noise"""
    rng = np.random.default_rng(seed)
    nodes = (np.arange(count) * len(truth)) // count
    Z = truth[nodes].copy()
    Z[:, :, :3] = Z[:, :, :3] @ planar(SIGMA_FIX_ROT * rng.standard_normal(count), 0.0, 0.0)[:, :, :3]
    Z[:, :, 3] += SIGMA_FIX * rng.standard_normal((count, 3))
    om = np.diag([1.0 / SIGMA_FIX_ROT ** 2] * 3 + [1.0 / SIGMA_FIX ** 2] * 3)
    return nodes, Z, np.broadcast_to(om, (count, 6, 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000x10,10000x100,10000x512")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--priors", type=int, default=0)
    ap.add_argument("--pose", action="store_true")
    ap.add_argument("--anchored", action="store_true")
    ap.add_argument("--marginals", action="store_true")
    a = ap.parse_args()
    if a.anchored and not (a.priors and a.pose):
        ap.error("--anchored needs --priors and --pose")
    fx = FeatureExtraction(device=0, max_points_per_scan=1024, max_batch=1)
    lines = []
    for size in a.sizes.split(","):
        n, loops = (int(v) for v in size.split("x"))
        start, truth, edges = circle(n, loops)
        if a.priors and a.pose:
            nodes, Z, full = pose_fixes(truth, min(a.priors, n))
            priors = pose_graph_priors(nodes, Z, full, robust=True)
        elif a.priors:
            nodes, at = fixes(truth, min(a.priors, n), LEVER)
            priors = pose_graph_priors(nodes, at, np.broadcast_to(np.eye(3) / SIGMA_FIX ** 2, (len(nodes), 3, 3)), LEVER, position=True, robust=True)
        if a.anchored:
            identity = np.zeros((1, 3, 4))
            identity[0, :, :3] = np.eye(3)
            edges = edges.copy()
            edges["i"] += 1
            edges["j"] += 1
            edges = np.concatenate([edges, pose_graph_edges(np.zeros(len(nodes), np.int64), nodes + 1, Z, full, 1)])
            start, truth = np.concatenate([identity, start]), np.concatenate([identity, truth])
            pg = fx.pose_graph(n + 1, len(edges), max_loop_edges=loops + len(nodes))
            pg.add_nodes(start)
            pg.set_fixed(1, True)
            pg.add_edges(edges)
        else:
            pg = fx.pose_graph(n, len(edges), max_loop_edges=max(loops, 1))
            pg.add_nodes(start)
            pg.add_edges(edges)
            if a.priors:
                pg.reserve_priors(len(nodes))
                pg.add_priors(priors)
        if a.marginals:
            pg.reserve_marginals()
            base = (np.arange(64) * (n // 2)) // 64
            pairs = np.stack([base, base + n // 2], axis=1).astype(np.uint32)
        res = pg.optimize()                         # (warm: the kernels' first launches)
        if a.marginals:
            pg.marginals()
            pg.joint_covariances(pairs)
        err = lambda p: float(np.linalg.norm(p[:, :, 3] - truth[:, :, 3], axis=1).max())     # noqa: E731
        line = dict(nodes=n, loop_edges=res["n_loop"], priors=pg.prior_info()["n_priors"], anchored=bool(a.anchored), code=res["code"], iterations=res["iterations"], chi2_initial=res["chi2_initial"],
                    chi2_final=res["chi2_final"], worst_error_before_m=err(start), worst_error_after_m=err(pg.poses()),
                    device_bytes=pg.info()["device_bytes"], call_ms=[], kernels_ms_per_call=[], share_chain_factor=[])
        for _ in range(a.runs):
            pg.set_poses(start)
            pg.poses(0, 1)                          # (the upload has landed)
            t0 = time.perf_counter()
            pg.optimize()
            line["call_ms"].append(round(1e3 * (time.perf_counter() - t0), 3))
            if a.marginals:
                for key, call in (("marginals_first_ms", pg.marginals), ("marginals_again_ms", pg.marginals),
                                  ("joint_64_ms", lambda: pg.joint_covariances(pairs))):
                    t0 = time.perf_counter()
                    call()
                    line.setdefault(key, []).append(round(1e3 * (time.perf_counter() - t0), 3))
        for _ in range(a.runs):
            pg.set_poses(start)
            fx._L.lfx_set_profiling(fx._ctx, 1)
            pg.optimize()
            kt = {k: (ms, cnt) for k, (ms, cnt) in fx.kernel_times().items() if k.startswith("pose_graph_") and cnt}
            fx._L.lfx_set_profiling(fx._ctx, 0)
            total = sum(ms for ms, _ in kt.values())
            line["kernels_ms_per_call"].append({k.replace("pose_graph_", "").replace("_kernel", ""): [round(ms, 3), cnt] for k, (ms, cnt) in kt.items()})
            line["share_chain_factor"].append(round(kt["pose_graph_chain_factor_kernel"][0] / total, 4))
        pg.close()
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    fx.close()


if __name__ == "__main__":
    main()
