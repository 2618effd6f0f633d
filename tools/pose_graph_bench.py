"""Times of lfx_pose_graph_optimize on a two-lap circle with N nodes and L loop closures: per call (wall clock, profiling off)
and per kernel (lfx_kernel_times: HIP events around every launch, profiling on), one JSON line per size.

    python tools/pose_graph_bench.py [--sizes 1000x10,10000x100,10000x512] [--runs 3] [--out FILE]

The graph: radius 20 m, chained odometry with noise 0.002 rad / 0.01 m, the start its composition, loop closures from the first
lap to the second.  Every run starts from the same chained poses (set_poses), so the iterations are the same each time.
share_chain_factor: the sequential block factorisation's part of the kernels' time."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lidar_feature_extraction_amd import FeatureExtraction, pose_graph_edges  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000x10,10000x100,10000x512")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fx = FeatureExtraction(device=0, max_points_per_scan=1024, max_batch=1)
    lines = []
    for size in a.sizes.split(","):
        n, loops = (int(v) for v in size.split("x"))
        start, truth, edges = circle(n, loops)
        pg = fx.pose_graph(n, len(edges), max_loop_edges=max(loops, 1))
        pg.add_nodes(start)
        pg.add_edges(edges)
        res = pg.optimize()                         # (warm: the kernels' first launches)
        err = lambda p: float(np.linalg.norm(p[:, :, 3] - truth[:, :, 3], axis=1).max())     # noqa: E731
        line = dict(nodes=n, loop_edges=loops, code=res["code"], iterations=res["iterations"], chi2_initial=res["chi2_initial"],
                    chi2_final=res["chi2_final"], worst_error_before_m=err(start), worst_error_after_m=err(pg.poses()),
                    device_bytes=pg.info()["device_bytes"], call_ms=[], kernels_ms_per_call=[], share_chain_factor=[])
        for _ in range(a.runs):
            pg.set_poses(start)
            pg.poses(0, 1)                          # (the upload has landed)
            t0 = time.perf_counter()
            pg.optimize()
            line["call_ms"].append(round(1e3 * (time.perf_counter() - t0), 3))
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
