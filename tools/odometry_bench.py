"""tools/odometry_bench.py -- time of lfx_odometry_update_batch (Odometry::Update over EdgeSurfaceMap) on a
moving 64 x 1800 sequence, beside lfx_localize_batch's one-scan time in the same process and the oracle chain on one core.

  python3 tools/odometry_bench.py [--rings 64] [--cols 1800] [--scans 48] [--warmup 16] [--batches 1 16] [--cpu-scans 6]

Per batch size: a fresh odometry (n_local_scans 7, window grids of 1.0) takes `warmup` scans untimed, then the remaining
scans of the sequence in batches of that size; every update_batch is timed by HIP events around it on the stream (it waits
for its own alignments, so the span includes the host's part).  ms per scan = the sum of the spans / scans timed.  The
scans are extracted (untimed) before every call.  Localize: lfx_localize_batch of one scan against maps built from the last
odometry's window, warmed, the median of `--localize-reps` calls.  CPU: the odometry part of the oracle chain
(tests/odometry_restatement.py: transform, Downsample, Optimizer::Run with an exhaustive neighbour search; extraction not
counted) on the first `cpu-scans` scans.  Between warm-up and the timed calls the script calls hipMemGetInfo once, and once
after them: a HIP trace shows where the timed part begins and ends."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _marker():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    hip.hipMemGetInfo(C.byref(free), C.byref(total))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--cols", type=int, default=1800)
    ap.add_argument("--scans", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--localize-reps", type=int, default=20)
    ap.add_argument("--cpu-scans", type=int, default=6)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from lidar_feature_extraction_amd import FeatureExtraction, concat, make_sequence
    clouds, truth = make_sequence(a.scans, a.rings, a.cols, seed=9100)
    per = a.rings * a.cols
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    d_all = torch.from_numpy(concat(clouds).view(np.uint8).copy()).to(dev)      # every scan on the device before anything is timed
    B = max(a.batches)
    fx = FeatureExtraction(device=0, max_points_per_scan=per, max_batch=B, max_points_per_ring=a.cols, max_rings=a.rings)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def extract(lo, hi):
        fx.extract_batch_device(d_all.data_ptr() + lo * per * 32, [per] * (hi - lo), stream)

    out = dict(metric="odometry_update_batch", rings=a.rings, cols=a.cols, n_local_scans=7, scans=a.scans, warmup=a.warmup)
    odos = {}
    for b in a.batches:
        odo = fx.odometry(n_local_scans=7)
        for lo in range(0, a.warmup, b):           # warm-up, in batches of the same size (the buffers grow to the batch)
            hi = min(lo + b, a.warmup)
            extract(lo, hi)
            odo.update_batch(hi - lo, stream)
        odos[b] = odo
    _marker()                                      # (the timed part begins)
    final = None
    for b in a.batches:
        odo, spans, timed, aligned = odos[b], [], 0, 0
        for lo in range(a.warmup, a.scans, b):
            hi = min(lo + b, a.scans)
            extract(lo, hi)
            ev0.record()
            res = odo.update_batch(hi - lo, stream)
            ev1.record()
            ev1.synchronize()
            spans.append(ev0.elapsed_time(ev1))
            timed += hi - lo
            aligned += sum(r["aligned"] for r in res)
        out["batch_%d_ms_per_scan" % b] = sum(spans) / timed
        out["batch_%d_scans_timed" % b] = timed
        out["batch_%d_aligned" % b] = aligned
        final = odo
    _marker()                                      # (the timed part ends)
    # the last pose against the ground truth (a sanity check of what was timed)
    out["final_translation_error_m"] = float(np.linalg.norm(final.pose()[:, 3] - truth[-1][:, 3]))
    # lfx_localize_batch, one scan, against maps of the odometry's last window
    v = final.view()
    emap = fx.make_map(v["edge_window"], v["n_edge_window"], 1.0, stream)
    smap = fx.make_map(v["surface_window"], v["n_surface_window"], 1.0, stream)
    extract(a.scans - 1, a.scans)
    pose = final.pose()[None]
    for _ in range(3):
        fx.localize_batch(emap, smap, pose, 15, 20, 1.0, stream)
    loc = []
    for _ in range(a.localize_reps):
        ev0.record()
        fx.localize_batch(emap, smap, pose, 15, 20, 1.0, stream)
        ev1.record()
        ev1.synchronize()
        loc.append(ev0.elapsed_time(ev1))
    out["localize_batch_1_ms"] = float(np.median(loc))
    out["window_points"] = [int(v["n_edge_window"]), int(v["n_surface_window"])]
    emap.close()
    smap.close()
    for odo in odos.values():
        odo.close()
    fx.close()
    # the oracle chain's odometry part on one core
    if a.cpu_scans:
        from oracle import binding as OB
        from tests.odometry_restatement import EdgeSurfaceMap, Odometry, downsample, optimize_scan
        feats = [OB.extract(c, canonical_ties=False) for c in clouds[:a.cpu_scans]]

        def updater(recent):
            def run(scan, pose):
                return optimize_scan(recent[0], recent[1], 15, scan[0], downsample(scan[1], 1.0), pose, 20)["pose"]
            return run
        odo = Odometry(updater, EdgeSurfaceMap(7))
        odo.update((feats[0]["edge_points"], feats[0]["surface_points"]))     # (the first scan is only added)
        t0 = time.perf_counter()
        for f in feats[1:]:
            odo.update((f["edge_points"], f["surface_points"]))
        out["oracle_chain_ms_per_scan_one_core"] = (time.perf_counter() - t0) * 1e3 / (len(feats) - 1)
        out["oracle_chain_scans_timed"] = len(feats) - 1
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
