#!/usr/bin/env python3
"""tools/long_ring_bench.py [--batch 64] [--steps 20] [--json PATH] -- throughput of rings longer than LFX_MAX_RING_POINTS
(the long-ring kernel) against the CPU oracle on one core, in the same run.

Per shape: scans/s and ms per scan of lfx_extract_batch_device at the given batch (device-resident input, timed with
events over --steps batches after a warm-up); every kernel's time per batch from lfx_kernel_times; for a shuffled shape
the same scans in angle order as well, so that the long-ring kernel's time splits into its angle sort and the rest.  The
batch's first scan is checked against the oracle."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (make_scan emits column-major grids: "16x8192 grid" is a driver's organised scan, which the organised route gives up)
SHAPES = [("4x5000 shuffled", 4, 5000, True), ("6x8000", 6, 8000, False), ("1x100000 shuffled", 1, 100000, True),
          ("16x8192 grid", 16, 8192, False)]


def run_shape(name, rings, cols, shuffle, batch, steps):
    import torch
    from lidar_feature_extraction_amd import FeatureExtraction, make_scan, synth
    from oracle import binding as OB
    from tests.parity import assert_scan_equal
    clouds = [make_scan(rings, cols, seed=5000 + i, shuffle=shuffle) for i in range(batch)]
    # the oracle on one core: the median of a few scans
    ts = []
    for c in clouds[:3]:
        t = time.perf_counter()
        OB.extract(c, canonical_ties=True)
        ts.append(time.perf_counter() - t)
    oracle_ms = 1e3 * float(np.median(ts))
    out = {"shape": name, "batch": batch, "points_per_scan": rings * cols, "oracle_ms_per_scan": round(oracle_ms, 2)}
    variants = [("", clouds)]
    if shuffle:
        variants.append(("sorted_", [make_scan(rings, cols, seed=5000 + i) for i in range(batch)]))
    for tag, cl in variants:
        f = FeatureExtraction(device=0, max_points_per_scan=rings * cols, max_batch=batch, max_points_per_ring=cols,
                              max_rings=rings)
        stream = torch.cuda.current_stream().cuda_stream
        dev = torch.from_numpy(synth.concat(cl).view(np.uint8).copy()).to("cuda:0")
        n = [len(c) for c in cl]
        for _ in range(3):
            f.extract_batch_device(dev.data_ptr(), n, stream)
        torch.cuda.synchronize()
        if tag == "":
            assert_scan_equal(f.download(0, stream), OB.extract(cl[0], canonical_ties=True), name)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            f.extract_batch_device(dev.data_ptr(), n, stream)
        b.record()
        torch.cuda.synchronize()
        ms_batch = a.elapsed_time(b) / steps
        f.set_profiling(True, every=1)
        for _ in range(max(2, steps // 4)):
            f.extract_batch_device(dev.data_ptr(), n, stream)
        torch.cuda.synchronize()
        kt = {k: round(1e3 * ms / cnt, 1) for k, (ms, cnt) in f.kernel_times().items() if cnt}
        f.set_profiling(False)
        f.close()
        out[tag + "ms_per_batch"] = round(ms_batch, 3)
        out[tag + "ms_per_scan"] = round(ms_batch / batch, 4)
        out[tag + "scans_per_s"] = round(1e3 * batch / ms_batch, 1)
        out[tag + "kernel_us_per_batch"] = kt
    out["speedup_vs_oracle_per_scan"] = round(oracle_ms / out["ms_per_scan"], 1)
    if shuffle:
        lk, lks = out["kernel_us_per_batch"].get("ring_long_kernel", 0.0), out["sorted_kernel_us_per_batch"].get("ring_long_kernel", 0.0)
        out["long_kernel_us_sort"] = round(lk - lks, 1)
        out["long_kernel_us_label_and_rest"] = lks
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    for s in SHAPES:
        r = run_shape(*s, batch=a.batch, steps=a.steps)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
