"""tools/rolling_map_bench.py -- times of the rolling voxel map (lfx_rolling_map_*) on a moving 64 x 1800 sequence at the
default config (leaves 0.2 / 0.4, windows of 102.4 x 102.4 x 25.6 m, match boxes of +-50, 50, 12.8 m), beside
lfx_odometry_update_batch on the same scans in the same process.

  python3 tools/rolling_map_bench.py [--rings 64] [--cols 1800] [--scans 48] [--warmup 16] [--batches 1 16] [--reps 20]

update_batch: per batch size a fresh odometry and a fresh rolling map take `warmup` scans untimed, then the remaining scans
in batches of that size, the odometry's poses handed to the map; each of the two calls is timed by HIP events around it on
the stream (both wait for their own alignments, so a span includes the host's part).  ms per scan = the sum of the spans /
scans timed.  The scans are extracted (untimed) before every pair of calls.  insert: lfx_rolling_map_insert of one scan's
edge and surface clouds (both stores) into the last map, the median of `reps` calls -- after the first one every record
merges, which costs what an insert into an empty voxel costs but for the winners' stores.  extract: lfx_rolling_map_extract
of the match box around the last pose, per kind, into a buffer that holds it, the median of `reps` calls; the box's cells (one
8-byte key read each) are reported with it."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--cols", type=int, default=1800)
    ap.add_argument("--scans", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from lidar_feature_extraction_amd import FeatureExtraction, concat, make_sequence
    clouds, truth = make_sequence(a.scans, a.rings, a.cols, seed=9100)
    per = a.rings * a.cols
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    d_all = torch.from_numpy(concat(clouds).view(np.uint8).copy()).to(dev)      # every scan on the device before anything is timed
    fx = FeatureExtraction(device=0, max_points_per_scan=per, max_batch=max(a.batches), max_points_per_ring=a.cols, max_rings=a.rings)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]

    def extract(lo, hi):
        fx.extract_batch_device(d_all.data_ptr() + lo * per * 32, [per] * (hi - lo), stream)

    out = dict(metric="rolling_map_update_batch", rings=a.rings, cols=a.cols, scans=a.scans, warmup=a.warmup)
    rm = None
    for b in a.batches:
        if rm is not None:
            rm.close()
        odo, rm = fx.odometry(n_local_scans=7), fx.rolling_map()
        spans_o, spans_m, timed, aligned = [], [], 0, 0
        spans = [(lo, min(lo + b, a.warmup)) for lo in range(0, a.warmup, b)] + [(lo, min(lo + b, a.scans)) for lo in range(a.warmup, a.scans, b)]
        for lo, hi in spans:
            extract(lo, hi)
            ev[0].record()
            poses = np.stack([r["pose"] for r in odo.update_batch(hi - lo, stream)])
            ev[1].record()
            res = rm.update_batch(poses, hi - lo, stream)
            ev[2].record()
            ev[2].synchronize()
            if lo >= a.warmup:
                spans_o.append(ev[0].elapsed_time(ev[1]))
                spans_m.append(ev[1].elapsed_time(ev[2]))
                timed += hi - lo
                aligned += sum(r["aligned"] and r["inserted"] for r in res)
        out["batch_%d_map_ms_per_scan" % b] = sum(spans_m) / max(timed, 1)
        out["batch_%d_odometry_ms_per_scan" % b] = sum(spans_o) / max(timed, 1)
        out["batch_%d_scans_timed" % b] = timed
        out["batch_%d_placed" % b] = aligned
        out["batch_%d_map_translation_error_m" % b] = float(np.linalg.norm(rm.pose()[:, 3] - truth[-1][:, 3]))
        out["batch_%d_odometry_translation_error_m" % b] = float(np.linalg.norm(odo.pose()[:, 3] - truth[-1][:, 3]))
        odo.close()
    view = rm.view(stream)
    out["live_voxels"] = [int(view["edge"]["live"]), int(view["surface"]["live"])]
    # insert: the last scan's two clouds into both stores
    extract(a.scans - 1, a.scans)
    pose = rm.pose()[None]
    spans = []
    for _ in range(a.reps + 3):
        ev[0].record()
        rm.insert_batch("edge", pose, stream)
        rm.insert_batch("surface", pose, stream)
        ev[1].record()
        ev[1].synchronize()
        spans.append(ev[0].elapsed_time(ev[1]))
    out["insert_scan_ms"] = float(np.median(spans[3:]))
    # extract: the match box around the last pose
    t = rm.pose()[:, 3]
    half = np.asarray(rm.config["match_half_extent"], np.float64)
    for kind in ("edge", "surface"):
        n = rm.extract_device(kind, t - half, t + half, 0, 0, stream)
        buf = torch.empty((max(n, 1), 4), dtype=torch.float32, device=dev)
        spans = []
        for _ in range(a.reps + 3):
            ev[0].record()
            rm.extract_device(kind, t - half, t + half, buf.data_ptr(), n, stream)
            ev[1].record()
            ev[1].synchronize()
            spans.append(ev[0].elapsed_time(ev[1]))
        leaf, o, dims = float(view[kind]["leaf"]), view[kind]["origin"], view[kind]["dims"]
        cells = 1
        for ax in range(3):
            first = max(int(np.floor((t[ax] - half[ax]) / leaf)), o[ax])
            last = min(int(np.floor((t[ax] + half[ax]) / leaf)), o[ax] + dims[ax] - 1)
            cells *= max(last - first + 1, 0)
        out["extract_%s_ms" % kind] = float(np.median(spans[3:]))
        out["extract_%s_points" % kind] = n
        out["extract_%s_box_cells" % kind] = cells
    rm.close()
    fx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
