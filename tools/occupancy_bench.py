"""Times of the occupancy grid (lfx_occupancy_*): N scans of `synth` 64 x 1800 records reduced to W = 1800 beams each and
rendered into a 4096 x 4096 grid of 0.1 m, on two laps of a circle; one JSON line.

    python tools/occupancy_bench.py [--scans 1024] [--batch 256] [--beams 1800] [--side 4096] [--chunk 32] [--out FILE]

Medians of five after a warm-up, HIP events around the calls:

  add_batch_us       lfx_occupancy_add_batch of one batch of --batch scans (every record line read once, binned by azimuth, two
                     64-bit atomics' worth of candidates), and beside it
  scan_context_us    lfx_scan_context_batch of the same batch, which reads the same records and bins them the same way;
                     both with the GB/s of the batch's 32-byte records, beside lfx_box_calibration's copy rate
  render_us          lfx_occupancy_clear + lfx_occupancy_render of all N scans, with the counters' vote totals: votes per second
                     is what stands beside the voxel filter's scattered-atomic rate
  emit_us            lfx_occupancy_emit of the whole grid to device memory"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lidar_feature_extraction_amd import FeatureExtraction, concat, make_scan  # noqa: E402
from tools.keyframes_bench import circle  # noqa: E402

RUNS = 5


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--beams", type=int, default=1800)
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--resolution", type=float, default=0.1)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rings, cols, n, batch = 64, 1800, a.scans, min(a.batch, a.scans)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    fx = FeatureExtraction(device=0, max_points_per_scan=rings * cols, max_batch=batch, max_points_per_ring=cols, max_rings=rings)
    distinct = [make_scan(rings, cols, seed=7000 + k) for k in range(min(batch, 8))]
    clouds = [distinct[k % len(distinct)] for k in range(batch)]
    d_in = torch.from_numpy(np.ascontiguousarray(concat(clouds)).view(np.uint8).reshape(-1).copy()).to(dev)
    fx.extract_batch_device(d_in.data_ptr(), [len(c) for c in clouds], stream)
    records = sum(len(c) for c in clouds)
    poses = circle(n, spacing=0.25)
    half = 0.5 * a.side * a.resolution
    line = dict(scans=n, batch=batch, beams=a.beams, side=a.side, resolution=a.resolution, chunk_scans=a.chunk, batch_records=records)

    def events(call):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        begin.record()
        call()
        end.record()
        torch.cuda.synchronize()
        return 1e3 * begin.elapsed_time(end)

    def median(call, before=None):
        took = []
        for _ in range(RUNS + 1):
            if before:
                before()
            took.append(events(call))
        return round(float(np.median(took[1:])), 1)                      # (the first run warms the kernels)

    line["copy_gb_s"] = [round(fx.box_calibration(0, stream)[0], 1) for _ in range(3)]
    desc = fx.scan_context(stream=stream)
    line["scan_context_us"] = median(lambda: fx.scan_context(out=desc.data_ptr(), stream=stream))
    line["scan_context_gb_s"] = round(32.0 * records / (1e3 * line["scan_context_us"]), 1)

    # the add: a grid of its own with room for one batch, emptied by making it again (create is not timed)
    holder = {}

    def fresh():
        if "g" in holder:
            holder["g"].close()
        holder["g"] = fx.occupancy_grid(64, 64, a.resolution, (-half, -half), max_scans=batch, n_beams=a.beams, chunk_scans=a.chunk)

    line["add_batch_us"] = median(lambda: holder["g"].add_batch(poses[:batch], stream=stream), before=fresh)
    line["add_batch_gb_s"] = round(32.0 * records / (1e3 * line["add_batch_us"]), 1)
    line["add_over_scan_context"] = round(line["add_batch_us"] / line["scan_context_us"], 2)
    holder["g"].close()

    g = fx.occupancy_grid(a.side, a.side, a.resolution, (-half, -half), max_scans=n, n_beams=a.beams, chunk_scans=a.chunk)
    for first in range(0, n, batch):
        m = min(batch, n - first)
        sel = np.zeros(batch, np.uint8)
        sel[:m] = 1
        g.add_batch(np.concatenate([poses[first:first + m], poses[:batch - m]]), sel, stream=stream)
    torch.cuda.synchronize()
    info = g.info()
    line["device_bytes"], line["window"] = info["device_bytes"], info["window"]

    def render():
        g.clear(stream)
        g.render(stream=stream)

    line["render_us"] = median(render)
    c = g.counters(stream)
    line["counters"] = c
    votes = c["n_occupied_votes"] + c["n_free_votes"]
    line["votes_per_us"] = round(votes / line["render_us"], 1)
    line["beams_per_us"] = round((c["n_hit_beams"] + c["n_clear_beams"]) / line["render_us"], 1)
    out = g.emit(stream=stream)
    line["emit_us"] = median(lambda: g.emit(out=out.data_ptr(), stream=stream))
    line["emit_gb_s"] = round(9.0 * a.side * a.side / (1e3 * line["emit_us"]), 1)
    grid = out.cpu().numpy()
    line["cells"] = dict(unknown=int((grid == -1).sum()), free=int(((grid >= 0) & (grid <= 25)).sum()), occupied=int((grid >= 65).sum()))
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    g.close()
    fx.close()


if __name__ == "__main__":
    main()
