"""Times of the grid matcher (lfx_grid_match_*): 64 scans of `synth` 64 x 1800 records reduced to 1800 beams each and rendered
into a 4096 x 4096 occupancy grid of 0.1 m on a lap of a circle, the grid's distance field turned into a score field with
the default table, then scores and searches of the same scans; one JSON line.

    python tools/grid_match_bench.py [--side 4096] [--scans 64] [--out FILE] [--only CASE]

Medians of five after a warm-up, HIP events around the calls, all in microseconds:

  set_field_us            lfx_grid_match_set_field, beside floor_us: 6 bytes per cell (4 read, 2 written) at
                          lfx_box_calibration's copy rate
  search                  per window Nx x Ny x T and number of scans: the time, and point-candidate pairs per second (the
                          scans' kept points x Nx x Ny x T over the time); the centres are the scans' own poses, 3 cells off
  score_us                lfx_grid_match_score of P candidates around the scan's own pose, P = 4096 and 2^20, with pairs/s
  numpy_search_s          the numpy restatement's search of the smallest window for one scan, on the host: for scale
  --only CASE             run one search case alone (`101x101x61_64`, ...), ten times: what a counter run is pointed at"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lidar_feature_extraction_amd import FeatureExtraction, concat, grid_match_table, make_scan  # noqa: E402
from tools.keyframes_bench import circle  # noqa: E402

RUNS = 5
RES = 0.1
WINDOWS = [(10, 10, 0), (50, 50, 0), (50, 50, 30)]
THETA_STEP = 0.005


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    rings, cols, n, side = 64, 1800, a.scans, a.side
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    fx = FeatureExtraction(device=0, max_points_per_scan=rings * cols, max_batch=n, max_points_per_ring=cols, max_rings=rings)
    distinct = [make_scan(rings, cols, seed=7000 + k) for k in range(min(n, 8))]
    clouds = [distinct[k % len(distinct)] for k in range(n)]
    d_in = torch.from_numpy(np.ascontiguousarray(concat(clouds)).view(np.uint8).reshape(-1).copy()).to(dev)
    fx.extract_batch_device(d_in.data_ptr(), [len(c) for c in clouds], stream)
    poses = circle(n, spacing=1.0)

    def events(call):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        begin.record()
        call()
        end.record()
        torch.cuda.synchronize()
        return 1e3 * begin.elapsed_time(end)

    def median(call):
        took = [events(call) for _ in range(RUNS + 1)]
        return round(float(np.median(took[1:])), 1)                      # (the first run warms the kernels)

    half = 0.5 * side * RES
    line = dict(side=side, resolution=RES, scans=n, beams=1800, theta_step=THETA_STEP)
    line["copy_gb_s"] = [round(fx.box_calibration(0, stream)[0], 1) for _ in range(3)]
    line["floor_us"] = round(6.0 * side * side / (1e3 * float(np.median(line["copy_gb_s"]))), 1)
    g = fx.occupancy_grid(side, side, RES, (-half, -half), max_scans=n, n_beams=1800)
    g.add_batch(poses, stream=stream)
    g.render(stream=stream)
    df = fx.distance_field(side, side)
    df.from_occupancy(g, stream=stream)
    m = fx.grid_matcher(side, side, RES, (-half, -half), max_scans=n, max_beams=1800, max_half_x=50, max_half_y=50, max_half_theta=30)
    lut = grid_match_table(None, RES)
    line["table_cells"] = int(np.sqrt(len(lut) - 1))
    line["device_bytes"] = m.info()["device_bytes"]
    m.set_field(df, lut, stream=stream)
    m.set_scans_occupancy(g, stream=stream)
    pts = m.points(stream)
    line["points_per_scan"] = round(float(np.mean([len(p) for p in pts])), 1)
    stored = g.poses(stream=stream)
    # the scans' own poses, 3 cells off: the stored rotation is the level, so the heading searched for is 0
    centres = np.stack([stored[:, 0, 3] + 3 * RES, stored[:, 1, 3] - 3 * RES, np.zeros(n)], axis=1)

    def case(hx, hy, ht, k):
        cfg = dict(half_x=hx, half_y=hy, half_theta=ht, step_cells=1, theta_step=THETA_STEP if ht else 0.0)
        return cfg, "%dx%dx%d_%d" % (2 * hx + 1, 2 * hy + 1, 2 * ht + 1, k)

    if a.only:
        for hx, hy, ht in WINDOWS:
            for k in (1, n):
                cfg, name = case(hx, hy, ht, k)
                if name == a.only:
                    for _ in range(10):
                        m.search(centres[:k], cfg, stream=stream)
                    torch.cuda.synchronize()
                    print(json.dumps(dict(only=name, runs=10)))
        return
    line["set_field_us"] = median(lambda: m.set_field(df, lut, stream=stream))
    line["search"] = {}
    for hx, hy, ht in WINDOWS:
        for k in (1, n):
            cfg, name = case(hx, hy, ht, k)
            us = median(lambda: m.search(centres[:k], cfg, stream=stream))
            pairs = float(sum(len(p) for p in pts[:k])) * (2 * hx + 1) * (2 * hy + 1) * (2 * ht + 1)
            line["search"][name] = dict(us=us, pairs_per_s=float("%.4g" % (pairs / (us * 1e-6))))
    line["score_us"] = {}
    rng = np.random.default_rng(1)
    for P in (4096, 1 << 20):
        ang = rng.uniform(-0.2, 0.2, P)
        cand = torch.from_numpy(np.stack([stored[0, 0, 3] + rng.uniform(-3, 3, P), stored[0, 1, 3] + rng.uniform(-3, 3, P), np.cos(ang), np.sin(ang)],
                                         axis=1)).to(dev)
        us = median(lambda: m.score(0, cand, stream=stream))
        line["score_us"][str(P)] = dict(us=us, pairs_per_s=float("%.4g" % (len(pts[0]) * P / (us * 1e-6))))
    from tests import grid_match_restatement as G
    Sh = m.field(stream)
    geom = G.geometry(side, side, RES, -half, -half)
    t0 = time.perf_counter()
    G.search(Sh, pts[:1], centres[:1], G.search_config(half_x=10, half_y=10), geom)
    line["numpy_search_s"] = round(time.perf_counter() - t0, 3)
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    for o in (m, df, g):
        o.close()
    fx.close()


if __name__ == "__main__":
    main()
