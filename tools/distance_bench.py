"""Times of the distance field (lfx_distance_*): N scans of `synth` 64 x 1800 records rendered into a SIDE x SIDE occupancy
grid of 0.1 m on a lap of a circle, then the grid's distance field, costmap and metres; one JSON line per side.

    python tools/distance_bench.py [--sides 4096,16384] [--scans 256] [--out FILE]

Medians of five after a warm-up, HIP events around the calls, all in microseconds:

  emit_us                 lfx_occupancy_emit of the grid to device memory: what every transform below stands beside
  floor_us                17 bytes per cell (8 read, 1 + 2 written, 2 read, 4 written) at lfx_box_calibration's copy rate
  from_occupancy_us       lfx_distance_from_occupancy of the rendered grid, by case: cap12 and cap6 (Rc of the default cost
                          config at 0.05 m and at 0.1 m: the outward search), uncapped (the envelope kernel), each without and
                          with `inside`
  adversarial_us          lfx_distance_from_grid, uncapped, of a grid whose only obstacle is the cell (0, 0)
  adversarial_row_us      ... of a grid whose row 0 is all obstacles and nothing else: every column's distance grows with y
  costmap_us, metres_us   of the cap6 transform, to device memory
  scipy_edt_s             scipy.ndimage.distance_transform_edt of the same grid on the host (sides up to 4096, if scipy
                          imports), beside cap12"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lidar_feature_extraction_amd import FeatureExtraction, concat, distance_cost_table, make_scan  # noqa: E402
from tools.keyframes_bench import circle  # noqa: E402

RUNS = 5
RES = 0.1


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", default="4096,16384")
    ap.add_argument("--scans", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rings, cols, n = 64, 1800, a.scans
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

    caps = dict(cap12=int(np.sqrt(len(distance_cost_table(None, 0.05)) - 1)), cap6=int(np.sqrt(len(distance_cost_table(None, 0.1)) - 1)), uncapped=0)
    lines = []
    for side in [int(s) for s in a.sides.split(",")]:
        half = 0.5 * side * RES
        line = dict(side=side, resolution=RES, scans=n, caps=caps)
        line["copy_gb_s"] = [round(fx.box_calibration(0, stream)[0], 1) for _ in range(3)]
        line["floor_us"] = round(17.0 * side * side / (1e3 * float(np.median(line["copy_gb_s"]))), 1)
        g = fx.occupancy_grid(side, side, RES, (-half, -half), max_scans=n, n_beams=1800)
        g.add_batch(poses, stream=stream)
        g.render(stream=stream)
        out = g.emit(stream=stream)
        line["emit_us"] = median(lambda: g.emit(out=out.data_ptr(), stream=stream))
        df = fx.distance_field(side, side)
        line["device_bytes"] = df.info()["device_bytes"]
        line["from_occupancy_us"] = {}
        for name, cap in caps.items():
            for inside in (0, 1):
                key = name + ("_inside" if inside else "")
                line["from_occupancy_us"][key] = median(lambda: df.from_occupancy(g, stream=stream, max_cells=cap, inside=inside))
                if not inside:
                    line.setdefault("stats", {})[name] = df.stats(stream)
        df.from_occupancy(g, stream=stream, max_cells=caps["cap6"])
        cost, metres = df.costmap(RES, stream=stream), df.metres(RES, stream=stream)
        line["costmap_us"] = median(lambda: df.costmap(RES, out=cost.data_ptr(), stream=stream))
        line["metres_us"] = median(lambda: df.metres(RES, out=metres.data_ptr(), stream=stream))
        torch.cuda.synchronize()
        line["cost_cells"] = dict(lethal=int((cost == 254).sum()), inflated=int(((cost > 0) & (cost < 254)).sum()), unknown=int((cost == 255).sum()))
        del cost, metres
        if side <= 4096:
            try:
                from scipy import ndimage
                grid = out.cpu().numpy()
                t0 = time.perf_counter()
                ndimage.distance_transform_edt(grid < 65)
                line["scipy_edt_s"] = round(time.perf_counter() - t0, 2)
            except ImportError:
                line["scipy_edt_s"] = None
        # the adversarial grids, through from_grid
        corner = torch.zeros((side, side), dtype=torch.int8, device=dev)
        corner[0, 0] = 100
        line["adversarial_us"] = median(lambda: df.from_grid(corner, stream=stream))
        line["adversarial_stats"] = df.stats(stream)
        corner[0, :] = 100
        line["adversarial_row_us"] = median(lambda: df.from_grid(corner, stream=stream))
        del corner, out
        df.close()
        g.close()
        text = json.dumps(line)
        print(text, flush=True)
        lines.append(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    fx.close()


if __name__ == "__main__":
    main()
