"""Times of the visibility votes (lfx_visibility_run) and of the masked build (lfx_keyframes_build_masked): a store of N
keyframes whose per-keyframe clouds come from a real extraction of `synth` 64 x 1800 scans, on a drive with revisits; one JSON
line per store size.

    python tools/visibility_bench.py [--keyframes 1000 10000] [--scans 64] [--resident 0] [--warm-ms 200] [--runs 5] [--out FILE]

  run            one lfx_visibility_run over the whole store (flags only), HIP events around the call: the median of `runs`
                 after warming by the clock (--warm-ms of back-to-back runs), and the list
  pairs_per_s, votes_per_s   the result's n_pairs, and the records of every target times its qualifying viewers, per second
  floor_share    the floor -- one read of the window's records (16 bytes each) plus one write of its flag bytes and vote words
                 (5 bytes) at lfx_box_calibration's copy rate on the same box -- over the run's time
  build, build_masked   the whole store of a kind to a device buffer, plain and through the run's flags: medians, and
                 bytes read plus written per second beside the copy rate
The run is one number: its launches (pairs, then per chunk of viewers images, occupied cells and one vote launch per kind) are
told apart with a kernel trace of this tool, not by the tool.  --resident 0 keeps every image on the device at once.
The poses lie on two laps of a circle sized so that neighbours are 2.5 m apart: every place is passed twice."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lidar_feature_extraction_amd import FeatureExtraction, Keyframes, concat, make_scan  # noqa: E402


def circle(n, spacing=2.5):
    ang = 4.0 * np.pi * np.arange(n) / n
    radius = spacing * n / (4.0 * np.pi)
    T = np.zeros((n, 3, 4))
    yaw = ang + np.pi / 2
    T[:, 0, 0], T[:, 0, 1], T[:, 1, 0], T[:, 1, 1], T[:, 2, 2] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw), 1.0
    T[:, 0, 3], T[:, 1, 3] = radius * np.cos(ang), radius * np.sin(ang)
    return T


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--resident", type=int, default=0)
    ap.add_argument("--warm-ms", type=float, default=200.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rings, cols, batch = 64, 1800, a.scans
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    fx = FeatureExtraction(device=0, max_points_per_scan=rings * cols, max_batch=batch, max_points_per_ring=cols, max_rings=rings)
    distinct = [make_scan(rings, cols, seed=7000 + k) for k in range(min(batch, 8))]
    clouds = [distinct[k % len(distinct)] for k in range(batch)]
    d_in = torch.from_numpy(np.ascontiguousarray(concat(clouds)).view(np.uint8).reshape(-1).copy()).to(dev)
    fx.extract_batch_device(d_in.data_ptr(), [len(c) for c in clouds], stream)
    got = [fx.download(s, stream) for s in range(batch)]
    per = np.array([[len(g.edge_points), len(g.surface_points)] for g in got], np.int64)

    def events(call):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        begin.record()
        call()
        end.record()
        torch.cuda.synchronize()
        return round(1e3 * begin.elapsed_time(end), 1)

    def measured(call):
        """warm by the clock, then `runs` timed calls: (median, all) in microseconds"""
        t0 = time.perf_counter()
        while 1e3 * (time.perf_counter() - t0) < a.warm_ms:
            call()
            torch.cuda.synchronize()
        us = [events(call) for _ in range(a.runs)]
        return float(np.median(us)), us

    lines = []
    for n in a.keyframes:
        counts = per[np.arange(n) % batch]
        total = counts.sum(axis=0)
        poses = circle(n)
        kf = fx.keyframes(n, (int(total[0]), int(total[1])))
        v = fx.device_view()
        cap = fx.max_points_per_scan * fx.max_batch
        info = int(v.scan_info)
        for first in range(0, n, batch):
            m = min(batch, n - first)
            e = Keyframes.clouds(v.edge_points, v.scan_begin, info + 8, 4, cap)
            s = Keyframes.clouds(v.surface_points, v.scan_begin, info + 12, 4, cap)
            kf.add(e, s, poses[first:first + m], stream)      # (a last, shorter add takes the first m clouds of the batch)
        assert kf.info()["n_points"] == (int(total[0]), int(total[1]))
        resident = a.resident or n
        vis = fx.visibility(n, resident)
        line = dict(keyframes=n, edge_records=int(total[0]), surface_records=int(total[1]), max_resident_images=resident,
                    visibility_device_bytes=vis.info()["device_bytes"])
        flags = tuple(torch.zeros(max(int(total[k]), 1), dtype=torch.uint8, device=dev) for k in range(2))
        _, _, res = vis.run(kf, 0, n, flags=flags, stream=stream)
        line["result"] = res
        med, us = measured(lambda: vis.run(kf, 0, n, flags=flags, stream=stream))
        line["run_us"], line["run_us_all"] = med, us
        # every target keyframe's records times its qualifying viewers: from the poses, as the rule counts pairs
        t = poses[:, :, 3]
        votes = 0
        for k0 in range(0, n, 1024):
            d = t[k0:k0 + 1024, None, :] - t[None, :, :]
            near = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] <= 15.0 * 15.0).sum(1) - 1
            votes += int((near * counts[k0:k0 + 1024].sum(1)).sum())
        line["record_votes"] = votes
        line["pairs_per_s"] = round(res["n_pairs"] / (1e-6 * med), 1)
        line["votes_per_s"] = round(votes / (1e-6 * med), 1)
        copy = [fx.box_calibration(0, stream)[0] for _ in range(3)]
        line["copy_gb_s"] = round(float(np.median(copy)), 1)
        floor_us = 21.0 * float(total.sum()) / (line["copy_gb_s"] * 1e3)
        line["floor_us"], line["floor_share"] = round(floor_us, 1), round(floor_us / med, 5)
        for kind, name in ((0, "edge"), (1, "surface")):
            records = int(total[kind])
            out = torch.empty((records, 4), dtype=torch.float32, device=dev)
            med_b, _ = measured(lambda: kf.build(kind, 0, n, d_out=out.data_ptr(), capacity_points=records, stream=stream))
            kept = kf.build_masked(kind, flags[kind], 0, n, d_out=out.data_ptr(), capacity_points=records, stream=stream)
            med_m, _ = measured(lambda: kf.build_masked(kind, flags[kind], 0, n, d_out=out.data_ptr(), capacity_points=records, stream=stream))
            line["build_%s_us" % name], line["build_masked_%s_us" % name], line["kept_%s" % name] = med_b, med_m, kept
            line["build_%s_gb_s" % name] = round(32.0 * records / (1e3 * med_b), 1)
            line["build_masked_%s_gb_s" % name] = round((17.0 * records + 16.0 * kept) / (1e3 * med_m), 1)
            del out
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
        vis.close()
        kf.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    fx.close()


if __name__ == "__main__":
    main()
