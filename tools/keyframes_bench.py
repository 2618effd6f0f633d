"""Times of the keyframe store (lfx_keyframes): a store of N keyframes whose per-keyframe counts come from a real extraction of
`synth` 64 x 1800 scans, built, cut and moved; one JSON line.

    python tools/keyframes_bench.py [--keyframes 10000] [--scans 64] [--runs 3] [--out FILE] [--masked]

  --masked     instead of the figures below: submap_masked over the store's own flags beside submap and build_masked (masked())

  build        the whole store of a kind to a device buffer: HIP events around the call, and bytes read plus written (32 per
               record) per second beside lfx_box_calibration's copy rate on the same box
  mapper       the same rebuild through the route that was there before: a fresh Mapper (thresholds 0, capacity pre-sized),
               the poses downloaded from the graph, one add of N clouds; wall clock from the download to the stream's end
  submap       of about 25 and about 200 keyframes: flag, plan, the wait and the transform; wall clock to the stream's end
  follow       N poses from a pose graph's device array: HIP events
  add          one batch of `scans` scans, both clouds, from the context's buffers: wall clock to the stream's end

The poses lie on two laps of a circle sized so that neighbours are 2.5 m apart.  Every figure is the list of the runs."""
import argparse
import ctypes as C
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


def masked(a, fx, kf, counts, poses, line, wall):
    """--masked: the store's own flags at shares 0, 0.05 and 0.5 (drawn per record), and per kind
      w25          a window of 25 ids, all selected: submap_masked beside submap and build_masked of the same keyframes
      w1000_all    a window of 1 000 ids, all selected
      w1000_five   the same window with a radius that selects five keyframes in its middle: the runs of 1 024 records without
                   a selected keyframe are skipped, so the time should follow the five, not the thousand
    Medians of --runs, wall clock to the stream's end (each call waits once for its result).  `stages` counts what the
    masked call queues: launches, and the runs of the window, those counted and those the scatter is launched over."""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    n = len(poses)
    kf.reserve_flags(stream)
    line["flags_device_bytes"] = kf.flags_info(stream)["device_bytes"]
    mid = n // 4                                                             # (far from the lap's seam and from the second lap)
    windows = {"w25": (mid - 12, 25, 1e9), "w1000_all": (mid - 500, 1000, 1e9), "w1000_five": (mid - 500, 1000, 5.1)}
    rng = np.random.default_rng(5)

    def median(call):
        call()
        return float(np.median([wall(call)[0] for _ in range(a.runs)]))

    for kind, name in ((0, "edge"), (1, "surface")):
        begin = np.concatenate([[0], np.cumsum(counts[:, kind])])
        out = torch.empty((int(begin[-1]), 4), dtype=torch.float32, device=dev)
        for share in (0.0, 0.05, 0.5):
            drawn = torch.from_numpy((rng.random(int(begin[-1])) < share).astype(np.uint8)).to(dev)
            kf.set_flags(kind, drawn, 0, n, stream)
            d_flags = kf.flags(stream)[kind]
            for wname, (first, count, radius) in windows.items():
                first, count = max(first, 0), min(count, n - max(first, 0))
                center = poses[min(mid, n - 1), :, 3]
                args = (kind, center, radius, first, count)
                room = int(begin[first + count] - begin[first])
                key = "%s_%s_share_%g" % (wname, name, share)
                res = kf.submap_masked(*args, d_out=out.data_ptr(), capacity_points=room, stream=stream)[1]
                line[key] = dict(
                    submap_masked_us=median(lambda: kf.submap_masked(*args, d_out=out.data_ptr(), capacity_points=room, stream=stream)),
                    submap_us=median(lambda: kf.submap(*args, d_out=out.data_ptr(), capacity_points=room, stream=stream)),
                    n_selected=res["n_selected"], n_points=res["n_points"], window_records=room)
                if wname == "w25":
                    line[key]["build_masked_us"] = median(lambda: kf.build_masked(kind, d_flags, first, count, d_out=out.data_ptr(),
                                                                                  capacity_points=room, stream=stream))
                    line[key]["build_us"] = median(lambda: kf.build(kind, first, count, d_out=out.data_ptr(), capacity_points=room, stream=stream))
                if share == 0.0:
                    # the stages: flag, count, scan, kept, plan (5 launches), the record's copy and wait, the scatter
                    sel = np.linalg.norm(poses[first:first + count, :, 3] - center, axis=1) <= radius
                    run_of = lambda i: (i - begin[first]) // 1024
                    ids = first + np.nonzero(sel & (counts[first:first + count, kind] > 0))[0]
                    counted = set()
                    for k in ids:
                        counted.update(range(int(run_of(begin[k])), int(run_of(begin[k + 1] - 1)) + 1))
                    line[key]["stages"] = dict(launches=6 if res["n_points"] else 5, submap_launches=3 if res["n_points"] else 2,
                                               window_runs=int(-(-room // 1024)), counted_runs=len(counted),
                                               scatter_runs=int(run_of(begin[ids[-1] + 1] - 1) - run_of(begin[ids[0]]) + 1) if len(ids) else 0)
        del out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=10000)
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--masked", action="store_true", help="time submap_masked beside submap and build_masked, and nothing else")
    a = ap.parse_args()
    rings, cols, n, batch = 64, 1800, a.keyframes, a.scans
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    fx = FeatureExtraction(device=0, max_points_per_scan=rings * cols, max_batch=batch, max_points_per_ring=cols, max_rings=rings)
    distinct = [make_scan(rings, cols, seed=7000 + k) for k in range(min(batch, 8))]
    clouds = [distinct[k % len(distinct)] for k in range(batch)]
    d_in = torch.from_numpy(np.ascontiguousarray(concat(clouds)).view(np.uint8).reshape(-1).copy()).to(dev)
    fx.extract_batch_device(d_in.data_ptr(), [len(c) for c in clouds], stream)
    got = [fx.download(s, stream) for s in range(batch)]
    per = np.array([[len(g.edge_points), len(g.surface_points)] for g in got], np.int64)
    counts = per[np.arange(n) % batch]
    total = counts.sum(axis=0)
    poses = circle(n)
    line = dict(keyframes=n, scans_per_batch=batch, edge_per_scan=[int(per[:, 0].min()), int(per[:, 0].max())],
                surface_per_scan=[int(per[:, 1].min()), int(per[:, 1].max())], edge_records=int(total[0]), surface_records=int(total[1]))

    def wall(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        return round(1e6 * (time.perf_counter() - t0), 1), out

    def events(call):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        begin.record()
        call()
        end.record()
        torch.cuda.synchronize()
        return round(1e3 * begin.elapsed_time(end), 1)

    kf = fx.keyframes(n, (int(total[0]), int(total[1])))
    line["device_bytes"] = kf.info()["device_bytes"]
    line["add_batch_us"] = []
    for first in range(0, n, batch):
        m = min(batch, n - first)
        v = fx.device_view()
        cap = fx.max_points_per_scan * fx.max_batch
        info = int(v.scan_info)
        us, _ = wall(lambda: kf.add(Keyframes.clouds(v.edge_points, v.scan_begin, info + 8, 4, cap),
                                    Keyframes.clouds(v.surface_points, v.scan_begin, info + 12, 4, cap), poses[first:first + m], stream))
        if m == batch and 0 < first <= a.runs * batch:
            line["add_batch_us"].append(us)
    assert kf.info()["n_points"] == (int(total[0]), int(total[1]))
    pg = fx.pose_graph(n, 1)
    pg.add_nodes(poses, stream)
    kf.follow(pg, stream=stream)
    line["follow_us"] = [events(lambda: kf.follow(pg, stream=stream)) for _ in range(a.runs)]
    line["copy_gb_s"] = [round(fx.box_calibration(0, stream)[0], 1) for _ in range(a.runs)]
    if a.masked:
        masked(a, fx, kf, counts, poses, line, wall)
    view = kf.view(stream)
    for kind, name in (() if a.masked else ((0, "edge"), (1, "surface"))):
        records = int(total[kind])
        out = torch.empty((records, 4), dtype=torch.float32, device=dev)
        kf.build(kind, 0, n, d_out=out.data_ptr(), capacity_points=records, stream=stream)
        us = [events(lambda: kf.build(kind, 0, n, d_out=out.data_ptr(), capacity_points=records, stream=stream)) for _ in range(a.runs)]
        line["build_%s_us" % name] = us
        line["build_%s_gb_s" % name] = [round(32.0 * records / (1e3 * u), 1) for u in us]
        # the route that was there before: poses down, a fresh mapper, one add of n clouds
        begin = np.concatenate([[0], np.cumsum(counts[:, kind])])[:-1].astype(np.uint32)
        d_begin = torch.from_numpy(begin.view(np.int32).copy()).to(dev)
        d_count = torch.from_numpy(counts[:, kind].astype(np.uint32).view(np.int32).copy()).to(dev)
        line["mapper_%s_us" % name] = []
        same = None
        for _ in range(a.runs + 1):
            mp = fx.mapper(translation_threshold=0.0, rotation_threshold=0.0, initial_capacity_points=records, max_points=max(records, 1))
            us, _ = wall(lambda: mp.add(view["points"][kind], d_begin.data_ptr(), d_count.data_ptr(), 1, n, records, pg.poses(stream=stream), stream))
            line["mapper_%s_us" % name].append(us)
            if same is None:
                got_map = torch.empty((records, 4), dtype=torch.float32, device=dev)
                hip = fx._L
                hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
                assert hip.hipMemcpy(got_map.data_ptr(), mp.view()["points"], 16 * records, 3) == 0
                same = bool(torch.equal(got_map.view(torch.int32), out.view(torch.int32)))
                del got_map
            mp.close()
        line["mapper_%s_us" % name] = line["mapper_%s_us" % name][1:]          # (the first run warms the kernel and the pinned block)
        line["mapper_%s_same_bytes" % name] = same
        # submaps around keyframe 0 of about 25 and about 200 keyframes
        d = np.sort(np.linalg.norm(poses[:, :, 3] - poses[0, :, 3], axis=1))
        for want in (25, 200):
            radius = float(0.5 * (d[want - 1] + d[want]))
            kf.submap(kind, poses[0, :, 3], radius, 0, n, d_out=out.data_ptr(), capacity_points=records, stream=stream)
            runs = [wall(lambda: kf.submap(kind, poses[0, :, 3], radius, 0, n, d_out=out.data_ptr(), capacity_points=records, stream=stream))
                    for _ in range(a.runs)]
            line["submap_%d_%s_us" % (want, name)] = [us for us, _ in runs]
            line["submap_%d_%s" % (want, name)] = [runs[-1][1][1]["n_selected"], runs[-1][1][1]["n_points"]]
        del out
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    pg.close()
    kf.close()
    fx.close()


if __name__ == "__main__":
    main()
