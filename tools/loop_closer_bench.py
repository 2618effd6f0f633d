"""tools/loop_closer_bench.py -- time of lfx_place_db_query_gated beside lfx_place_db_query, and of the loop closer's verify and
update with the shares of their steps (include/lfx.h, the place recognition and the loop closer sections).

  python3 tools/loop_closer_bench.py [--entries 65536] [--queries 1,64] [--eligible 64] [--repeats 9]
                                     [--rings 64] [--cols 1800] [--places 8] [--out FILE]

The query: `entries` random descriptors (as tools/place_bench.py makes them), k = 4.  Poses put `eligible` entries within the
radius of the queries' pose and every other entry far away ("gated_few"), or every entry within it ("gated_all"); "gated_limit"
is the gated call without poses (limit = entries: nothing but the limit gates).  "ungated" is lfx_place_db_query over the
same range.  All calls are synchronous, so a value is the host's clock around the call; the four take turns, one call each
per round, `repeats` rounds after two untimed ones, and the value is the median.
The closer: `places` places along a line, 3 m apart, each visited twice (2 x places keyframes of rings x cols from
synth.make_scan; min_gap = places), the second visit 0.2 m off and turned; poses are the true ones.  verify_us: the median over
the second visits of one lfx_loop_closer_verify; the shares are the same steps composed by hand from the public calls with the
device drained after each (submap: both kinds; map: both lfx_map_create; downsample; align: lfx_scan_to_map_align_report).
update_us_per_keyframe: one lfx_loop_closer_update over all second visits (detect, the verifications, the edges, the
optimiser, follow) on a fresh graph, divided by their number."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def planar(yaw, x, y):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0.0, x], [s, c, 0.0, y], [0.0, 0.0, 1.0, 0.0]], np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=65536)
    ap.add_argument("--queries", default="1,64")
    ap.add_argument("--eligible", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--cols", type=int, default=1800)
    ap.add_argument("--places", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from lidar_feature_extraction_amd import FeatureExtraction, concat, make_scan, motion_between, pose_graph_edges, scan_context_config
    from tests import loop_closer_restatement as LR
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    per = a.rings * a.cols
    n_key = 2 * a.places
    fx = FeatureExtraction(device=0, max_points_per_scan=per, max_batch=n_key, max_points_per_ring=a.cols, max_rings=a.rings)
    gbs, mhz = fx.box_calibration(0, stream)
    out = dict(metric="loop_closer", box_copy_gbs=round(gbs, 1), box_clock_mhz=round(mhz, 1), entries=a.entries, eligible=a.eligible)
    cfg = scan_context_config()
    R_, S_ = int(cfg.n_rings), int(cfg.n_sectors)

    # --- 1. the gated query beside the ungated one ---------------------------------------------------------------------------
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)

    def descriptors(n):
        d = torch.rand((n, R_, S_), generator=gen, device=dev, dtype=torch.float32) * 5.0
        d[torch.rand((n, R_, S_), generator=gen, device=dev) < 0.1] = 0.0
        d[:, :, 7:11] = 0.0
        return d.contiguous()
    n = a.entries
    n_queries = [int(v) for v in a.queries.split(",") if v]
    db = fx.place_db(n)
    entries, queries = descriptors(n), descriptors(max(n_queries))
    db.add(entries, n, stream)
    few = np.zeros((n + 1, 3, 4))
    few[:, 0, 0] = few[:, 1, 1] = few[:, 2, 2] = 1.0
    few[:n, 0, 3] = 1000.0
    few[np.linspace(0, n - 1, a.eligible).astype(np.int64), 0, 3] = 1.0     # the eligible entries: spread over the index
    near = few.copy()
    near[:n, 0, 3] = 1.0
    d_few, d_near = torch.from_numpy(few).to(dev), torch.from_numpy(near).to(dev)
    torch.cuda.synchronize()
    for nq in n_queries:
        gates = [(n, n)] * nq
        calls = dict(ungated=lambda: db.query_raw(queries, nq, 4, 0, n, stream),
                     gated_few=lambda: db.query_gated_raw(queries, gates, d_few, 15.0, 4, stream),
                     gated_all=lambda: db.query_gated_raw(queries, gates, d_near, 15.0, 4, stream),
                     gated_limit=lambda: db.query_gated_raw(queries, gates, 0, float("inf"), 4, stream))
        spans = {name: [] for name in calls}
        for i in range(2 + a.repeats):
            for name, call in calls.items():
                t = time.perf_counter()
                call()
                if i >= 2:
                    spans[name].append(time.perf_counter() - t)
        for name in calls:
            out["%s_%dx%d_us" % (name, nq, n)] = round(float(np.median(spans[name])) * 1e6, 1)
        plain = bytes(calls["ungated"]())
        out["gated_equals_ungated_%d" % nq] = bool(bytes(calls["gated_all"]()[0]) == plain and bytes(calls["gated_limit"]()[0]) == plain)
        out["gated_few_eligible_%d" % nq] = int(calls["gated_few"]()[1][0])
    db.close()
    del entries, queries, d_few, d_near

    # --- 2. the closer -------------------------------------------------------------------------------------------------------
    places = [(3.0 * i - 1.5 * a.places, 0.5 * (i % 3)) for i in range(a.places)]
    truth = [planar(0.0, x, y) for x, y in places] + [planar(0.6 * (i + 1), x + 0.2, y - 0.15) for i, (x, y) in enumerate(places)]
    scans = [make_scan(a.rings, a.cols, seed=8000 + k, sensor_pose=(p[0, 3], p[1, 3], float(np.arctan2(p[1, 0], p[0, 0])))) for k, p in enumerate(truth)]
    poses = np.stack(truth)
    d_scans = torch.from_numpy(concat(scans).view(np.uint8).copy()).to(dev)
    fx.extract_batch_device(d_scans.data_ptr(), [per] * n_key, stream)
    fx.batch_status(stream)
    db = fx.place_db(n_key)
    db.add(fx.scan_context(cfg, None, stream), n_key, stream)
    kf = fx.keyframes(n_key, n_key * per)
    kf.add_batch(poses, stream)
    info = np.diag([1.0 / 0.005 ** 2] * 3 + [1.0 / 0.1 ** 2] * 3)
    chain = pose_graph_edges(range(n_key - 1), range(1, n_key), [motion_between(poses[k], poses[k + 1]) for k in range(n_key - 1)],
                             [info] * (n_key - 1))

    def new_graph():
        g = fx.pose_graph(n_key, 4 * n_key)
        g.add_nodes(poses, stream)
        g.add_edges(chain, stream)
        return g
    settings = dict(min_gap=a.places, search_radius=2.0, max_distance=1.0, submap_half_window=2, submap_radius=5.0, submap_capacity=5 * per)
    graph = new_graph()
    lc = fx.loop_closer(kf, db, graph, **settings)
    cands, _ = lc.detect(a.places, a.places, stream)
    out["closer_keyframes"] = n_key
    out["closer_detected"] = sum(1 for row in cands if row[0]["entry"] is not None)
    out["closer_true_place"] = sum(1 for q, row in enumerate(cands) if row[0]["entry"] == q)
    steps = dict(submap=[], map=[], downsample=[], align=[])
    verify, accepted = [], 0

    def timed(name, call):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = call()
        torch.cuda.synchronize()
        steps[name].append(time.perf_counter() - t)
        return r
    for rep in range(2 + min(a.repeats, 3)):
        for s, row in enumerate(cands):
            q, cand = a.places + s, row[0]
            if cand["entry"] is None:
                continue
            t = time.perf_counter()
            closure = lc.verify_raw(q, cand, stream)
            if rep >= 2:
                verify.append(time.perf_counter() - t)
                accepted += int(closure.accepted) if rep == 2 else 0
            # the same steps by hand
            keep = {k: len(v) for k, v in steps.items()}
            c = cand["entry"]
            pose_c = kf.poses(c, 1, stream)[0]
            lo, count = LR.window(c, q, a.places, 2)
            subs = timed("submap", lambda: [kf.submap(kind, pose_c[:, 3], 5.0, lo, count, capacity_points=5 * per, stream=stream) for kind in (0, 1)])
            maps = timed("map", lambda: [fx.make_map(cloud.data_ptr(), res["n_points"], 1.0, stream) for cloud, res in subs])
            v = kf.view(stream)
            begin = [kf._range_points(kind, 0, q) for kind in (0, 1)]
            cnt = [kf._range_points(kind, q, 1) for kind in (0, 1)]
            words = torch.tensor([0, cnt[0], cnt[1], 0, 0, 0, 0, 0], dtype=torch.int32, device=dev)
            w = words.data_ptr()
            edge, surface = v["points"][0] + 16 * begin[0], v["points"][1] + 16 * begin[1]
            down = torch.zeros((cnt[1] + 1, 4), dtype=torch.float32, device=dev)
            timed("downsample", lambda: fx.voxel_downsample(surface, w, w + 8, 1, 1, cnt[1], 1.0, down.data_ptr(), w + 12, w + 16, stream))
            n_down, status = int(words[3]), int(words[4])
            scan, at, n_scan = (down.data_ptr(), w + 12, n_down) if status == 0 else (surface, w + 8, cnt[1])
            timed("align", lambda: fx.scan_to_map_align(maps[0], maps[1], 15, 20, edge, w, w + 4, 1, cnt[0], cnt[0], scan, w, at, 1, n_scan, n_scan,
                                                        [LR.initial_pose(pose_c, cand["yaw"])], stream, report=True))
            for m in maps:
                m.close()
            if rep < 2:
                for k in steps:
                    del steps[k][keep[k]:]
    out["verify_us"] = round(float(np.median(verify)) * 1e6, 1) if verify else None
    out["verify_accepted"] = accepted
    total = sum(float(np.median(v)) for v in steps.values() if v)
    for k, v in steps.items():
        out["step_%s_us" % k] = round(float(np.median(v)) * 1e6, 1) if v else None
        out["share_%s" % k] = round(float(np.median(v)) / total, 3) if v else None
    spans = []
    for rep in range(1 + min(a.repeats, 3)):
        g = new_graph()
        kf.set_poses(poses, 0, stream)
        closer = fx.loop_closer(kf, db, g, **settings)
        torch.cuda.synchronize()
        t = time.perf_counter()
        _closures, result = closer.update(a.places, a.places, stream)
        if rep >= 1:
            spans.append(time.perf_counter() - t)
        out["update_accepted"] = result["n_accepted"]
        closer.close()
        g.close()
    out["update_us_per_keyframe"] = round(float(np.median(spans)) * 1e6 / a.places, 1)
    lc.close()
    graph.close()
    kf.close()
    db.close()
    fx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
