"""tools/place_bench.py -- time of lfx_scan_context_batch and lfx_place_db_query (include/lfx.h, the place recognition section)
beside this box's copy rate, the de-skew kernel's time from the same run and the numpy restatement on one core.

  python3 tools/place_bench.py [--rings 64] [--cols 1800] [--batch 1024] [--distinct 16] [--window 0.5] [--repeats 5]
                               [--entries 256,4096,65536] [--queries 1,64] [--numpy-entries 256] [--out FILE]

The descriptor: the batch is `distinct` scans (synth.make_scan from different places) repeated to `batch` scans on the
device; warm-up by the clock (0.25 s), then `repeats` windows of at least `window` seconds of back-to-back calls between two
device events (each call: the table's copy, the keys' memset, both kernels); the value is the median window's time per call.
scan_context_line_gbs counts the record lines the call reads, 32 B per record (12 of them useful), nothing else.
deskew_index_us: lfx_deskew_batch out of place with index times (deskew_kernel<0>) on the same batch, timed the same way: it
walks the feature records (about an eighth of the input records), not the input.
The index: `entries` random descriptors (a tenth of the cells and a few columns empty) and `queries` of the same kind,
k = 4; lfx_place_db_query is synchronous, so the value is the host's clock around the call, the median of `repeats` calls
after two untimed ones.  query_*_pairs_per_s counts (query, entry) pairs.  numpy_us_per_pair: the restatement
(tests/scan_context_restatement.py shift_distances, one core) for one query against `numpy-entries` entries."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def windows(call, sync, ev0, ev1, window, repeats):
    t = time.perf_counter()
    n_warm = 0
    while time.perf_counter() - t < 0.25:
        call()
        n_warm += 1
    sync()
    per_call = max((time.perf_counter() - t) / n_warm, 1e-6)
    calls = max(int(window / per_call) + 1, 4)
    spans = []
    for _ in range(repeats):
        ev0.record()
        for _ in range(calls):
            call()
        ev1.record()
        ev1.synchronize()
        spans.append(ev0.elapsed_time(ev1) / calls)
    return float(np.median(spans)), calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--cols", type=int, default=1800)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--entries", default="256,4096,65536")
    ap.add_argument("--queries", default="1,64")
    ap.add_argument("--numpy-entries", type=int, default=256)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from lidar_feature_extraction_amd import FeatureExtraction, binding as B, concat, make_scan, scan_context_config
    from lidar_feature_extraction_amd.extraction import _sweeps
    from tests import scan_context_restatement as R
    per = a.rings * a.cols
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    scans = [make_scan(a.rings, a.cols, seed=7000 + i, sensor_pose=(0.9 * i - 7.0, 0.3 * i - 2.0, 0.4 * i)) for i in range(a.distinct)]
    one = torch.from_numpy(concat(scans).view(np.uint8).copy()).to(dev)
    d_all = one.repeat((a.batch + a.distinct - 1) // a.distinct)[:a.batch * per * 32].contiguous()
    fx = FeatureExtraction(device=0, max_points_per_scan=per, max_batch=a.batch, max_points_per_ring=a.cols, max_rings=a.rings)
    fx.extract_batch_device(d_all.data_ptr(), [per] * a.batch, stream)
    torch.cuda.synchronize()
    gbs, mhz = fx.box_calibration(0, stream)
    out = dict(metric="place", rings=a.rings, cols=a.cols, batch=a.batch, input_records=a.batch * per, box_copy_gbs=round(gbs, 1),
               box_clock_mhz=round(mhz, 1))
    L, ctx = fx._L, fx._ctx
    cfg = scan_context_config()
    R_, S_ = int(cfg.n_rings), int(cfg.n_sectors)
    desc = torch.zeros((a.batch, R_, S_), dtype=torch.float32, device=dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def scan_context():
        B.check(ctx, L.lfx_scan_context_batch(ctx, C.byref(cfg), a.batch, desc.data_ptr(), stream), L)
    ms, calls = windows(scan_context, torch.cuda.synchronize, ev0, ev1, a.window, a.repeats)
    out["scan_context_us"] = round(ms * 1e3, 1)
    out["scan_context_line_gbs"] = round(a.batch * per * 32 / (ms * 1e-3) / 1e9, 1)
    out["scan_context_calls_per_window"] = calls
    # the first scans' descriptors against the restatement: the timed call computes what the tests pin
    got = desc[:min(a.distinct, a.batch)].cpu().numpy()
    out["scan_context_equals_restatement"] = bool(all(got[i].tobytes() == R.descriptor_of_cloud(cfg, scans[i]).tobytes() for i in range(len(got))))
    # deskew_kernel<0> on the same batch, out of place
    identity = np.eye(4)[:3]
    sw, _ = _sweeps([(0.0, 0.1, identity)] * a.batch)
    index = B.TimeField(B.TIME_FROM_INDEX, 0, 0, 0, 1.0)
    other = (torch.zeros((a.batch * per + 1, 4), dtype=torch.float32, device=dev), torch.zeros((a.batch * per + 1, 4), dtype=torch.float32, device=dev))

    def deskew():
        B.check(ctx, L.lfx_deskew_batch(ctx, C.byref(index), sw, a.batch, B.DESKEW_TO_END, other[0].data_ptr(), other[1].data_ptr(), stream), L)
    ms, calls = windows(deskew, torch.cuda.synchronize, ev0, ev1, a.window, a.repeats)
    out["deskew_index_us"] = round(ms * 1e3, 1)
    del other, d_all
    # the index
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)

    def descriptors(n):
        d = torch.rand((n, R_, S_), generator=gen, device=dev, dtype=torch.float32) * 5.0
        d[torch.rand((n, R_, S_), generator=gen, device=dev) < 0.1] = 0.0
        d[:, :, 7:11] = 0.0
        return d.contiguous()
    sizes = [int(v) for v in a.entries.split(",") if v]
    n_queries = [int(v) for v in a.queries.split(",") if v]
    queries = descriptors(max(n_queries))
    for n in sizes:
        db = fx.place_db(n)
        entries = descriptors(n)
        db.add(entries, n, stream)
        torch.cuda.synchronize()
        for nq in n_queries:
            spans = []
            for i in range(2 + a.repeats):
                t = time.perf_counter()
                db.query_raw(queries, nq, 4, 0, n, stream)
                if i >= 2:
                    spans.append(time.perf_counter() - t)
            sec = float(np.median(spans))
            out["query_%dx%d_us" % (nq, n)] = round(sec * 1e6, 1)
            out["query_%dx%d_pairs_per_s" % (nq, n)] = round(nq * n / sec, 1)
        if n == sizes[0]:
            m = min(a.numpy_entries, n)
            host_q, host_e = queries[0].cpu().numpy(), entries[:m].cpu().numpy()
            t = time.perf_counter()
            want = R.query(host_q, host_e, 4)
            out["numpy_us_per_pair"] = round((time.perf_counter() - t) * 1e6 / m, 1)
            raw = db.query_raw(queries, 1, 4, 0, m, stream)
            out["query_equals_restatement"] = [(int(r.entry), int(r.shift), float(r.distance), float(r.yaw)) for r in raw[:4]] == \
                [(e, s, d, y) for e, s, d, y in want]
        db.close()
        del entries
    fx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
