"""tools/segment_bench.py -- time of lfx_segment_batch and lfx_pack_features_segmented (include/lfx.h, the segmentation
section) beside this box's copy rate.

  python3 tools/segment_bench.py [--shapes 64x1800,16x1800] [--batch 1024] [--distinct 16] [--window 0.5] [--repeats 5]
                                 [--calls N] [--out FILE]

Per shape H x W: the batch is `distinct` scans (synth.make_scan from different places) repeated to `batch` scans on the
device, extracted once; the image is H x W, ground rows 0 .. H/2 - 1.  Warm-up by the clock (0.25 s), then `repeats` windows
of at least `window` seconds of back-to-back calls between two device events; the values are the median window's time per
call and the least and the largest window's (the spread).  A call is everything lfx_segment_batch queues: per chunk of scans
the image's memset and the seven kernels.
segment_record_gbs: the records' bytes (32 B each) read ONCE over the call's time -- the call reads them twice (projection,
per-record pass) and the images several times, so this is the rate a caller sees, not a kernel's; segment_share_of_copy is
that rate over box_copy_gbs / 2 (a copy's rate counts bytes read plus bytes written; a pure read would reach about half).
Per kernel: run the tool under `rocprofv3 --kernel-trace --stats` with --calls N (N timed calls per shape, no windows: tracing
slows the host) and read the segment_* rows of its kernel statistics; the times here are taken with the profiler off.
The first scans' classes are compared with the numpy restatement (tests/segment_restatement.py, which needs scipy): the timed
call computes what the tests pin.  Run from an installed package, without the repository's tests/ beside it, the comparison
is left out and *_equals_restatement is null."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def windows(call, sync, ev0, ev1, window, repeats, fixed_calls=0):
    t = time.perf_counter()
    n_warm = 0
    while time.perf_counter() - t < 0.25 or n_warm < 2:
        call()
        n_warm += 1
    sync()
    per_call = max((time.perf_counter() - t) / n_warm, 1e-6)
    calls = fixed_calls if fixed_calls else max(int(window / per_call) + 1, 4)
    spans = []
    for _ in range(1 if fixed_calls else repeats):
        ev0.record()
        for _ in range(calls):
            call()
        ev1.record()
        ev1.synchronize()
        spans.append(ev0.elapsed_time(ev1) / calls)
    return float(np.median(spans)), float(min(spans)), float(max(spans)), calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x1800,16x1800")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from lidar_feature_extraction_amd import FeatureExtraction, binding as B, concat, make_scan, segment_config
    try:
        from tests import segment_restatement as R
    except ImportError:                  # (no tests/ beside the package, or no scipy)
        R = None
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = dict(metric="segment", batch=a.batch)
    for shape in [s for s in a.shapes.split(",") if s]:
        rings, cols = (int(v) for v in shape.split("x"))
        per = rings * cols
        scans = [make_scan(rings, cols, seed=7000 + i, sensor_pose=(0.9 * i - 7.0, 0.3 * i - 2.0, 0.4 * i)) for i in range(a.distinct)]
        one = torch.from_numpy(concat(scans).view(np.uint8).copy()).to(dev)
        d_all = one.repeat((a.batch + a.distinct - 1) // a.distinct)[:a.batch * per * 32].contiguous()
        fx = FeatureExtraction(device=0, max_points_per_scan=per, max_batch=a.batch, max_points_per_ring=cols, max_rings=rings)
        fx.extract_batch_device(d_all.data_ptr(), [per] * a.batch, stream)
        torch.cuda.synchronize()
        if "box_copy_gbs" not in out:
            gbs, mhz = fx.box_calibration(0, stream)
            out["box_copy_gbs"], out["box_clock_mhz"] = round(gbs, 1), round(mhz, 1)
        L, ctx = fx._L, fx._ctx
        cfg = segment_config(n_rows=rings, n_columns=cols, ground_last_row=rings // 2 - 1)
        classes = torch.zeros(a.batch * per, dtype=torch.uint8, device=dev)
        ids = torch.zeros(a.batch * per, dtype=torch.int32, device=dev)
        counts = torch.zeros((a.batch, 4), dtype=torch.int32, device=dev)

        def segment():
            B.check(ctx, L.lfx_segment_batch(ctx, C.byref(cfg), a.batch, classes.data_ptr(), ids.data_ptr(), counts.data_ptr(), stream), L)
        ms, lo, hi, calls = windows(segment, torch.cuda.synchronize, ev0, ev1, a.window, a.repeats, a.calls)
        key = "segment_%s" % shape
        out[key + "_us"] = round(ms * 1e3, 1)
        out[key + "_us_spread"] = [round(lo * 1e3, 1), round(hi * 1e3, 1)]
        out[key + "_calls_per_window"] = calls
        out[key + "_input_records"] = a.batch * per
        rate = a.batch * per * 32 / (ms * 1e-3) / 1e9
        out[key + "_record_gbs"] = round(rate, 1)
        out[key + "_share_of_copy"] = round(rate / (out["box_copy_gbs"] / 2.0), 3) if out["box_copy_gbs"] else None
        n = min(a.distinct, a.batch, 2)
        got = classes[:n * per].cpu().numpy()
        out[key + "_equals_restatement"] = bool(got.tobytes() == R.segment_batch(cfg, scans[:n])[0].tobytes()) if R else None
        out[key + "_counts_scan0"] = counts[0].cpu().numpy().view(np.uint32).tolist()
        cap = a.batch * per // 4
        edge = torch.zeros((cap, 4), dtype=torch.float32, device=dev)
        surface = torch.zeros((cap, 4), dtype=torch.float32, device=dev)
        offsets = torch.zeros((2, a.batch + 1), dtype=torch.int32, device=dev)
        kept = torch.zeros((2, a.batch), dtype=torch.int32, device=dev)

        def pack():
            B.check(ctx, L.lfx_pack_features_segmented(ctx, classes.data_ptr(), B.SEG_EDGE_MASK_DEFAULT, B.SEG_SURFACE_MASK_DEFAULT, edge.data_ptr(),
                                                       surface.data_ptr(), offsets.data_ptr(), kept.data_ptr(), cap, stream), L)
        ms, lo, hi, calls = windows(pack, torch.cuda.synchronize, ev0, ev1, a.window, a.repeats, a.calls)
        out["pack_%s_us" % shape] = round(ms * 1e3, 1)
        out["pack_%s_us_spread" % shape] = [round(lo * 1e3, 1), round(hi * 1e3, 1)]
        off = offsets.cpu().numpy().view(np.uint32)
        out["pack_%s_kept" % shape] = [int(off[0][a.batch]), int(off[1][a.batch])]
        fx.close()
        del d_all, classes, ids, counts, edge, surface
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
