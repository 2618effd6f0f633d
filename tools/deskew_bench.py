"""tools/deskew_bench.py -- time of lfx_deskew_batch and lfx_deskew_batch_trajectory (include/lfx.h, the de-skew section) on a
launch-scale batch, beside this box's copy rate and the compaction kernel's time from the same run, and the odometry's time
per scan without de-skew, with its own prediction and along the sweeps' true trajectories.

  python3 tools/deskew_bench.py [--rings 64] [--cols 1800] [--batch 1024] [--distinct 16] [--window 0.5] [--repeats 5]
                                [--odometry-scans 24] [--trajectory-knots 2,21,64] [--kernels-only] [--out FILE]

The batch is `distinct` sweeps (synth.make_sweep, moving sensor) repeated to `batch` scans on the device.  Out of place
(the index, and the FLOAT32 field at byte 24, as the time source): warm-up by the clock (0.25 s), then `repeats` windows of at
least `window` seconds of back-to-back calls between two device events, the profiler off; the value is the median window's
time per call.  In place (the same two sources): a batch may be de-skewed in place once, so every sample is one call behind
a fresh extraction of the batch, two device events around that call alone (they span the table's copy and the kernel; the
extraction before them is not in it); the value is the median of `--in-place-samples` samples after 5 untimed ones.  GB/s
counts algorithmic bytes: 36 B per feature record (16 read, 4 index, 16 written), + 4 for the FLOAT32 field.
feature_compact_ms: the compaction kernel's time for the same batch (lfx_set_profiling around one extraction), which moves
similar bytes.  The odometry: ms per scan, scan by scan, with and without de-skew, and both runs' largest translation error
against the sweeps' true end poses.
Trajectory mode (--trajectory-knots, "" to leave it out; index times): per knot count the whole call out of place and in
place, timed as above -- back to back, the host's work on one call's segment tables runs while the device is busy with the
call before, so the figure is the larger of the two sides --, beside two parts of a call timed alone: trajectory_K_call_host_us
(the host clock from the call to its return on an idle stream: the checks, lfx_trajectory_segments for every scan, queueing)
and trajectory_K_copy_us (a pinned-to-device copy of the table's bytes between two events).  The kernel alone is not timed
here but by the profiler, in a run of its own per knot count:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/deskew_bench.py --kernels-only --trajectory-knots K
queues 10 untimed and 50 out-of-place calls of lfx_deskew_batch and of lfx_deskew_batch_trajectory with K knots and nothing
else after the extraction; the statistics' rows of deskew_kernel and deskew_trajectory_kernel are the figures.
The odometry's third run hands every sweep's true trajectory to lfx_odometry_update_batch_trajectory."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--cols", type=int, default=1800)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--in-place-samples", type=int, default=30)
    ap.add_argument("--odometry-scans", type=int, default=24)
    ap.add_argument("--trajectory-knots", default="2,21,64")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from lidar_feature_extraction_amd import FeatureExtraction, binding as B, concat, make_sweep
    from tests import deskew_restatement as R
    per = a.rings * a.cols
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    D = R.pose([0.01, -0.02, 0.06], [1.5, 0.1, -0.05])
    sweeps = [make_sweep(a.rings, a.cols, seed=9500 + i, motion=D)[0] for i in range(a.distinct)]
    one = torch.from_numpy(concat(sweeps).view(np.uint8).copy()).to(dev)
    d_all = one.repeat((a.batch + a.distinct - 1) // a.distinct)[:a.batch * per * 32].contiguous()
    fx = FeatureExtraction(device=0, max_points_per_scan=per, max_batch=a.batch, max_points_per_ring=a.cols, max_rings=a.rings)
    fx.set_profiling(True)
    fx.extract_batch_device(d_all.data_ptr(), [per] * a.batch, stream)
    torch.cuda.synchronize()
    compact = fx.kernel_times().get("feature_compact_kernel", (0.0, 0))
    fx.set_profiling(False)
    fx.extract_batch_device(d_all.data_ptr(), [per] * a.batch, stream)
    v = fx.device_view()
    info = torch.zeros(4 * a.batch, dtype=torch.int32, device=dev)
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    torch.cuda.synchronize()
    hip.hipMemcpy(info.data_ptr(), int(v.scan_info), 16 * a.batch, 3)
    counts = info.cpu().numpy().reshape(a.batch, 4)
    records = int(counts[:, 2].sum() + counts[:, 3].sum())
    gbs, mhz = fx.box_calibration(0, stream)
    out = dict(metric="deskew_batch", rings=a.rings, cols=a.cols, batch=a.batch, feature_records=records,
               box_copy_gbs=round(gbs, 1), box_clock_mhz=round(mhz, 1),
               feature_compact_ms=round(compact[0] / max(compact[1], 1), 4))
    index = B.TimeField(B.TIME_FROM_INDEX, 0, 0, 0, 1.0)
    field = B.TimeField(B.TIME_FROM_FIELD, 24, B.FLOAT32, 0, 1.0)
    # (the C entry point itself, its arguments built once: the binding's per-call conversion of 1 024 sweeps would be what is timed)
    from lidar_feature_extraction_amd.extraction import _sweeps
    sw, _ = _sweeps([(0.0, 0.1, D)] * a.batch)
    L, ctx = fx._L, fx._ctx

    def deskew(tf, edge_out, surface_out):
        B.check(ctx, L.lfx_deskew_batch(ctx, C.byref(tf), sw, a.batch, B.DESKEW_TO_END, edge_out, surface_out, stream), L)
    other = (torch.zeros((a.batch * per + 1, 4), dtype=torch.float32, device=dev), torch.zeros((a.batch * per + 1, 4), dtype=torch.float32, device=dev))
    forms = [("out_of_place_index", index, 36), ("out_of_place_f32_field", field, 40)]
    dst = (other[0].data_ptr(), other[1].data_ptr())
    from lidar_feature_extraction_amd.extraction import _trajectories
    from tests import trajectory_cases as TC
    if a.kernels_only:                                # (for the profiler: see the docstring)
        for knots in [int(k) for k in a.trajectory_knots.split(",") if k]:
            times, poses = TC.turning(R.IDENTITY, knots=knots)
            tr, _, _keep = _trajectories([(times, poses, 1.0)] * a.batch)
            for _ in range(60):
                deskew(index, dst[0], dst[1])
                B.check(ctx, L.lfx_deskew_batch_trajectory(ctx, C.byref(index), tr, a.batch, dst[0], dst[1], stream), L)
            torch.cuda.synchronize()
        fx.close()
        return
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, tf, nbytes in forms:
        call = lambda: deskew(tf, dst[0], dst[1])   # noqa: E731
        t = time.perf_counter()
        n_warm = 0
        while time.perf_counter() - t < 0.25:
            call()
            n_warm += 1
        torch.cuda.synchronize()
        per_call = max((time.perf_counter() - t) / n_warm, 1e-6)
        calls = max(int(a.window / per_call) + 1, 4)
        spans = []
        for _ in range(a.repeats):
            ev0.record()
            for _ in range(calls):
                call()
            ev1.record()
            ev1.synchronize()
            spans.append(ev0.elapsed_time(ev1) / calls)
        ms = float(np.median(spans))
        out[name + "_us"] = round(ms * 1e3, 1)
        out[name + "_gbs"] = round(records * nbytes / (ms * 1e-3) / 1e9, 1)
        out[name + "_calls_per_window"] = calls
    for name, tf, nbytes in (("in_place_index", index, 36), ("in_place_f32_field", field, 40)):
        spans = []
        for i in range(5 + a.in_place_samples):
            fx.extract_batch_device(d_all.data_ptr(), [per] * a.batch, stream)
            ev0.record()
            deskew(tf, None, None)
            ev1.record()
            ev1.synchronize()
            if i >= 5:
                spans.append(ev0.elapsed_time(ev1))
        ms = float(np.median(spans))
        out[name + "_us"] = round(ms * 1e3, 1)
        out[name + "_gbs"] = round(records * nbytes / (ms * 1e-3) / 1e9, 1)
    # along trajectories: the whole call, and two of its parts alone
    for knots in [int(k) for k in a.trajectory_knots.split(",") if k]:
        times, poses = TC.turning(R.IDENTITY, knots=knots)
        tr, _, _keep = _trajectories([(times, poses, 1.0)] * a.batch)

        def along(edge_out, surface_out):
            B.check(ctx, L.lfx_deskew_batch_trajectory(ctx, C.byref(index), tr, a.batch, edge_out, surface_out, stream), L)
        key = "trajectory_%d_" % knots
        fx.extract_batch_device(d_all.data_ptr(), [per] * a.batch, stream)      # (the in-place samples before left the batch de-skewed)
        t = time.perf_counter()
        n_warm = 0
        while time.perf_counter() - t < 0.25:
            along(dst[0], dst[1])
            n_warm += 1
        torch.cuda.synchronize()
        calls = max(int(a.window / max((time.perf_counter() - t) / n_warm, 1e-6)) + 1, 4)
        spans = []
        for _ in range(a.repeats):
            ev0.record()
            for _ in range(calls):
                along(dst[0], dst[1])
            ev1.record()
            ev1.synchronize()
            spans.append(ev0.elapsed_time(ev1) / calls)
        out[key + "out_of_place_us"] = round(float(np.median(spans)) * 1e3, 1)
        spans = []
        for i in range(5 + a.in_place_samples):
            fx.extract_batch_device(d_all.data_ptr(), [per] * a.batch, stream)
            ev0.record()
            along(None, None)
            ev1.record()
            ev1.synchronize()
            if i >= 5:
                spans.append(ev0.elapsed_time(ev1))
        out[key + "in_place_us"] = round(float(np.median(spans)) * 1e3, 1)
        fx.extract_batch_device(d_all.data_ptr(), [per] * a.batch, stream)
        torch.cuda.synchronize()
        host = []
        for _ in range(20):
            torch.cuda.synchronize()
            t = time.perf_counter()
            along(dst[0], dst[1])
            host.append(time.perf_counter() - t)
        torch.cuda.synchronize()
        table = np.zeros((a.batch, knots - 1, B.TRAJECTORY_SEGMENT_DOUBLES))
        pinned = torch.from_numpy(table).pin_memory()
        d_table = torch.zeros_like(pinned, device=dev)
        copies = []
        for _ in range(20):
            ev0.record()
            d_table.copy_(pinned, non_blocking=True)
            ev1.record()
            ev1.synchronize()
            copies.append(ev0.elapsed_time(ev1))
        out[key + "table_bytes"] = int(table.nbytes)
        out[key + "call_host_us"] = round(float(np.median(host)) * 1e6, 1)
        out[key + "copy_us"] = round(float(np.median(copies)) * 1e3, 1)
    # the odometry with and without de-skew, scan by scan (batches of 1)
    n = a.odometry_scans
    if n:
        slow = R.pose([0.002, -0.003, 0.02], [0.3, 0.02, -0.005])
        p, seq, ends, true = R.pose([0.0, 0.0, 0.2], [-1.0, -1.5, 1.8]), [], [], []
        for i in range(n):
            seq.append(make_sweep(a.rings, a.cols, seed=9700 + i, pose0=p, motion=slow)[0])
            # (the sweep's true trajectory: 11 knots of the constant motion make_sweep was given)
            true.append((np.arange(11) / 10.0, np.stack([R.compose(p, R.scale(slow, k / 10.0)) for k in range(11)]), 1.0))
            p = R.compose(p, slow)
            ends.append(p)
        d_seq = torch.from_numpy(concat(seq).view(np.uint8).copy()).to(dev)
        for name in ("plain", "deskewed", "trajectory"):
            odo = fx.odometry(initial_pose=ends[0])
            total, timed, worst = 0.0, 0, 0.0
            for i in range(n):
                fx.extract_batch_device(d_seq.data_ptr() + i * per * 32, [per], stream)
                ev0.record()
                if name == "plain":
                    r = odo.update_batch(1, stream)[0]
                elif name == "deskewed":
                    r = odo.update_batch_deskewed(None, None, 1.0, "end", 1, stream)[0]
                else:
                    r = odo.update_batch_trajectory(None, [true[i]], 1, stream)[0]
                worst = max(worst, float(np.linalg.norm(r["pose"][:, 3] - ends[i][:, 3])))
                ev1.record()
                ev1.synchronize()
                if i >= n // 3:                       # (the first third warms the window up)
                    total += ev0.elapsed_time(ev1)
                    timed += 1
            out["odometry_%s_ms_per_scan" % name] = round(total / timed, 3)
            out["odometry_%s_worst_translation_error_m" % name] = round(worst, 4)
            odo.close()
    fx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
