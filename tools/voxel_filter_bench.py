"""Times of the voxel filter (lfx_voxel_filter) over the store of tools/keyframes_bench.py: N keyframes whose per-keyframe
counts come from a real extraction of `synth` 64 x 1800 scans, on two laps of a circle; one JSON line.

    python tools/voxel_filter_bench.py [--keyframes 10000] [--scans 64] [--runs 3] [--out FILE]

Per kind (edge at leaf 0.2, surface at leaf 0.4) and per masked share 0 / 0.05 / 0.5 (flags drawn per record into the store's own
flags; share 0 is the unmasked call, which reads no flag), medians of --runs:

  add_keyframes_us   lfx_voxel_filter_add_keyframes over the whole store, HIP events around the call (the reset before it is
                     not timed); _gb_s: the 16 bytes read per record per second, beside lfx_box_calibration's copy rate
  emit_us            lfx_voxel_filter_emit of everything, wall clock to the stream's end (it waits once, for its result)
  kept               voxels written / records accumulated
  load               occupied entries / entries of the table

and once per kind build_us, lfx_keyframes_build of the same range into a device buffer (HIP events): one pass over the records
that writes the world cloud the filter does without.  The table is sized as INTEGRATION.md section 5 says: a first pass into a
table of at least as many entries as records counts the voxels, the timed filter has the next power of two above twice those.

Which form of the add is timed is decided by the library: LFX_LIB_PATH names another build.  The A/B builds of DESIGN.md
section 7 are `make variant NAME=liblfx_vf_noblock EXTRA=-DLFX_VF_BLOCK=0` (equal neighbours of a wave merged, no table of the
workgroup's own) and `make variant NAME=liblfx_vf_unmerged EXTRA="-DLFX_VF_MERGE=0 -DLFX_VF_BLOCK=0"` (every record its own
atomics on the global table)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lidar_feature_extraction_amd import FeatureExtraction, Keyframes, concat, make_scan  # noqa: E402
from tools.keyframes_bench import circle  # noqa: E402

LEAVES = (0.2, 0.4)
SHARES = (0.0, 0.05, 0.5)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=10000)
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
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
    line = dict(keyframes=n, edge_records=int(total[0]), surface_records=int(total[1]), library=os.environ.get("LFX_LIB_PATH", "liblfx.so"))

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
    for first in range(0, n, batch):
        m = min(batch, n - first)
        v = fx.device_view()
        cap = fx.max_points_per_scan * fx.max_batch
        info = int(v.scan_info)
        kf.add(Keyframes.clouds(v.edge_points, v.scan_begin, info + 8, 4, cap), Keyframes.clouds(v.surface_points, v.scan_begin, info + 12, 4, cap),
               poses[first:first + m], stream)
    torch.cuda.synchronize()
    assert kf.info()["n_points"] == (int(total[0]), int(total[1]))
    kf.reserve_flags(stream)
    line["copy_gb_s"] = [round(fx.box_calibration(0, stream)[0], 1) for _ in range(a.runs)]
    rng = np.random.default_rng(5)
    for kind, name in ((0, "edge"), (1, "surface")):
        records, leaf = int(total[kind]), LEAVES[kind]
        out = torch.empty((records, 4), dtype=torch.float32, device=dev)
        kf.build(kind, 0, n, d_out=out.data_ptr(), capacity_points=records, stream=stream)
        us = float(np.median([events(lambda: kf.build(kind, 0, n, d_out=out.data_ptr(), capacity_points=records, stream=stream)) for _ in range(a.runs)]))
        line["build_%s_us" % name] = us
        line["build_%s_gb_s" % name] = round(32.0 * records / (1e3 * us), 1)
        # the sizing pass: a table nobody can fill counts the voxels
        sizing = fx.voxel_filter(max(4, int(np.ceil(np.log2(max(records, 2))))), records)
        sizing.reset(leaf, stream)
        sizing.add_keyframes(kf, kind, stream=stream)
        rc, res = sizing.emit_raw(1, out.data_ptr(), records, 0, stream)
        assert rc == 0, (rc, res)
        sizing.close()
        log2_slots = min(30, max(4, int(np.ceil(np.log2(2 * max(res["n_voxels"], 1))))))
        vf = fx.voxel_filter(log2_slots, records)
        line["%s_log2_slots" % name] = log2_slots
        line["%s_device_bytes" % name] = vf.info()["device_bytes"]
        for share in SHARES:
            drawn = torch.from_numpy((rng.random(records) < share).astype(np.uint8)).to(dev)
            kf.set_flags(kind, drawn, 0, n, stream)
            del drawn
            add_us, emit_us = [], []
            for _ in range(a.runs + 1):
                vf.reset(leaf, stream)
                add_us.append(events(lambda: vf.add_keyframes(kf, kind, masked=share > 0.0, stream=stream)))
                t, (rc, res) = wall(lambda: vf.emit_raw(1, out.data_ptr(), records, 0, stream))
                assert rc == 0, (rc, res)
                emit_us.append(t)
            add, emit = float(np.median(add_us[1:])), float(np.median(emit_us[1:]))          # (the first run warms the kernels)
            line["%s_leaf_%g_share_%g" % (name, leaf, share)] = dict(
                add_keyframes_us=add, add_keyframes_gb_s=round(16.0 * records / (1e3 * add), 1), emit_us=emit, n_accumulated=res["n_accumulated"],
                n_voxels=res["n_voxels"], kept=round(res["n_written"] / max(res["n_accumulated"], 1), 4),
                load=round(res["n_voxels"] / float(1 << log2_slots), 4))
        vf.close()
        del out
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    kf.close()
    fx.close()


if __name__ == "__main__":
    main()
