"""tools/mapping_bench.py -- the keyframe mapper (lfx_mapper_add, SURVEY.md 8f, the mapping row) and the map files on one
MI355X, beside the CPU restatement of MapBuilder::Callback.

  python3 tools/mapping_bench.py [--rings 64] [--cols 1800] [--scans 64] [--calls 20] [--odometry-scans 32]
                                 [--pcd-points 10000000] [--skip-pcd] [--out FILE]

add_all: lfx_mapper_add of a batch of `scans` extracted scans' edge clouds with thresholds 0 (every cloud added), `calls`
calls, each on its own mapper, made before the timed calls, whose capacity holds the call (no growth); HIP events around
the call (it waits for the counts once, then queues one map_append_kernel; the span ends behind the kernel), median.  The
script calls hipMemGetInfo once before these calls and once after them: a HIP trace shows that nothing is allocated in
between.  add_default: the same batch
again and again with the default thresholds on one mapper (add_default_outcomes: what its first call decided).
odometry: ms per scan of lfx_odometry_update_batch (batches of 1) alone, and with two mappers fed its poses.  pcd: host
write and read rates of a map of `pcd-points` random records: binary as lfx_pcd_write writes it, and the same records as
binary_compressed (random floats do not compress: the block is literal runs of 32 bytes, what an LZF encoder leaves of
such data), and lfx_map_create_host from what was read.  cpu: the
numpy restatement of MapBuilder::Callback (tests/mapping_restatement.py) per scan.  For map_append_kernel's own time run
this under `rocprofv3 --kernel-trace --stats`: every add call that adds a cloud shows exactly one map_append_kernel
(`adding_calls` in the output counts those calls)."""
import ctypes as C
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _marker():
    """hipMemGetInfo through the HIP runtime the library is bound to: a mark in a HIP trace"""
    from lidar_feature_extraction_amd import binding
    L = binding.load()
    free, total = C.c_size_t(), C.c_size_t()
    L.hipMemGetInfo(C.byref(free), C.byref(total))


def _literal_lzf(raw):
    """raw bytes as one LZF block of literal runs (control byte 31, then 32 bytes; a shorter run at the end)"""
    b = np.frombuffer(raw, np.uint8)
    full = len(b) // 32
    body = np.empty((full, 33), np.uint8)
    body[:, 0] = 31
    body[:, 1:] = b[:full * 32].reshape(full, 32)
    tail = b[full * 32:]
    return body.tobytes() + (bytes([len(tail) - 1]) + tail.tobytes() if len(tail) else b"")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--cols", type=int, default=1800)
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--odometry-scans", type=int, default=32)
    ap.add_argument("--pcd-points", type=int, default=10_000_000)
    ap.add_argument("--skip-pcd", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from lidar_feature_extraction_amd import FeatureExtraction, Mapper, ScanMap, concat, make_sequence, read_pcd, write_pcd
    from tests.mapping_restatement import MapBuilder
    per = a.rings * a.cols
    clouds, truth = make_sequence(a.scans, a.rings, a.cols, seed=9500, step=0.25, yaw_step_deg=1.0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    d_all = torch.from_numpy(concat(clouds).view(np.uint8).copy()).to(dev)
    fx = FeatureExtraction(device=0, max_points_per_scan=per, max_batch=a.scans, max_points_per_ring=a.cols, max_rings=a.rings)
    fx.extract_batch_device(d_all.data_ptr(), [per] * a.scans, stream)
    feats = [fx.download(s, stream) for s in range(a.scans)]
    n_edge = sum(len(f.edge_points) for f in feats)
    out = dict(metric="mapper_add", rings=a.rings, cols=a.cols, scans=a.scans, edge_records=n_edge,
               bytes_moved=2 * 16 * n_edge)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        ev0.record()
        r = fn()
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1), r

    calls = dict(add=0, adding=0)

    def add_batch(m, which, poses):
        r = m.add_batch(which, poses, stream)
        calls["add"] += 1
        calls["adding"] += int((r == 0).any())
        return r

    # thresholds 0: every cloud added; a mapper per call, made before the calls, its capacity holding the call
    mappers = [Mapper(fx, translation_threshold=0.0, rotation_threshold=0.0, initial_capacity_points=n_edge + 1)
               for _ in range(a.calls + 2)]
    torch.cuda.synchronize()
    _marker()                                      # (the warmed calls begin: no allocation until the next mark)
    spans = []
    for k, m in enumerate(mappers):
        ms, res = timed(lambda: add_batch(m, "edge", truth))
        assert int((res == 0).sum()) == sum(len(f.edge_points) > 0 for f in feats)
        if k >= 2:
            spans.append(ms)
    _marker()                                      # (they end)
    for m in mappers:
        m.close()
    out["add_all_ms"] = float(np.median(spans))
    out["add_all_gbs"] = out["bytes_moved"] / (out["add_all_ms"] * 1e-3) / 1e9
    # default thresholds, the batch again and again on one mapper
    m = Mapper(fx)
    first = add_batch(m, "edge", truth)
    out["add_default_outcomes"] = [int((first == k).sum()) for k in range(3)]
    spans = [timed(lambda: add_batch(m, "edge", truth))[0] for _ in range(a.calls + 2)][2:]
    out["add_default_ms"] = float(np.median(spans))
    m.close()
    # odometry alone, and with two mappers fed its poses (batches of 1, the node's order)
    n_odo = min(a.odometry_scans, a.scans)
    fx1 = FeatureExtraction(device=0, max_points_per_scan=per, max_batch=1, max_points_per_ring=a.cols, max_rings=a.rings)
    for mapping in (False, True):
        odo = fx1.odometry()
        em, sm = Mapper(fx1), Mapper(fx1)
        total = 0.0
        for s in range(n_odo):
            fx1.extract_batch_device(d_all.data_ptr() + s * per * 32, [per], stream)

            def step():
                p = odo.update_batch(1, stream)[0]["pose"]
                if mapping:
                    add_batch(em, "edge", p)
                    add_batch(sm, "surface", p)
            ms, _ = timed(step)
            if s >= 4:
                total += ms
        out["odometry%s_ms_per_scan" % ("_two_mappers" if mapping else "")] = total / (n_odo - 4)
        if mapping:
            out["odometry_map_points"] = [int(em.view()["n_points"]), int(sm.view()["n_points"])]
        em.close(); sm.close(); odo.close()
    fx1.close()
    # CPU: the restatement of MapBuilder::Callback per scan (the transform in numpy, the gate in Python)
    ref = MapBuilder(0.0, 0.0)
    t0 = time.perf_counter()
    for f, p in zip(feats, truth):
        ref.callback(f.edge_points, p)
    out["cpu_restatement_ms_per_scan_add_all"] = (time.perf_counter() - t0) * 1e3 / a.scans
    # PCD rates on the host
    if not a.skip_pcd:
        rng = np.random.default_rng(1)
        big = rng.normal(0, 50, (a.pcd_points, 4)).astype(np.float32)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "map.pcd")
            t0 = time.perf_counter()
            write_pcd(path, big)
            out["pcd_write_binary_mrec_per_s"] = a.pcd_points / (time.perf_counter() - t0) / 1e6
            t0 = time.perf_counter()
            got = read_pcd(path, drop_nonfinite=True)
            out["pcd_read_binary_mrec_per_s"] = a.pcd_points / (time.perf_counter() - t0) / 1e6
            t0 = time.perf_counter()
            smap = ScanMap(fx, 0, 0, 1.0, stream, host_points=got)
            torch.cuda.synchronize()
            out["map_create_host_ms"] = (time.perf_counter() - t0) * 1e3
            out["pcd_points"] = a.pcd_points
            smap.close()
            # the same records as binary_compressed: x, y, z one field after another, one LZF block
            raw = b"".join(np.ascontiguousarray(big[:, k]).tobytes() for k in range(3))
            block = _literal_lzf(raw)
            n = a.pcd_points
            head = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\n"
                    "WIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary_compressed\n" % (n, n)).encode()
            cpath = os.path.join(d, "c.pcd")
            with open(cpath, "wb") as f:
                f.write(head + np.array([len(block), len(raw)], "<u4").tobytes() + block)
            del raw, block
            t0 = time.perf_counter()
            back = read_pcd(cpath)
            out["pcd_read_compressed_mrec_per_s"] = n / (time.perf_counter() - t0) / 1e6
            assert back[:, :3].tobytes() == big[:, :3].tobytes()
    fx.close()
    out["add_calls"], out["adding_calls"] = calls["add"], calls["adding"]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
