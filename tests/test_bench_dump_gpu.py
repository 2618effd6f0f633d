"""bench.py --dump-outputs: what the last timed step computed, written as .npy files, is what the CPU oracle computes for the
same seeded scans -- so that two builds of the library can be compared output for output through the bench itself.  And
--steps is the number of timed steps, and a run without --full measures the headline alone."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_refuses_zero_steps():
    """(CPU) a timed region of no step is refused before anything touches a device."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, cwd=ROOT, timeout=120)
    assert p.returncode == 2 and b"--steps must be at least 1" in p.stderr, p.stderr[-2000:]


@pytest.mark.gpu
def test_a_plain_run_measures_the_headline_alone():
    """Without --full the line holds the headline and the figures its own timed region gives; nothing that takes a run or a
    check of its own (box calibration, the oracle, the host API, the consumer) is measured, the CPU baseline included."""
    batch, steps = 24, 3
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rings", "16", "--cols", "900", "--batch", str(batch),
           "--unique", "5", "--steps", str(steps), "--warmup", "1", "--warm-seconds", "0"]
    p = subprocess.run(cmd, capture_output=True, cwd=ROOT, timeout=420)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == 1 and d["unit"] == "scans/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["value"] > 0 and abs(d["value"] - batch * steps / (d["ms_per_step"] * steps * 1e-3)) / d["value"] < 1e-3
    assert d["roofline"]["frac"] > 0 and d["roofline"]["kernel_us_per_launch"]
    for k in ("box", "parity_spot_check", "cpu_baseline", "end_to_end", "consumer", "configs"):
        assert d[k] is None, (k, d[k])


@pytest.mark.gpu
def test_bench_dump_outputs_match_the_oracle(tmp_path):
    from lidar_feature_extraction_amd import make_scan
    from oracle import binding as OB
    rings, cols, batch, unique = 16, 900, 24, 5
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rings", str(rings), "--cols", str(cols),
           "--batch", str(batch), "--unique", str(unique), "--steps", "2", "--warmup", "1", "--warm-seconds", "0",
           "--full", "--no-cpu-baseline", "--dump-outputs", str(out)]
    p = subprocess.run(cmd, capture_output=True, cwd=ROOT, timeout=420)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["repeats"] == 1 and d["parity_spot_check"] is True

    files = sorted(glob.glob(str(out / "*.npy")))
    arrays = {os.path.basename(f)[:-4]: np.load(f) for f in files}
    assert sum(os.path.getsize(f) for f in files) <= 64 * 1000 * 1000
    assert all(v.dtype in (np.float32, np.float64) for v in arrays.values())
    scans = arrays["scans"].astype(np.int64)
    assert len(scans) == 16 and len(set(scans[:, 0])) == 16 and scans[:, 0].max() < batch
    at = {k: 0 for k in ("p", "s", "e", "f", "r")}
    for j, n, n_sorted, ne, ns, nr in scans:
        cloud = make_scan(rings, cols, seed=1234 + j % unique, vfov_deg=15.0)      # bench.py's stream: scan j is clouds[j % unique]
        w = OB.extract(cloud, canonical_ties=False)
        assert n == len(cloud)
        labels = arrays["labels"][at["p"]:at["p"] + n]
        curvature = arrays["curvature"][at["p"]:at["p"] + n]
        edge_index = arrays["edge_index"][at["e"]:at["e"] + ne]
        surface_index = arrays["surface_index"][at["f"]:at["f"] + ns]
        assert np.array_equal(labels, w["labels"].astype(np.float32)), "scan %d: labels" % j
        assert curvature.tobytes() == w["curvature"].tobytes(), "scan %d: curvature bits" % j
        assert np.array_equal(edge_index, w["edge_index"].astype(np.float64)), "scan %d: edge index" % j
        assert np.array_equal(surface_index, w["surface_index"].astype(np.float64)), "scan %d: surface index" % j
        assert arrays["edge_points"][at["e"]:at["e"] + ne].tobytes() == w["edge_points"].tobytes(), "scan %d: edge cloud" % j
        assert arrays["surface_points"][at["f"]:at["f"] + ns].tobytes() == w["surface_points"].tobytes(), "scan %d: surface cloud" % j
        assert np.array_equal(arrays["sorted_index"][at["s"]:at["s"] + n_sorted], w["sorted_index"].astype(np.float64)), "scan %d: sorted index" % j
        assert np.array_equal(arrays["ring_count"][at["r"]:at["r"] + nr], w["ring_count"].astype(np.float64)), "scan %d: ring counts" % j
        at["p"] += n
        at["s"] += n_sorted
        at["e"] += ne
        at["f"] += ns
        at["r"] += nr
    assert at["p"] == len(arrays["labels"]) and at["e"] == len(arrays["edge_index"]) and at["r"] == len(arrays["ring_id"])
