"""tools/covariance_check.py -- how far the reported covariance is from the scatter of the poses (GPU box).

  python3 tools/covariance_check.py [--rings 64] [--cols 1800] [--scans 200] [--map-scans 8] [--sigma 0.01] [--batch 25]

`scans` scans taken at ONE pose of the synthetic room, each with range noise of its own seed (sigma metres), are localized
from one initial pose against one fixed map built from the features of `map-scans` scans of other seeds.  Per coordinate,
in the order of geometry_msgs/PoseWithCovariance (x y z, rotation about X Y Z; lfx_align_covariance_ros): the empirical
standard deviation of the poses, the mean predicted one (square root of the mean reported variance), and their ratio.

The reported covariance is the Gauss-Newton one, sigma2 * H^-1 from the scan's own rows: it knows nothing of the map's noise
(which is common to all the scans here and so moves their mean, not their scatter), of wrong associations, of the
discreteness of which points become features, or of the robust scale's variance.  The ratio says how much a binder should
inflate it on a scene like this one; nothing bounds it.  One JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rotation_vector(R):
    """The rotation vector of a rotation matrix close to the identity (fixed axes)."""
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2.0
    s = np.linalg.norm(w)
    return w if s < 1e-12 else w * (np.arcsin(min(s, 1.0)) / s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--cols", type=int, default=1800)
    ap.add_argument("--scans", type=int, default=200)
    ap.add_argument("--map-scans", type=int, default=8)
    ap.add_argument("--sigma", type=float, default=0.01)
    ap.add_argument("--batch", type=int, default=25)
    ap.add_argument("--cell", type=float, default=1.0)
    a = ap.parse_args()
    import torch
    from lidar_feature_extraction_amd import FeatureExtraction, concat, covariance_ros, make_scan
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    fx = FeatureExtraction(device=0, max_points_per_scan=a.rings * a.cols, max_batch=max(a.batch, a.map_scans), max_points_per_ring=a.cols,
                           max_rings=a.rings)

    def extract(seeds):
        clouds = [make_scan(a.rings, a.cols, seed=s, sigma=a.sigma) for s in seeds]
        d = torch.from_numpy(concat(clouds).view(np.uint8).copy()).to(dev)
        fx.extract_batch_device(d.data_ptr(), [len(c) for c in clouds], stream)
        return d

    keep = extract([30000 + i for i in range(a.map_scans)])
    scans = [fx.download(s, stream) for s in range(a.map_scans)]
    edge_map = np.ascontiguousarray(np.concatenate([s.edge_points for s in scans]), np.float32)
    surf_map = np.ascontiguousarray(np.concatenate([s.surface_points for s in scans]), np.float32)
    emap, smap = fx.make_map_from_host(edge_map, a.cell), fx.make_map_from_host(surf_map, a.cell)
    start = np.array([[1, 0, 0, 0.02], [0, 1, 0, -0.015], [0, 0, 1, 0.01]], np.float64)
    poses, variances, codes, degenerate, ranks = [], [], {}, 0, []
    for at in range(0, a.scans, a.batch):
        n = min(a.batch, a.scans - at)
        keep = extract([20000 + at + i for i in range(n)])
        res, reps = fx.localize_batch(emap, smap, np.repeat(start[None], n, 0), 15, 20, 1.0, stream, report=True)
        for r, rep in zip(res, reps):
            codes[str(r["code"])] = codes.get(str(r["code"]), 0) + 1
            if not rep["valid"]:
                continue
            degenerate += int(rep["degenerate"])
            ranks.append(rep["rank"])
            poses.append(np.concatenate([r["pose"][:, 3], rotation_vector(r["pose"][:, :3])]))
            variances.append(np.diag(covariance_ros(r["pose"], rep["covariance"])))
    del keep
    poses, variances = np.array(poses), np.array(variances)
    empirical = poses.std(axis=0, ddof=1)
    predicted = np.sqrt(variances.mean(axis=0))
    print(json.dumps({
        "rings": a.rings, "cols": a.cols, "scans": a.scans, "with_report": len(poses), "map_scans": a.map_scans, "sigma": a.sigma,
        "edge_map_points": len(edge_map), "surface_map_points": len(surf_map), "codes": codes, "degenerate": degenerate,
        "rank_min": int(min(ranks)) if ranks else None, "order": ["x", "y", "z", "rx", "ry", "rz"],
        "mean_pose": [float(v) for v in poses.mean(axis=0)], "empirical_std": [float(v) for v in empirical],
        "predicted_std": [float(v) for v in predicted], "empirical_over_predicted": [float(v) for v in empirical / predicted]}))
    emap.close()
    smap.close()
    fx.close()


if __name__ == "__main__":
    main()
