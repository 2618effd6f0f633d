"""What the de-skew GPU tests share: sweeps along an arc, the device plumbing, the comparison with the restatement."""
import ctypes as C

import numpy as np

from tests import deskew_restatement as R


def dev():
    import torch
    return torch.device("cuda", 0)


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def sync():
    import torch
    torch.cuda.synchronize()


def upload_bytes(records):
    """The records of a batch (any 32-byte dtype) as a device tensor of bytes."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(-1).copy()).to(dev())


def arc(start, motion, n):
    """n sweeps one after the other: (P0_k, P1_k) with P0_0 = start, P1_k = P0_k motion, P0_{k+1} = P1_k."""
    out, p = [], np.asarray(start, np.float64).reshape(3, 4)
    for _ in range(n):
        q = R.compose(p, motion)
        out.append((p, q))
        p = q
    return out


def fx_for(rings, cols, batch, **kw):
    from lidar_feature_extraction_amd import FeatureExtraction
    return FeatureExtraction(device=0, max_points_per_scan=rings * cols, max_batch=batch, max_points_per_ring=cols, max_rings=rings, **kw)


def extract(fx, clouds):
    """clouds through the device path: the device buffer (the caller keeps it alive) and every scan's download()."""
    from lidar_feature_extraction_amd import concat
    d = upload_bytes(concat(clouds))
    fx.extract_batch_device(d.data_ptr(), [len(c) for c in clouds], stream())
    return d, [fx.download(s, stream()) for s in range(len(clouds))]


def out_buffers(total):
    import torch
    return torch.zeros((total + 1, 4), dtype=torch.float32, device=dev()), torch.zeros((total + 1, 4), dtype=torch.float32, device=dev())


def slices(buffers, clouds, got):
    """Scan s's records of two buffers laid out like the context's clouds."""
    sync()
    e, s = buffers[0].cpu().numpy(), buffers[1].cpu().numpy()
    begin = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    return [(e[begin[k]:begin[k] + len(g.edge_points)].copy(), s[begin[k]:begin[k] + len(g.surface_points)].copy()) for k, g in enumerate(got)]


def compare(gpu, ref, what):
    """The tolerance of the issue: per coordinate |gpu - ref| <= spacing_f32(ref) + 1e-12; the 4th floats equal.  Returns
    (coordinates that differ at all, coordinates)."""
    gpu, ref = np.asarray(gpu, np.float32), np.asarray(ref, np.float32)
    assert gpu.shape == ref.shape, (what, gpu.shape, ref.shape)
    assert gpu[:, 3].tobytes() == ref[:, 3].tobytes(), what
    g, r = gpu[:, :3].astype(np.float64), ref[:, :3].astype(np.float64)
    tol = np.spacing(np.abs(ref[:, :3])).astype(np.float64) + 1e-12
    bad = np.abs(g - r) > tol
    assert not bad.any(), (what, int(bad.sum()), g[bad][:4], r[bad][:4])
    return int((gpu[:, :3] != ref[:, :3]).sum()), int(ref[:, :3].size)


def d2h(ptr, n_records, floats=4):
    out = np.zeros((int(n_records), floats), np.float32)
    if n_records:
        sync()
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(out.ctypes.data, int(ptr), out.nbytes, 2) == 0
    return out
