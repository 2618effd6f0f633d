"""What the newer subsystems' GPU tests share (segmentation, scan context, the place index, the rolling map): the device
plumbing of tests/test_segment_gpu.py, a batch of 33 distinct 16 x 900 scans with the restatements' results made once, two
streams, and a hold -- a busy kernel of torch's that keeps a stream from running what is queued behind it."""
import time

import numpy as np

from tests import deskew_cases as K
from tests import segment_restatement as R

RINGS, COLS, N_SCANS = 16, 900, 33
HOLD_MS = 50.0                                # what a hold is sized for (the cap: the files stay at a few seconds)

_MADE = {}


def device_batch(fx, clouds):
    """clouds through the device path; the device buffer of their records, which the caller keeps alive."""
    from lidar_feature_extraction_amd import concat
    records = concat(clouds)
    d = K.upload_bytes(records) if len(records) else K.upload_bytes(np.zeros(32, np.uint8))
    fx.extract_batch_device(d.data_ptr(), [len(c) for c in clouds], K.stream())
    return d


def numpy_of(got):
    """segment()'s three tensors on the host, as the restatement's types (after a synchronise)."""
    K.sync()
    cls, ids, counts = got
    return cls.cpu().numpy(), ids.cpu().numpy().view(np.uint32), counts.cpu().numpy().view(np.uint32)


def same(got, want, what):
    for name, g, w in zip(("class", "id", "counts"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            raise AssertionError((what, name, len(bad), bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def same_floats(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError((what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def seg_outputs(total, n_scans):
    """Outputs of one lfx_segment_batch call, marked."""
    import torch
    return (torch.full((total,), 77, dtype=torch.uint8, device=K.dev()), torch.full((total,), 77, dtype=torch.int32, device=K.dev()),
            torch.full((n_scans, 4), 77, dtype=torch.int32, device=K.dev()))


def scans33():
    """33 scans of 16 x 900, no two alike: the five synthetic scans of the segmentation tests as they are, each in five
    seeded permutations of its records, and three of them with 5 % of the records dropped.  Made once."""
    from lidar_feature_extraction_amd import make_scan
    if "scans" not in _MADE:
        base = [make_scan(RINGS, COLS, seed=700 + s, sensor_pose=(1.5 * s - 3.0, 0.4 * s, 0.3 * s)) for s in range(5)]
        out = list(base)
        for s, c in enumerate(base):
            for p in range(5):
                out.append(np.ascontiguousarray(c[np.random.default_rng(1000 + 10 * s + p).permutation(len(c))]))
        for s in range(3):
            c = base[s]
            out.append(np.ascontiguousarray(c[np.random.default_rng(2000 + s).uniform(0, 1, len(c)) >= 0.05]))
        assert len(out) == N_SCANS and len({c.tobytes() for c in out}) == N_SCANS
        _MADE["scans"] = out
    return _MADE["scans"]


def fx33():
    """A context that takes the 33 scans and images of up to 128 rows."""
    from lidar_feature_extraction_amd import FeatureExtraction
    return FeatureExtraction(device=0, max_points_per_scan=RINGS * COLS, max_batch=N_SCANS, max_points_per_ring=COLS, max_rings=128)


def segment_want(n, **fields):
    """The restatement's (class, id, counts) of the first n of the 33 scans under R.config(**fields); every scan's result is
    made once per config and kept (128 x 4096 x 33 takes a while on the host)."""
    key = ("segment",) + tuple(sorted(fields.items()))
    if key not in _MADE:
        cfg = R.config(**fields)
        _MADE[key] = [R.segment_cloud(cfg, c) for c in scans33()]
    per = _MADE[key][:n]
    return np.concatenate([p[0] for p in per]), np.concatenate([p[1] for p in per]), np.stack([p[2] for p in per])


def descriptors_want(n, **fields):
    """The scan-context restatement's descriptors [n][R][S] of the first n of the 33 scans, every scan's made once per config."""
    from tests import scan_context_restatement as SC
    key = ("descriptor",) + tuple(sorted(fields.items()))
    if key not in _MADE:
        cfg = SC.config(**fields)
        _MADE[key] = [SC.descriptor_of_cloud(cfg, c) for c in scans33()]
    return np.stack(_MADE[key][:n])


# --- streams -----------------------------------------------------------------------------------------------------------------
def two_streams():
    import torch
    return torch.cuda.Stream(), torch.cuda.Stream()


class Hold:
    """hold(stream): a busy kernel of torch's queued on `stream`, sized to run for about HOLD_MS (torch.cuda._sleep, its
    cycles per millisecond measured once on this device; without it a chain of matmuls, measured likewise).  What is queued
    on the stream afterwards has not run while an event recorded behind it says so: the tests assert exactly that."""

    def __init__(self):
        import torch
        self.sleep = getattr(torch.cuda, "_sleep", None)
        self.a = None
        if self.sleep is None:
            self.a = torch.rand((2048, 2048), dtype=torch.float32, device=K.dev())
        self.unit = 1000000 if self.sleep is not None else 4
        self._run(self.unit, torch.cuda.current_stream())                # (the first launch pays for loading the kernel)
        K.sync()
        took = []
        for _ in range(3):                                               # (the least of three: a neighbour's work only adds)
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record()
            self._run(self.unit, torch.cuda.current_stream())
            end.record()
            K.sync()
            took.append(begin.elapsed_time(end))
        self.ms_per_unit = max(min(took), 1e-3)
        self.amount = max(1, int(self.unit * HOLD_MS / self.ms_per_unit))
        self.issue_ms = []

    def _run(self, amount, stream):
        import torch
        with torch.cuda.stream(stream):
            if self.sleep is not None:
                self.sleep(int(amount))
            else:
                b = self.a
                for _ in range(int(amount)):
                    b = (b @ self.a) * 4.8828125e-4
                self.a_keep = b

    def __call__(self, stream):
        self.began = time.perf_counter()
        self._run(self.amount, stream)

    def still_held(self, event, what):
        """The assertion a held case rests on: `event`, recorded behind the producer, has not been reached.  The time since
        the hold was queued is kept for the report."""
        ms = 1e3 * (time.perf_counter() - self.began)
        assert not event.query(), "%s: the producer had run %.2f ms after its hold of about %.0f ms was queued" % (what, ms, HOLD_MS)
        self.issue_ms.append((what, ms))
        return ms


def event_behind(stream):
    import torch
    e = torch.cuda.Event()
    e.record(stream)
    return e
