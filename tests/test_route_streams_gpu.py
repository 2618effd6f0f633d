"""The route selection over whole streams ON THE DEVICE, unpinned: one context per run, a batch of eight 16 x 600 scans of one
kind per call, every batch waited for (its report must have landed before the next choice).  What a batch was run as is read
off lfx_kernel_times -- profiling on, every batch sampled: the launch counts of ring_unit_org_kernel, ring_cut_kernel and
grid_count_kernel (the slot covers scan_count_kernel) are the device's (fused, xform, holes) -- and off lfx_scan_routes.
  1  those equal what the closed loop of tests/route_stream_model.py gives, batch for batch: every kind alone, the two streams
     the machine used never to leave (turned rings with zero records; the holes hint where the form cannot run), six
     transitions.  This is what holds the report model, and with it tests/test_route_streams.py, to the kernels;
  2  in every batch two scans equal the oracle in full (the two move through the batch from call to call), and every scan's
     route word is the one the form implies;
  3  the holes hint without the zero filter: a ragged stream is on the bucketing route within the bound, a clean one stays
     fused without a count pass ever launched;
  4  past the settling bound at most one batch in any 16 consecutive ones runs the organised-scan kernel for more than a
     quarter of its scans to end on route 0."""
import collections

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from lidar_feature_extraction_amd import FeatureExtraction, concat, make_scan  # noqa: E402
from lidar_feature_extraction_amd import binding as LB  # noqa: E402
from oracle import binding as OB  # noqa: E402
from tests import route_stream_model as M  # noqa: E402
from tests.parity import assert_filtered_equal  # noqa: E402
from tests.test_gpu_parity import _zeroed  # noqa: E402

R, COLS, NB = 16, 600, 8
HINT = {"unknown": LB.STREAM_UNKNOWN, "turned_rings": LB.STREAM_TURNED_RINGS, "no_grid": LB.STREAM_NO_GRID,
        "grid_with_holes": LB.STREAM_GRID_WITH_HOLES}
SLOTS = ("ring_unit_org_kernel", "ring_cut_kernel", "grid_count_kernel", "ring_scatter_kernel")


def _make(kind, i):
    """Scan i of a kind: (records, mask of its zero records)."""
    if kind == "clean":
        c = make_scan(R, COLS, seed=5100 + i)
    elif kind == "turned":
        c = make_scan(R, COLS, seed=5200 + i, start_col=77)
    elif kind == "holes":
        return _zeroed(make_scan(R, COLS, seed=5300 + i), 0.06, 80 + i)
    elif kind == "turned_holes":
        return _zeroed(make_scan(R, COLS, seed=5400 + i, start_col=77), 0.06, 90 + i)
    elif kind == M.SPARSE:
        return _zeroed(make_scan(R, COLS, seed=5500 + i, start_col=77), 0.002, 100 + i)
    elif kind == "ragged":
        # (a length that happens to be a multiple of the ring count would read as a grid with the wrong ring ids: another stream)
        c = next(c for c in (make_scan(R, COLS, seed=5600 + 10 * i + k, drop_fraction=0.1) for k in range(10)) if len(c) % R)
    else:
        assert kind == "shuffled", kind
        c = make_scan(R, COLS, seed=5700 + i, shuffle=True)
    return c, np.zeros(len(c), bool)


class Streams:
    """Eight distinct scans per kind, on the host and (back to back) on the device; one oracle result per scan, computed once."""

    def __init__(self):
        import torch
        self.torch = torch
        self.stream = torch.cuda.current_stream().cuda_stream
        self.scans, self.dev, self.n, self.want = {}, {}, {}, {}

    def kind(self, kind):
        if kind not in self.scans:
            self.scans[kind] = [_make(kind, i) for i in range(NB)]
            clouds = [c for c, _ in self.scans[kind]]
            self.dev[kind] = self.torch.from_numpy(concat(clouds).view(np.uint8).copy()).cuda()
            self.n[kind] = np.array([len(c) for c in clouds], np.uint32)
        return self.scans[kind]

    def oracle(self, kind, i, drop_zero):
        """(result on the records the context keeps, their indices, the mask of the dropped ones)"""
        key = (kind, i, drop_zero)
        if key not in self.want:
            c, zero = self.kind(kind)[i]
            zero = zero if drop_zero else np.zeros(len(c), bool)
            keep = np.nonzero(~zero)[0]
            self.want[key] = (OB.extract(np.ascontiguousarray(c[keep]), canonical_ties=False), keep, zero)
        return self.want[key]


@pytest.fixture(scope="module")
def streams():
    return Streams()


@pytest.fixture(scope="module")
def lib():
    return M.load()


Seen = collections.namedtuple("Seen", "kind fused xform holes scatter routes ms")


def run_on_device(S, phases, hint="unknown", drop_zero=True):
    """The phases on a fresh context; per batch what was launched, the scans' routes and the kernels' time.  Two scans of every
    batch are held to the oracle, and every scan's route to the form the batch was run in."""
    f = FeatureExtraction(device=0, max_points_per_scan=R * COLS, max_batch=NB, max_points_per_ring=COLS, max_rings=R,
                          drop_zero_points=drop_zero, stream_hint=HINT[hint])
    f.set_profiling(True)
    seen, before, t = [], f.kernel_times(), 0
    try:
        for kind, n in phases:
            S.kind(kind)
            for _ in range(n):
                f.extract_batch_device(S.dev[kind].data_ptr(), S.n[kind], S.stream)
                routes = f.scan_routes(NB, S.stream).tolist()
                S.torch.cuda.synchronize()
                now = f.kernel_times()
                launched = [now[k][1] - before[k][1] for k in SLOTS]
                ms = sum(now[k][0] - before[k][0] for k in now)
                before = now
                assert all(v in (0, 1) for v in launched), "batch %d: launches %s" % (t, dict(zip(SLOTS, launched)))
                fused, xform, holes, scatter = launched
                what = "hint %s, batch %d (%s, %s)" % (hint, t, kind, "fused %d xform %d holes %d" % (fused, xform, holes))
                code = 0 if not fused else (2 if xform else (3 if holes else 1))
                assert set(routes) <= {0, code}, "%s: routes %s" % (what, routes)
                for i in ((2 * t) % NB, (2 * t + 1) % NB):
                    want, keep, zero = S.oracle(kind, i, drop_zero)
                    assert_filtered_equal(f.download(i, S.stream), want, keep, zero, "%s scan %d" % (what, i))
                seen.append(Seen(kind, fused, xform, holes, scatter, routes, ms))
                t += 1
    finally:
        f.close()
    return seen


def device_forms(seen):
    return "".join("-" if not s.fused else ("X" if s.xform else ("H" if s.holes else "F")) + ("!" if wasted(s) else "") for s in seen)


def wasted(s):
    return bool(s.fused) and 4 * sum(1 for r in s.routes if r == 0) > len(s.routes)


def check_against_model(lib, seen, phases, hint, holes_possible, drop_zero):
    model = M.drive(lib, phases, hint=hint, holes_possible=holes_possible, drop_zero=drop_zero, batch=NB, rings=R)
    ctx = "%s, hint %s\ndevice %s\nmodel  %s" % (phases, hint, device_forms(seen), M.forms(model).replace("f", "F"))
    print(ctx)
    for t, (d, m) in enumerate(zip(seen, model)):
        assert (d.fused, d.xform, d.holes) == (m.fused, m.xform, m.holes), "batch %d: device %s, model %s\n%s" % (t, d[1:4], m[1:4], ctx)
        # (the one-launch tail stands in for the bucketing route's launches: no scatter launch exactly there)
        assert d.scatter == (0 if m.fused and m.short_tail and not m.xform else 1), "batch %d: scatter launches %d\n%s" % (t, d.scatter, ctx)
        code = 0 if not m.fused or m.fell else (2 if m.xform else (3 if m.holes else 1))
        assert d.routes == [code] * NB, "batch %d: routes %s, the model's form implies %d\n%s" % (t, d.routes, code, ctx)
    return model


def check_waste(seen, phases, ctx=""):
    at = 0
    for kind, n in phases:
        w = [t for t in range(at + M.SETTLE, at + n) if wasted(seen[t])]
        for a, b in zip(w, w[1:]):
            assert b - a >= M.RETRY_PERIOD, "%s: wasted batches %d and %d within 16 consecutive ones: %s" % (ctx, a, b, device_forms(seen))
        at += n


ALONE = [[(k, 24)] for k in M.KINDS + (M.SPARSE,)]
TRANSITIONS = [[(a, 20), (b, 20)] for a, b in (("turned_holes", "clean"), ("turned_holes", "turned"), ("turned_holes", "holes"),
                                               ("ragged", "turned_holes"), ("holes", "turned_holes"), ("turned", "turned_holes"))]


def _id(phases):
    return "-then-".join(k for k, _ in phases)


@pytest.mark.parametrize("phases", ALONE + TRANSITIONS, ids=[_id(p) for p in ALONE + TRANSITIONS])
def test_device_follows_the_model_batch_for_batch(streams, lib, phases):
    seen = run_on_device(streams, phases)
    if phases == [("turned_holes", 24)]:
        # (for the record, no assertion: what a batch of such a stream costs once the route has settled)
        last = [s.ms for s in seen[-16:]]
        print("turned_holes, %d x %d x %d: kernel time per batch over the last 16 batches: mean %.4f ms (min %.4f, max %.4f)" % (
            R, COLS, NB, sum(last) / 16, min(last), max(last)))
    check_against_model(lib, seen, phases, "unknown", True, True)
    check_waste(seen, phases, _id(phases))


def test_turned_rings_with_zero_records_leave_the_organised_route(streams, lib):
    """40 batches of rings turned AND holed, zero filter on: each form is tried once, then the bucketing route with one retry
    per 16 batches -- not ring_cut_kernel, the organised-scan kernel and a full fall-back in every batch."""
    for kind in ("turned_holes", M.SPARSE):
        phases = [(kind, 40)]
        seen = run_on_device(streams, phases)
        check_against_model(lib, seen, phases, "unknown", True, True)
        check_waste(seen, phases, kind)
        assert sum(wasted(s) for s in seen) <= 3 + -(-40 // M.RETRY_PERIOD), device_forms(seen)


def test_holes_hint_without_the_zero_filter(streams, lib):
    """stream_hint = GRID_WITH_HOLES on a context without the zero filter cannot be honoured (the holes form is the zero
    filter's): a ragged stream is bucketed within the bound, the organised kernel launched at most once per 16 batches from
    then on; a clean stream stays fused, and no count pass is ever launched."""
    phases = [("ragged", 40)]
    seen = run_on_device(streams, phases, hint="grid_with_holes", drop_zero=False)
    check_against_model(lib, seen, phases, "grid_with_holes", False, False)
    check_waste(seen, phases, "hinted ragged")
    assert not seen[M.SETTLE].fused or not seen[M.SETTLE + 1].fused, device_forms(seen)
    fused_at = [t for t in range(M.SETTLE, 40) if seen[t].fused]
    assert all(b - a >= M.RETRY_PERIOD for a, b in zip(fused_at, fused_at[1:])) and len(fused_at) <= 2, device_forms(seen)
    assert not any(s.holes for s in seen)
    phases = [("clean", 24)]
    seen = run_on_device(streams, phases, hint="grid_with_holes", drop_zero=False)
    check_against_model(lib, seen, phases, "grid_with_holes", False, False)
    assert all(s.fused and not s.holes and not s.xform and s.routes == [1] * NB for s in seen), device_forms(seen)
