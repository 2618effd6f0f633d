"""The ring of table slots lfx_deskew_batch and lfx_deskew_batch_trajectory share (lfx_deskew.hip): a slot changes owner
between the two calls and grows while it holds an older, smaller table, and every call still computes what it computes alone."""
import numpy as np
import pytest

from tests import deskew_cases as K
from tests import deskew_restatement as R
from tests import trajectory_cases as TC

RINGS, COLS, N = 16, 900, 4
SLOTS = 8                                    # lfx_ctx::kDeskewSlots
# The calls in their order.  ci / cf: lfx_deskew_batch on all 4 scans, index times / a FLOAT32 field; t2, t64, t3:
# lfx_deskew_batch_trajectory on all 4 scans with so many knots; od / ot: the predicting and the trajectory odometry call over
# the batch, which de-skew scan by scan: four slots each, taken with n = 1.
PLAN = ["ci", "t3", "cf", "t2", "od", "t64", "ci", "t3", "cf", "t64", "t2", "ot", "t64", "t3", "cf", "t2", "ci", "t64", "t3", "t2", "cf", "ci"]
KNOTS = {"t2": 2, "t64": 64, "t3": 3}
OT_KNOTS = (2, 5, 11, 21)


def _slots_of_the_plan():
    """Per slot the (kind, doubles) of the tables it is handed, in order: n rows of 24 doubles for a constant motion, the
    segments' rows and n + 1 words for trajectories."""
    slots, at = [[] for _ in range(SLOTS)], 0
    for op in PLAN:
        if op == "od":
            tables = [("constant", 24)] * N
        elif op == "ot":
            tables = [("trajectory", 24 * (k - 1) + 1) for k in OT_KNOTS]
        elif op in KNOTS:
            tables = [("trajectory", 24 * N * (KNOTS[op] - 1) + (N + 2) // 2)]
        else:
            tables = [("constant", 24 * N)]
        for t in tables:
            slots[at % SLOTS].append(t)
            at += 1
    return slots


def test_the_plan_makes_every_slot_change_owner_and_grow():
    """(no device) What the test below relies on: every slot serves both kinds of call, and at least once is handed a table
    larger than the room it has (half again what it was last grown for) straight after a table of the other kind."""
    for tables in _slots_of_the_plan():
        assert {k for k, _ in tables} == {"constant", "trajectory"}, tables
        room, grew, last = 0, False, None
        for kind, doubles in tables:
            if doubles > room:
                grew = grew or (room > 0 and kind != last)
                room = doubles + doubles // 2
            last = kind
        assert grew, tables


def _arguments(rng):
    """Every call's own arguments, none like another's: a stale table would show."""
    args = []
    for op in PLAN:
        if op == "ci":
            args.append([R.pose(TC.unit(rng) * rng.uniform(0.0, 0.3), rng.uniform(-2, 2, 3)) for _ in range(N)])
        elif op == "cf":
            args.append([(10.0, 10.1, R.pose(TC.unit(rng) * (rng.uniform(0.0, 0.3) if s % 2 else 1e-10), rng.uniform(-2, 2, 3))) for s in range(N)])
        elif op in KNOTS:
            args.append([TC.seeded(rng, KNOTS[op], small=op == "t3" and s == 1) + (rng.uniform(0.0, 1.0),) for s in range(N)])
        elif op == "od":
            args.append(rng.uniform(0.5, 1.0))
        else:
            legs = [TC.turning(R.IDENTITY, knots=k, speed=rng.uniform(1.0, 3.0), yaw_deg=11.0) for k in OT_KNOTS]
            args.append([(t, p, t[-1]) for t, p in legs])
    return args


def _context(clouds, raw):
    """A context with the batch extracted and the FLOAT32 times at byte 24 of its input records."""
    import torch
    fx = K.fx_for(RINGS, COLS, N)
    d, got = K.extract(fx, clouds)
    d.view(-1, 32)[:, 24:28] = torch.from_numpy(raw).to(K.dev())
    K.sync()
    return fx, d, got


def _call(fx, op, arg, out, stream):
    """One call of the plan, queued, into `out` (zeroed and waited for: the call may run on another stream); what holds its
    outputs."""
    from lidar_feature_extraction_amd import binding as B
    if op in ("od", "ot"):
        odo = fx.odometry()
        res = odo.update_batch_deskewed(None, None, arg, "end", N, stream) if op == "od" else odo.update_batch_trajectory(None, arg, N, stream)
        return odo, res
    dst = (out[0].data_ptr(), out[1].data_ptr())
    if op == "ci":
        fx.deskew(None, arg, "end", dst, stream)
    elif op == "cf":
        fx.deskew(B.TimeField(B.TIME_FROM_FIELD, 24, B.FLOAT32, 0, 1.0), arg, "start", dst, stream)
    else:
        fx.deskew_trajectory(None, arg, dst, stream)
    return out, None


def _bytes(op, held, res):
    """A call's outputs on the host: both clouds whole; for an odometry call every scan's result and the store, which holds
    the de-skewed clouds at their poses."""
    K.sync()
    if op in ("od", "ot"):
        _, edge, surface = TC.store(held)
        return edge.tobytes(), surface.tobytes(), res
    return held[0].cpu().numpy().tobytes(), held[1].cpu().numpy().tobytes(), None


@pytest.mark.gpu
def test_every_call_of_an_interleaving_equals_the_call_alone():
    """22 out-of-place calls of PLAN on one context of 16 x 900 x 4, alternating between two streams; after one synchronise
    every call's two output clouds equal, byte for byte, what the same call gives as the only de-skew call on a fresh context
    over the same batch (an odometry call: its results and its store)."""
    import torch
    from lidar_feature_extraction_amd import make_sweep
    rng = np.random.default_rng(53)
    clouds = [make_sweep(RINGS, COLS, seed=9100 + s)[0] for s in range(N)]
    total = sum(len(c) for c in clouds)
    raw = rng.uniform(9.998, 10.102, total).astype("<f4").view(np.uint8).reshape(total, 4)
    args = _arguments(rng)
    fx, d, got = _context(clouds, raw)
    assert min(len(g.edge_points) + len(g.surface_points) for g in got) > 256          # (more than one workgroup per scan)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [K.out_buffers(total) for _ in PLAN]
    K.sync()
    queued = [_call(fx, op, arg, outs[i], streams[i % 2].cuda_stream) for i, (op, arg) in enumerate(zip(PLAN, args))]
    K.sync()
    together = [_bytes(op, held, res) for op, (held, res) in zip(PLAN, queued)]
    for op, (held, _) in zip(PLAN, queued):
        if op in ("od", "ot"):
            held.close()
    fx.close()
    out = K.out_buffers(total)
    for i, (op, arg) in enumerate(zip(PLAN, args)):
        alone_fx, alone_d, _ = _context(clouds, raw)
        for b in out:
            b.zero_()
        K.sync()
        held, res = _call(alone_fx, op, arg, out, K.stream())
        edge, surface, results = _bytes(op, held, res)
        assert edge == together[i][0] and surface == together[i][1], (i, op)
        assert any(edge) and any(surface), (i, op)
        if results is not None:
            assert all(TC.same_result(a, b) for a, b in zip(results, together[i][2])), (i, op)
            assert sum(r["aligned"] for r in results) == N - 1, (i, op)
            held.close()
        alone_fx.close()
