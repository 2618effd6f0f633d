"""A model of what a stream of batches reports, and a driver that runs the route selection (lfx_route_choice = choose_route of
lfx_api.hip) over it in closed loop.  No tests in this file: tests/test_route_streams.py holds the machine to conditions over
every stream the model can make, tests/test_route_streams_gpu.py holds this model to the kernels batch for batch.

A stream is a list of (kind, n_batches) phases.  Every scan of a batch is of the batch's kind (rings x columns, 16 x 600 in the
device test):
  clean                 a grid in angle order
  turned                every ring a rotation of its angle order (make_scan(start_col=...))
  holes                 a grid with (0, 0, 0) records, so many that every unit of the organised-scan kernel meets one
  turned_holes          both
  turned_holes_sparse   both, the zero records so few that some unit holding a ring's wrap meets none
  ragged                records dropped at random: the scan is no rings x columns grid (its length is no multiple of the ring count)
  shuffled              rings x columns records in random order
The rules below give the counters block such a batch leaves (lfx_kernels_common.hpp:135-136) for the form it was run in; each
names the line of the kernel it was read from."""
import collections
import ctypes as C

from lidar_feature_extraction_amd import binding as LB

# the words of the report (lfx_kernels_common.hpp:135-136)
DEFER, REDO, SLOW, PREFIXED, FALLBACK, FUSED_RAN, BATCH, ORDER_FELL, TURNED, CUT_RAN, ZERO_FELL, HOLES_RAN, ZERO_GROUPS = range(13)
REPORT_WORDS, STATE_WORDS, CHOICE_WORDS = 14, 5, 7          # LFX_ROUTE_*_WORDS (include/lfx.h)

RETRY_PERIOD = 16            # batches between two tries of the organised route on a stream that falls back (choose_route, retry_in)
SETTLE = RETRY_PERIOD + 4    # batches after a change of kind within which the loop must be in the kind's steady pattern

KINDS = ("clean", "turned", "holes", "turned_holes", "ragged", "shuffled")
SPARSE = "turned_holes_sparse"
HINTS = ("unknown", "turned_rings", "no_grid", "grid_with_holes")      # LFX_STREAM_* in this order (binding.STREAM_*)

# organised_possible of lfx_route_choice: bit 0 the organised-scan kernel can run, bit 1 the context CANNOT run the holes form
# (no zero filter, or rings longer than the count pass takes: run_batch)
ORGANISED, NO_HOLES_FORM = 1, 2


def _has_zeros(kind):
    return kind in ("holes", "turned_holes", SPARSE)


def _is_turned(kind):
    return kind in ("turned", "turned_holes", SPARSE)


def effective_kind(kind, drop_zero):
    """Without the zero filter a (0, 0, 0) record is a point like any other to the route selection (unit_body tests for it
    only where og.drop_zero is set, lfx_kernels_unit.hpp:1187): the stream models as the same one without holes."""
    if drop_zero or not _has_zeros(kind):
        return kind
    return "turned" if _is_turned(kind) else "clean"


def report_of(kind, fused, xform, holes, batch, rings):
    """The 14 counter words a batch of `batch` scans of `kind` leaves when run in the form (fused, xform, holes) -- `holes` as
    run_batch launches it, i.e. only where the context can (zero filter on throughout; see effective_kind)."""
    rep = [0] * REPORT_WORDS
    groups = (rings + 3) // 4
    rep[BATCH] = batch                                  # feature_compact_kernel writes the host's own two words (lfx_kernels_extract.hpp:2239)
    rep[FUSED_RAN] = 1 if fused else 0
    if not fused:
        rep[FALLBACK] = batch                           # batch_reset_kernel puts every scan on the list (lfx_kernels_extract.hpp:30)
        return rep
    assert not (xform and holes), "the holes form takes rings as they stand (choose_route)"
    if xform:
        rep[CUT_RAN] = 1                                # ring_cut_kernel, scan 0, whatever the scans are (lfx_kernels_extract.hpp:1407)
        if _is_turned(kind) or kind == "shuffled":
            # a ring whose transform is not the identity counts once (lfx_kernels_extract.hpp:1476-1491); a shuffled ring has no
            # wrap, the search ends at some column -- hardly ever column 0.  (Zero records leave the count of a stream that is
            # NOT turned at 0 but for a scan whose very first record is one: ring 0's search starts there, :1436.)
            rep[TURNED] = batch * rings
        # ragged: C * max_rings != n, the kernel leaves such a scan alone (lfx_kernels_extract.hpp:1410)
    if holes:
        rep[HOLES_RAN] = 1                              # the count pass, scan 0 (lfx_kernels_extract.hpp:1138, 1270)
    if kind == "clean":
        return rep
    if kind == "ragged":
        # the host left columns = 0 in the scan's geometry: one unit puts it on the list without a reason
        # (lfx_kernels_unit.hpp:1089-1090); holes form: the count pass does, before it counts anything (lfx_kernels_extract.hpp:1139-1141)
        rep[FALLBACK] = batch
        return rep
    if kind == "shuffled":
        # records that do not carry the ring id of their place: no reason given (lfx_kernels_unit.hpp:1186, 1204); holes form: the
        # count pass finds them and leaves before the zero groups are counted (lfx_kernels_extract.hpp:1175-1179)
        rep[FALLBACK] = batch
        return rep
    if holes:
        # the count pass takes any grid whose ring ids are right; a ring group that holds a zero record counts once per scan
        # (grid_count_kernel :1179; scan_count_kernel adds the scan's groups at once, :1318)
        if _has_zeros(kind):
            rep[ZERO_GROUPS] = batch * groups
        if _is_turned(kind):
            # ... the unit kernel then takes the rings as they stand and gives the scan up for their order (lfx_kernels_unit.hpp:1422)
            rep[FALLBACK] = batch
            rep[ORDER_FELL] = batch                     # once per scan (scan_falls_back, lfx_kernels_common.hpp:278)
        return rep
    # plain form, or the transforms form (which only changes the columns a unit loads, lfx_kernels_unit.hpp:1171)
    if _has_zeros(kind):
        # a unit that meets a zero record leaves for that reason before it looks at the order (lfx_kernels_unit.hpp:1199-1202)
        rep[FALLBACK] = batch
        rep[ZERO_FELL] = batch                          # once per scan (lfx_kernels_common.hpp:279)
        if _is_turned(kind) and not xform and kind == SPARSE:
            rep[ORDER_FELL] = batch                     # a unit on a ring's wrap that met no zero record (lfx_kernels_unit.hpp:1105, 1241)
        return rep
    if _is_turned(kind) and not xform:
        rep[FALLBACK] = batch
        rep[ORDER_FELL] = batch                         # (lfx_kernels_unit.hpp:1105, 1241)
    return rep


def initial_state(hint):
    """(use_xform, bucket_all, retry_in, pre_order, use_holes) as lfx_create leaves it for a stream hint -- whatever the context
    can run: a hint it cannot honour is the route selection's to drop."""
    if hint == "turned_rings":
        return (1, 0, 0, 0, 0)
    if hint == "no_grid":
        return (0, 1, RETRY_PERIOD, 0, 0)
    if hint == "grid_with_holes":
        return (0, 0, 0, 0, 1)
    assert hint == "unknown", hint
    return (0, 0, 0, 0, 0)


def load():
    L = LB.load()
    L.lfx_route_choice.restype = C.c_int
    L.lfx_route_choice.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32), C.c_int, C.c_uint32, C.c_uint32,
                                   C.POINTER(C.c_uint32)]
    return L


# one batch of a run: what was chosen, what the batch then reported (None where it was not fused), the state after the choice
Step = collections.namedtuple("Step", "kind fused xform holes short_tail fell state")


def drive(lib, phases, hint="unknown", holes_possible=True, drop_zero=True, batch=8, rings=16):
    """lfx_route_choice in closed loop over the phases [(kind, n_batches), ...]: every batch's report is the next choice's
    input, as with a caller that waits for each batch.  Returns a Step per batch."""
    assert drop_zero or not holes_possible
    state = (C.c_uint32 * STATE_WORDS)(*initial_state(hint))
    rep = (C.c_uint32 * REPORT_WORDS)()
    rep_rings = 0
    possible = ORGANISED | (0 if holes_possible else NO_HOLES_FORM)
    steps = []
    for kind, n in phases:
        eff = effective_kind(kind, drop_zero)
        for _ in range(n):
            ch = (C.c_uint32 * CHOICE_WORDS)()
            assert lib.lfx_route_choice(rep, rep_rings, state, possible, batch, rings, ch) == 0
            fused, xform, short_tail = int(ch[0]), int(ch[1]), int(ch[3])
            holes = int(ch[6]) if holes_possible else 0            # run_batch launches the form only where the context can
            words = report_of(eff, fused, xform, holes, batch, rings)
            rep = (C.c_uint32 * REPORT_WORDS)(*words)
            rep_rings = batch * rings
            steps.append(Step(kind, fused, xform, holes, short_tail, words[FALLBACK] if fused else None, tuple(state)))
    return steps


def steady_form(kind, holes_possible=True, drop_zero=True):
    """The cheapest pattern the context can run on a stream of `kind`: (fused, xform, holes), or None = the bucketing route with
    one fused retry per RETRY_PERIOD batches."""
    eff = effective_kind(kind, drop_zero)
    if eff == "clean":
        return (1, 0, 0)
    if eff == "turned":
        return (1, 1, 0)
    if eff == "holes" and holes_possible:
        return (1, 0, 1)
    return None


def wasted(step, batch=8):
    """A batch that ran the organised-scan kernel for more than a quarter of its scans to fall back."""
    return bool(step.fused) and 4 * step.fell > batch


def forms(steps):
    return "".join("-" if not s.fused else ("X" if s.xform else ("H" if s.holes else ("f" if s.short_tail else "F"))) + ("!" if wasted(s) else "")
                   for s in steps)
