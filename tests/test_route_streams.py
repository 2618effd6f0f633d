"""The route selection over whole streams (no device): lfx_route_choice in closed loop with the report model of
tests/route_stream_model.py, over every kind of stream alone and every ordered pair of kinds -- the first run for 3, 10, 20 and
27 batches, so that the change falls at different points of a retry countdown -- unhinted, under each stream hint, and under
the holes hint on contexts that cannot run the holes form.  What is asserted are conditions on the loop, not sequences read off
the code under test:
  1  within SETTLE = retry period + 4 batches of a change of kind the loop is in that kind's steady pattern, and stays there;
  2  the steady pattern is the cheapest one the context can run (route_stream_model.steady_form);
  3  past that bound at most one batch in any 16 consecutive ones runs the organised-scan kernel for more than a quarter of its
     scans to fall back;
  4  past that bound on a clean stream no flag of the state is left set (retry_in is kept by the code).
The model itself is held to the kernels by tests/test_route_streams_gpu.py."""
import itertools

import pytest

from tests import route_stream_model as M

LENGTHS = (3, 10, 20, 27)
TAIL = M.SETTLE + 2 * M.RETRY_PERIOD + 5          # batches of the last phase: the bound, two retry periods, a few more
ALL_KINDS = M.KINDS + (M.SPARSE,)

# (hint, holes_possible, drop_zero, kinds): the last two starts are contexts that cannot run the holes form -- long rings with
# the zero filter on (scans with zero records fall back for them), and no zero filter at all (such records are points)
STARTS = [("unknown", True, True, ALL_KINDS)] + [(h, True, True, ALL_KINDS) for h in M.HINTS[1:]] + [
    ("grid_with_holes", False, True, ALL_KINDS),
    ("grid_with_holes", False, False, ("clean", "turned", "ragged", "shuffled")),
    ("unknown", False, True, ALL_KINDS),
]


@pytest.fixture(scope="module")
def lib():
    return M.load()


def check_phase(steps, first, last, kind, holes_possible, drop_zero, what):
    """Conditions 1 to 4 over steps[first:last], the batches of one phase of `kind`."""
    begin = first + M.SETTLE
    if begin >= last:
        return
    ctx = "%s: batches %d.. of '%s' (phase from %d): %s" % (what, begin, kind, first, M.forms(steps[first:last]))
    form = M.steady_form(kind, holes_possible, drop_zero)
    fused_at = [t for t in range(begin, last) if steps[t].fused]
    if form is not None:
        for t in range(begin, last):
            s = steps[t]
            assert (s.fused, s.xform, s.holes) == form and s.fell == 0, "%s\nbatch %d is %s, fell %s; steady form %s" % (ctx, t, s[1:4], s.fell, form)
            assert form != (1, 0, 0) or s.short_tail == 1, "%s\nbatch %d of a clean stream without the one-launch tail" % (ctx, t)
    else:
        # the bucketing route, the organised one retried once per period: never sooner, and never given up
        for a, b in zip(fused_at, fused_at[1:]):
            assert b - a == M.RETRY_PERIOD, "%s\nfused batches %d and %d" % (ctx, a, b)
        if last - begin >= M.RETRY_PERIOD:
            assert fused_at and fused_at[0] < begin + M.RETRY_PERIOD, "%s\nno retry within a period" % ctx
    waste_at = [t for t in range(begin, last) if M.wasted(steps[t])]
    for a, b in zip(waste_at, waste_at[1:]):
        assert b - a >= M.RETRY_PERIOD, "%s\nwasted batches %d and %d within 16 consecutive ones" % (ctx, a, b)
    if M.effective_kind(kind, drop_zero) == "clean":
        for t in range(begin, last):
            use_xform, bucket_all, _retry_in, pre_order, use_holes = steps[t].state
            assert (use_xform, bucket_all, pre_order, use_holes) == (0, 0, 0, 0), "%s\nstate %s after batch %d" % (ctx, steps[t].state, t)


def run_and_check(lib, phases, hint, holes_possible, drop_zero):
    steps = M.drive(lib, phases, hint=hint, holes_possible=holes_possible, drop_zero=drop_zero)
    what = "hint %s, holes form %s, zero filter %s, %s" % (hint, "possible" if holes_possible else "impossible", "on" if drop_zero else "off", phases)
    at = 0
    for kind, n in phases:
        check_phase(steps, at, at + n, kind, holes_possible, drop_zero, what)
        at += n
    return steps


@pytest.mark.parametrize("hint,holes_possible,drop_zero,kinds", STARTS, ids=["%s-%s-%s" % (s[0], "holes" if s[1] else "noholes", "filter" if s[2] else "nofilter") for s in STARTS])
def test_every_stream_settles_on_its_cheapest_route(lib, hint, holes_possible, drop_zero, kinds):
    for kind in kinds:
        run_and_check(lib, [(kind, TAIL)], hint, holes_possible, drop_zero)
    for a, b in itertools.permutations(kinds, 2):
        for n in LENGTHS:
            run_and_check(lib, [(a, n), (b, TAIL)], hint, holes_possible, drop_zero)


def test_turned_rings_with_zero_records_leave_the_organised_route(lib):
    """The first of the two streams the machine used to stay on for ever with every scan falling back (ring_cut_kernel, the
    organised-scan kernel and a full fall-back, each batch): rings turned AND zero records, zero filter on.  The transforms win
    over the holes form, so no report ever says the holes form ran -- and the excuse 'the holes form has not been tried yet'
    kept the stream off the bucketing route.  Whether the two reasons arrive in one report (few zero records) or in two."""
    for kind in ("turned_holes", M.SPARSE):
        for hint in M.HINTS:
            steps = run_and_check(lib, [(kind, 40)], hint, True, True)
            # (each of the three forms may be tried once before the stream is given up, then one retry per period)
            assert sum(M.wasted(s) for s in steps) <= 3 + -(-40 // M.RETRY_PERIOD), "%s, hint %s: %s" % (kind, hint, M.forms(steps))


def test_holes_hint_means_nothing_where_the_form_cannot_run(lib):
    """The second: stream_hint = GRID_WITH_HOLES on a context without the zero filter, or with long rings.  run_batch never
    launches the form there, so the state must not keep waiting for its report: a stream that falls back goes to the
    bucketing route as it does unhinted, and the state never holds the flag."""
    for drop_zero in (True, False):
        for kind in ("ragged", "shuffled"):
            hinted = run_and_check(lib, [(kind, 40)], "grid_with_holes", False, drop_zero)
            plain = run_and_check(lib, [(kind, 40)], "unknown", False, drop_zero)
            assert [s[1:5] for s in hinted] == [s[1:5] for s in plain], "%s\n%s" % (M.forms(hinted), M.forms(plain))
            assert not any(s.state[4] for s in hinted), [s.state for s in hinted]
    clean = run_and_check(lib, [("clean", 40)], "grid_with_holes", False, False)
    assert all(s.fused and not s.holes for s in clean), M.forms(clean)


def test_ways_out_of_turned_rings_with_zero_records(lib):
    """From the bucketing route a stream of turned rings with holes is left again: to a clean stream through one retry with
    the transforms (nothing turned), one batch of the holes form (no zero groups) and then the plain form; to a grid with holes
    through the retry (nothing turned) and then the holes form; to turned rings by the retry itself."""
    for n in LENGTHS:
        s = M.drive(lib, [("turned_holes", n + M.SETTLE), ("clean", TAIL)])
        at = n + M.SETTLE
        k = next(t for t in range(at, len(s)) if s[t].fused)
        assert [x[1:5] for x in s[k:k + 4]] == [(1, 1, 0, 0), (1, 0, 1, 1), (1, 0, 0, 1), (1, 0, 0, 1)], M.forms(s[at:])
        s = M.drive(lib, [("turned_holes", n + M.SETTLE), ("holes", TAIL)])
        k = next(t for t in range(at, len(s)) if s[t].fused)
        assert [x[1:4] for x in s[k:k + 3]] == [(1, 1, 0), (1, 0, 1), (1, 0, 1)] and s[k + 1].fell == 0, M.forms(s[at:])
        s = M.drive(lib, [("turned_holes", n + M.SETTLE), ("turned", TAIL)])
        k = next(t for t in range(at, len(s)) if s[t].fused)
        assert all(x[1:4] == (1, 1, 0) and x.fell == 0 for x in s[k:]), M.forms(s[at:])
