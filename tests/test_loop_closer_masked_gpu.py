"""A loop closer that verifies against clean submaps (lfx_loop_closer_set_masked, include/lfx.h) over the drive of
tests/loop_closer_cases.py: the masked verification against the hand composition of the public calls it is defined as, byte
for byte; the point of it -- a store with flagged ghost records verifies exactly as the store without them; and the refusal
on a store without flags."""
import numpy as np
import pytest

from tests import deskew_cases as K
from tests import loop_closer_cases as LC
from tests.test_loop_closer_gpu import CAPACITY, SCAN, Drive, _same

pytestmark = pytest.mark.gpu


class _Masked:
    """the drive's store with submap() answered by submap_masked(): what Drive.compose composes a masked verification from"""

    def __init__(self, kf):
        self._kf = kf

    def __getattr__(self, name):
        return getattr(self._kf, name)

    def submap(self, *args, **kw):
        return self._kf.submap_masked(*args, **kw)


@pytest.fixture(scope="module")
def drive():
    d = Drive()
    yield d
    d.close()


def _fields(**config):
    return dict(dict(min_gap=LC.MIN_GAP, search_radius=LC.SEARCH_RADIUS, max_distance=LC.MAX_DISTANCE, n_candidates=LC.N_CANDIDATES,
                     submap_capacity=CAPACITY, **LC.SUBMAP), **config)


def test_set_masked_on_a_store_without_flags_is_refused(drive):
    """(first in the file: the module's store has no flags yet)"""
    from lidar_feature_extraction_amd import binding as B
    lc = drive.closer()
    got, _ = lc.detect(6, 6, K.stream())
    before = lc.verify(8, got[2][0], K.stream())["raw"]
    assert lc.masked is False
    with pytest.raises(B.LfxError) as err:
        lc.set_masked(True)
    assert err.value.code == B.ERR_INVALID_ARGUMENT
    assert lc.masked is False and lc.verify(8, got[2][0], K.stream())["raw"] == before
    lc.set_masked(False)                                                # (0 needs no flags)
    assert lc.masked is False
    assert drive.fx._L.lfx_loop_closer_set_masked(None, 0) == B.ERR_INVALID_ARGUMENT
    assert drive.fx._L.lfx_loop_closer_get_masked(lc.handle, None) == B.ERR_INVALID_ARGUMENT


def test_masked_verify_equals_the_hand_composition(drive):
    """Node 6 against 0 (a submap of one keyframe) and node 8 against 2 (two), 30 % of every keyframe's records flagged: the
    closure is submap_masked -> lfx_map_create -> downsample -> align_report composed by hand.  Switched off again, the
    closer's bytes are a plain closer's."""
    import torch
    d = drive
    plain = d.closer()
    got, _ = plain.detect(6, 6, K.stream())
    want_plain = {q: plain.verify(q, got[q - 6][0], K.stream()) for q in (6, 8)}
    d.kf.reserve_flags(K.stream())
    n = d.kf.info()["n_points"]
    gen = torch.Generator(device="cpu").manual_seed(91)
    for kind in (0, 1):
        drawn = (torch.rand(n[kind], generator=gen) < 0.3).to(torch.uint8).to(K.dev())
        d.kf.set_flags(kind, drawn, 0, len(d.kf), K.stream())
    K.sync()
    flagged = d.kf.flags_info(K.stream())["n_flagged"]
    assert 0.2 * n[0] < flagged[0] < 0.4 * n[0] and 0.2 * n[1] < flagged[1] < 0.4 * n[1]
    lc = d.closer()
    lc.set_masked(True)
    assert lc.masked is True and plain.masked is False
    before = d.state()
    store = d.kf
    for q in (6, 8):
        cand = got[q - 6][0]
        d.kf = _Masked(store)
        try:
            hand = d.compose(q, cand)
        finally:
            d.kf = store
        closure = lc.verify(q, cand, K.stream())
        _same(closure, hand, q, cand["entry"])
        for kind in (0, 1):
            assert 0 < closure["submap"][kind]["n_points"] < want_plain[q]["submap"][kind]["n_points"]
            assert closure["submap"][kind]["n_written_keyframes"] == want_plain[q]["submap"][kind]["n_written_keyframes"]
        # the plain closer over the same store does not see the flags
        assert plain.verify(q, cand, K.stream())["raw"] == want_plain[q]["raw"]
    assert d.state() == before
    lc.set_masked(False)
    for q in (6, 8):
        assert lc.verify(q, got[q - 6][0], K.stream())["raw"] == want_plain[q]["raw"]
    d.kf.clear_flags(0, 0, len(d.kf), K.stream())
    d.kf.clear_flags(1, 0, len(d.kf), K.stream())
    K.sync()


def test_a_masked_closer_over_flagged_ghosts_is_the_plain_closer_without_them(drive):
    """Store A: the drive's clouds.  Store B: the same clouds with a block of ghost records inserted into every keyframe of
    the candidate's neighbourhood (node 8 against 2: keyframes 0, 1, 2), and exactly those flagged; the query keyframe gets
    none.  The kept records are the same bytes in the same order, so the masked closer on B is the plain closer on A."""
    d = drive
    rng = np.random.default_rng(93)
    q, c = 8, 2
    ghosts = 400
    kfa = d.fx.keyframes(16, LC.N * SCAN)
    kfb = d.fx.keyframes(16, LC.N * SCAN + 3 * ghosts)
    kfb.reserve_flags(K.stream())
    flags = [[], []]
    for k in range(LC.N):
        clouds = [np.ascontiguousarray(d.got[k].edge_points, np.float32).reshape(-1, 4), np.ascontiguousarray(d.got[k].surface_points, np.float32).reshape(-1, 4)]
        assert kfa.add_host(clouds[0], clouds[1], d.chained[k], K.stream()) == k
        with_ghosts = []
        for kind in (0, 1):
            f = np.zeros(len(clouds[kind]), np.uint8)
            if k <= c:
                # a car-sized box of records beside the sensor, put in the middle of the cloud
                ghost = np.hstack([rng.uniform([3.0, -1.0, -1.5], [7.0, 1.0, 0.0], (ghosts, 3)), np.ones((ghosts, 1))]).astype(np.float32)
                at = len(clouds[kind]) // 2 + 7 * k
                clouds[kind] = np.concatenate([clouds[kind][:at], ghost, clouds[kind][at:]])
                f = np.concatenate([f[:at], np.full(ghosts, 1 + k, np.uint8), f[at:]])
            with_ghosts.append(clouds[kind])
            flags[kind].append(f)
        assert kfb.add_host(with_ghosts[0], with_ghosts[1], d.chained[k], K.stream()) == k
    import torch
    for kind in (0, 1):
        f = np.concatenate(flags[kind])
        assert int((f != 0).sum()) == 3 * ghosts
        kfb.set_flags(kind, torch.from_numpy(f).to(K.dev()), 0, LC.N, K.stream())
    K.sync()
    assert kfb.flags_info(K.stream())["n_flagged"] == (3 * ghosts, 3 * ghosts)
    closers = [d.fx.loop_closer(kf, d.db, d.graph, **_fields()) for kf in (kfa, kfb, kfb)]
    plain_a, masked_b, plain_b = closers
    masked_b.set_masked(True)
    cand = plain_a.detect(q, 1, K.stream())[0][0][0]
    assert cand["entry"] == c
    a, m, b = (lc.verify_raw(q, cand, K.stream()) for lc in closers)
    for field in ("result", "report", "edge"):
        assert bytes(getattr(m, field)) == bytes(getattr(a, field)), field
    assert (m.accepted, m.reason, m.query, m.candidate) == (a.accepted, a.reason, q, c) and bytes(m.match) == bytes(a.match)
    for kind in (0, 1):
        assert bytes(m.submap[kind]) == bytes(a.submap[kind]) and a.submap[kind].n_points > 0
        assert b.submap[kind].n_points == a.submap[kind].n_points + int(a.submap[kind].n_written_keyframes) * ghosts
    assert a.submap[0].n_written_keyframes == 2
    # ... and the drive's own store, filled in one add from the device batch, verifies as A does
    assert bytes(d.closer().verify_raw(q, cand, K.stream())) == bytes(a)
    for x in closers:
        x.close()
    kfa.close()
    kfb.close()
