"""The launch shape every production batch runs, with real scans: from 32 scans on, lfx_segment_batch and
lfx_scan_context_batch give a scan 8 workgroups instead of 32 (lfx_segment.hip, lfx_place.hip).  33 distinct scans of
16 x 900 (tests/segment_cases.py): 14 400 records against 8 x 256 threads are 8 steps of the kernels' stride loops, the last
of them over 64 records of the scan -- workgroup 0 walks one whole wave there and the other seven none, and the scans with 5 %
of their records dropped end in a partial wave, whose ballots count the classes of fewer than 64 lanes.  Class, id, counts and
descriptors equal the restatements byte for byte.  (A call takes the whole of the last batch, so the 32 and the 33 scans
are two extractions on one context.)"""
import numpy as np
import pytest

from tests import deskew_cases as K
from tests import scan_context_restatement as SC
from tests import segment_cases as S
from tests import segment_restatement as R

pytestmark = pytest.mark.gpu

GRIDS = [dict(), dict(n_rings=40, n_sectors=120)]


@pytest.fixture(scope="module")
def ctx():
    fx = S.fx33()
    yield fx
    fx.close()


def _extracted(fx, n):
    clouds = S.scans33()[:n]
    d = S.device_batch(fx, clouds)
    fx.batch_status(K.stream())
    K.sync()
    return d


@pytest.mark.parametrize("n", [32, 33])
def test_segmentation_and_descriptors_of_32_and_33_scans(ctx, n):
    """16 x 900 over the first 32 scans and over all 33, one chunk each: the 8-workgroup shape on its threshold and past it;
    the descriptors of the same batch for the default grid and for 40 x 120."""
    clouds = S.scans33()[:n]
    # (the whole scans: 8 steps; the thinned ones: 7, the last of them with a partial wave)
    assert min(len(c) for c in clouds) > 6 * 8 * 256 and any(len(c) % 64 for c in clouds) and any(len(c) == 14400 for c in clouds)
    d = _extracted(ctx, n)
    fields = dict(n_rows=S.RINGS, n_columns=S.COLS)
    got = S.numpy_of(ctx.segment(R.config(**fields), stream=K.stream()))
    S.same(got, S.segment_want(n, **fields), ("16 x 900", n))
    assert (got[2].sum(axis=1) == [len(c) for c in clouds]).all() and got[2][:, R.GROUND].min() > 500 and (got[2].sum(axis=0) > 0).all()
    for f in GRIDS:
        out = ctx.scan_context(SC.config(**f), None, K.stream())
        K.sync()
        S.same_floats(out.cpu().numpy(), S.descriptors_want(n, **f), ("descriptors", n, f))
    del d


def test_the_largest_image_over_33_scans_is_two_chunks(ctx):
    """128 x 4096 over all 33 scans: 32 scans in the first chunk (8 workgroups a scan) and one in the second (32), with real
    records on both sides of first_scan."""
    from lidar_feature_extraction_amd import binding as B
    assert B.SEGMENT_BUDGET_CELLS // (128 * 4096) == 32
    d = _extracted(ctx, S.N_SCANS)
    fields = dict(n_rows=128, n_columns=4096)
    got = S.numpy_of(ctx.segment(R.config(**fields), stream=K.stream()))
    S.same(got, S.segment_want(S.N_SCANS, **fields), "128 x 4096")
    assert got[2][32].sum() == len(S.scans33()[32]) and got[2][32][R.SEGMENT] > 5000 and (got[2].sum(axis=0) > 0).all()
    del d
