"""Start-up relocalisation end to end on the device: the six keyframes and 24 revisits of the prototype
(tests/scan_context_restatement.py) through extract_batch_device -> scan_context -> PlaceDb, then each revisit localised
with localize_batch from the pose the index proposes."""
import numpy as np
import pytest

from tests import deskew_cases as K
from tests import scan_context_restatement as R

pytestmark = pytest.mark.gpu


def _rz(yaw, t=(0.0, 0.0, 0.0)):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0.0, t[0]], [s, c, 0.0, t[1]], [0.0, 0.0, 1.0, t[2]]], np.float64)


def test_revisits_are_recognised_and_localised_from_the_proposed_pose():
    """Every revisit names its keyframe with |yaw - truth| <= 2 pi / S (S = 60: the CPU oracle's localizer converges on every
    revisit from half a sector off, so no finer grid is needed), and the device's descriptors are the restatement's bits.
    Then each revisit is localised against maps made of its keyframe's own feature clouds, from Rz(yaw) with zero
    translation; the control starts from the true pose moved 0.2 m and turned 1 degree.  Per revisit the translation error
    is at most twice the largest control error of the 24.

    ON THE CPU ORACLE (the same clouds, the same starts): largest control error 0.122 m (bound 0.245 m), largest error from
    the proposed pose 0.160 m; every alignment ends with a success code.  A 16 x 900 scan against one keyframe's features
    is a coarse localisation; the bound is about the start, not about that."""
    from lidar_feature_extraction_amd import concat
    cfg = R.config()
    S = int(cfg.n_sectors)
    keys, revisits = R.keyframes(), R.revisits()
    fx = K.fx_for(R.RINGS, R.COLS, 8)
    d, got = K.extract(fx, keys)
    fx.batch_status(K.stream())
    desc = fx.scan_context(cfg, None, K.stream())
    db = fx.place_db(16, cfg)
    db.add(desc, len(keys), K.stream())
    assert len(db) == len(keys)
    assert db.download(stream=K.stream()).tobytes() == np.stack([R.descriptor_of_cloud(cfg, c) for c in keys]).tobytes()
    maps = [(fx.make_map_from_host(g.edge_points, 1.0, K.stream()), fx.make_map_from_host(g.surface_points, 1.0, K.stream())) for g in got]
    reloc, control = [], []
    for place in range(len(keys)):
        visits = [v for v in revisits if v[1] == place]
        clouds = [v[0] for v in visits]
        d2 = K.upload_bytes(concat(clouds))
        fx.extract_batch_device(d2.data_ptr(), [len(c) for c in clouds], K.stream())
        q = fx.scan_context(cfg, None, K.stream())
        matches = db.query(q, len(clouds), 2, stream=K.stream())
        starts, nudged, truth = [], [], []
        for (cloud, _place, yaw), m in zip(visits, matches):
            print("revisit of %d turned %.0f deg: entry %s shift %d distance %.3f yaw %.1f deg; runner-up %s at %.3f" % (
                place, np.rad2deg(yaw), m[0]["entry"], m[0]["shift"], m[0]["distance"], np.rad2deg(m[0]["yaw"]), m[1]["entry"], m[1]["distance"]))
            assert m[0]["entry"] == place, (place, yaw, m)
            assert R.yaw_error(m[0]["yaw"], yaw) <= 2.0 * np.pi / S, (place, yaw, m[0])
            starts.append(_rz(m[0]["yaw"]))
            truth.append(_rz(yaw, (R.REVISIT_OFFSET[0], R.REVISIT_OFFSET[1], 0.0)))
            nudged.append(_rz(yaw + np.deg2rad(1.0), (R.REVISIT_OFFSET[0] + 0.12, R.REVISIT_OFFSET[1] - 0.16, 0.0)))
        emap, smap = maps[place]
        for poses, errors in ((nudged, control), (starts, reloc)):
            res = fx.localize_batch(emap, smap, np.stack(poses), 15, 20, 1.0, K.stream())
            errors.extend(float(np.linalg.norm(r["pose"][:, 3] - t[:, 3])) for r, t in zip(res, truth))
        del d2
    control, reloc = np.array(control), np.array(reloc)
    for i, (c, r) in enumerate(zip(control, reloc)):
        print("revisit %2d: control %.4f m, from the proposed pose %.4f m" % (i, c, r))
    print("relocalise: largest control error %.4f m, largest error from the proposed pose %.4f m" % (control.max(), reloc.max()))
    assert control.max() < 0.3, control             # (the control converges on every revisit)
    assert (reloc <= 2.0 * control.max()).all(), (reloc, control)
    for e, s in maps:
        e.close()
        s.close()
    db.close()
    del d
    fx.close()
