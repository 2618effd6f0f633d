"""The conditions the loop closer's GPU tests rest on (tests/loop_closer_cases.py: the drive), with the restatement and the
CPU oracle's localizer alone -- no GPU.

MEASURED (printed by the tests): the chained poses are 0.719 m off at node 11, the worst of nodes 6-11; with the oracle's
alignments as loop edges the restated optimiser leaves 0.189 m.  (A first jitter of (0.07, 0.05) m per step left node 11
0.620 m off, short of the 0.64 m asked for; (0.08, 0.06) m is the one kept.)  The gate leaves every revisit exactly one
eligible entry, its true place."""
import numpy as np

from tests import loop_closer_cases as LC
from tests import loop_closer_restatement as LR
from tests import odometry_restatement as OR
from tests import pose_graph_restatement as PG
from tests import scan_context_restatement as SC

# the information of the CPU expectation's loop edges: the oracle's localizer leaves 0.160 m on these revisits
# (tests/test_relocalize_gpu.py's docstring), and a sector of S = 60 is 0.105 rad, of which an alignment leaves a tenth
LOOP_SIGMA_ROT, LOOP_SIGMA_T = 0.01, 0.16

_MADE = {}


def _descriptors():
    if "desc" not in _MADE:
        cfg = SC.config()
        _MADE["desc"] = (cfg, np.stack([SC.descriptor_of_cloud(cfg, c) for c in LC.clouds()]))
    return _MADE["desc"]


def _candidates():
    """the best gated candidate of every node 6 .. 11 at the chained poses"""
    if "cand" not in _MADE:
        _cfg, desc = _descriptors()
        _MADE["cand"] = LR.detect(desc, LC.chain()[1], 6, 6, LC.MIN_GAP, LC.SEARCH_RADIUS, LC.MAX_DISTANCE, LC.N_CANDIDATES)
    return _MADE["cand"]


def _alignments():
    """The oracle's alignment of every revisit from pose_c x Rz(yaw) against maps of the submap's records."""
    if "align" not in _MADE:
        from oracle import binding as OB
        chained = LC.chain()[1]
        feats = [OB.extract(c, canonical_ties=True) for c in LC.clouds()]
        out = []
        for q, row in zip(range(6, 12), _candidates()[0]):
            c, _shift, _d, yaw = row[0]
            ids = LR.submap_ids(chained, c, q, LC.MIN_GAP, LC.SUBMAP["submap_half_window"], LC.SUBMAP["submap_radius"])
            emap = np.concatenate([OR.transform(chained[k], feats[k]["edge_points"]) for k in ids])
            smap = np.concatenate([OR.transform(chained[k], feats[k]["surface_points"]) for k in ids])
            res = OR.optimize_scan(emap, smap, 15, feats[q]["edge_points"], OR.downsample(feats[q]["surface_points"], 1.0),
                                   LR.initial_pose(chained[c], yaw), 20)
            out.append((q, c, ids, res))
        _MADE["align"] = out
    return _MADE["align"]


def test_the_chain_drifts_far_enough_and_not_too_far():
    """The drift at node 11 is at least 0.64 m, four times what the oracle's localizer leaves on these revisits; and every
    revisit's true place is still within search_radius of it at the chained poses."""
    chained, truth = LC.chain()[1], LC.truth()
    drift = float(np.linalg.norm(chained[11][:, 3] - truth[11][:, 3]))
    print("chained: node 11 is %.3f m off; the worst of nodes 6-11 %.3f m" % (drift, LC.worst_error(chained)))
    assert drift >= 0.64
    for q in range(6, 12):
        place = LC.true_place(q)[0]
        assert place in LR.eligible(LC.N, LR.limit_of(q, LC.MIN_GAP), q, chained, LC.SEARCH_RADIUS), q


def test_gate_hand_cases():
    for translations, radius, want in LC.GATE_CASES:
        poses = np.zeros((len(translations), 3, 4))
        poses[:, :, 3] = np.array(translations, np.float64)
        n = len(translations) - 1
        assert list(LR.eligible(n, n, n, poses, radius)) == want, (translations, radius)
    assert LR.limit_of(5, 6) == 0 and LR.limit_of(6, 6) == 1 and LR.limit_of(11, 6) == 6
    assert LR.window(0, 6, 6, 2) == (0, 1) and LR.window(3, 11, 6, 2) == (1, 5) and LR.window(5, 11, 6, 2) == (3, 3)


def test_the_best_gated_candidate_is_the_true_place():
    cfg, _desc = _descriptors()
    rows, n_eligible = _candidates()
    for q, row, n in zip(range(6, 12), rows, n_eligible):
        place, yaw = LC.true_place(q)
        print("node %d: %d eligible; best entry %d, distance %.3f, yaw %.1f deg (true %.1f)" % (q, n, row[0][0], row[0][2], np.rad2deg(row[0][3]),
                                                                                                 np.rad2deg(yaw)))
        assert row[0][0] == place, (q, row)
        assert SC.yaw_error(row[0][3], yaw) <= 2.0 * np.pi / int(cfg.n_sectors), (q, row[0])


def test_the_oracle_aligns_every_revisit_from_the_proposed_pose():
    for q, c, ids, res in _alignments():
        print("node %d against %d (submap %s): code %d after %d iterations" % (q, c, ids, res["code"], res["iteration"]))
        assert res["success"], (q, res)


def test_the_restated_edges_pull_the_revisits_back():
    """The restated edges through pose_graph_restatement leave the worst position error of nodes 6-11 below the chained one."""
    edges, chained = LC.chain()
    info = np.diag([1.0 / LOOP_SIGMA_ROT ** 2] * 3 + [1.0 / LOOP_SIGMA_T ** 2] * 3)
    graph = [dict(i=i, j=j, z=z, information=om, flags=0) for i, j, z, om in edges]
    for q, c, _ids, res in _alignments():
        _i, _j, z, _om = LR.edge(c, q, chained[c], res["pose"], np.eye(6), 1.0, False)
        graph.append(dict(i=c, j=q, z=z.reshape(3, 4), information=info, flags=PG.ROBUST))
    poses, res, _ = PG.optimize(chained, graph)
    assert res["code"] in (PG.CONVERGED, PG.MAX_ITERATIONS), res
    before, after = LC.worst_error(chained), LC.worst_error(poses)
    print("worst position error of nodes 6-11: chained %.3f m, optimised %.3f m" % (before, after))
    assert after < before
