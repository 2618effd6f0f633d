"""What scan context, segmentation and the visibility votes share on the host (CPU): the three *_tables functions give the
same cos / sin arrays byte for byte for the same number of columns (one azimuth table, lfx_pose.cpp), and the five *_config
functions stand on one body -- each refuses an unknown field with its own TypeError and takes None, a dict, keywords and a
struct of its own type, which it copies."""
import numpy as np
import pytest

import lidar_feature_extraction_amd as lfx
from lidar_feature_extraction_amd import binding as B
from lidar_feature_extraction_amd import extraction as X

# (function, its struct, the name its TypeError gives the settings, an integer field and a value that is not its default)
CONFIGS = [
    (X.scan_context_config, B.ScanContextConfig, "scan-context", "n_sectors", 48),
    (X.segment_config, B.SegmentConfig, "segmentation", "n_columns", 900),
    (X.visibility_config, B.VisibilityConfig, "visibility", "n_columns", 720),
    (X.pose_graph_config, B.PoseGraphConfig, "pose-graph", "max_nodes", 77),
    (X.loop_closer_config, B.LoopCloserConfig, "loop-closer", "n_candidates", 5),
]
IDS = [c[2] for c in CONFIGS]


@pytest.mark.parametrize("W", [4, 60, 120])
def test_the_three_tables_share_their_cos_and_sin(W):
    # 120 is scan context's most sectors; rows and rings small, the rest the defaults
    sc = X.scan_context_tables(dict(n_sectors=W, n_rings=2))
    seg = X.segment_tables(dict(n_columns=W, n_rows=2, ground_first_row=0, ground_last_row=1))
    vis = X.visibility_tables(dict(n_columns=W, n_rows=2))
    for got in (sc, seg, vis):
        assert got[0].dtype == np.float64 and got[0].shape == (W,) and got[1].shape == (W,)
    for other in (seg, vis):
        assert other[0].tobytes() == sc[0].tobytes()
        assert other[1].tobytes() == sc[1].tobytes()
    # (and not an array of zeros: direction 0 is -pi, and the y < 0 half comes first)
    assert sc[0][0] == -1.0 and np.all(sc[1][1:W // 2] < 0.0) and np.all(sc[1][W // 2 + 1:] > 0.0)


@pytest.mark.parametrize("make,struct,what,field,value", CONFIGS, ids=IDS)
def test_a_config_refuses_an_unknown_field(make, struct, what, field, value):
    for call in (lambda: make(no_such_field=1), lambda: make({"no_such_field": 1}), lambda: make(struct(), no_such_field=1)):
        with pytest.raises(TypeError) as e:
            call()
        assert str(e.value) == "unknown %s setting 'no_such_field'" % what


@pytest.mark.parametrize("make,struct,what,field,value", CONFIGS, ids=IDS)
def test_a_config_takes_none_a_dict_keywords_and_its_struct(make, struct, what, field, value):
    default = make()
    assert isinstance(default, struct) and bytes(default) == bytes(make(None))
    assert getattr(default, field) != value
    by_dict, by_keyword = make({field: value}), make(**{field: value})
    assert isinstance(by_dict, struct) and getattr(by_dict, field) == value
    assert bytes(by_dict) == bytes(by_keyword)
    # (a keyword wins over the dict's entry)
    assert bytes(make({field: getattr(default, field)}, **{field: value})) == bytes(by_dict)
    # a struct is copied, not aliased, and keeps what it holds where no field replaces it
    copy = make(by_dict)
    assert copy is not by_dict and bytes(copy) == bytes(by_dict)
    setattr(copy, field, getattr(default, field))
    assert getattr(by_dict, field) == value and bytes(copy) == bytes(default)
    changed = make(by_dict, **{field: getattr(default, field)})
    assert bytes(changed) == bytes(default) and getattr(by_dict, field) == value


def test_the_loop_closer_config_keeps_its_submap_capacity_forms():
    default = lfx.loop_closer_config()
    one, two = lfx.loop_closer_config(submap_capacity=1234), lfx.loop_closer_config({"submap_capacity": (1234, 99)})
    assert tuple(one.submap_capacity) == (1234, 1234) and tuple(two.submap_capacity) == (1234, 99)
    again = lfx.loop_closer_config(two, n_candidates=int(default.n_candidates))
    assert tuple(again.submap_capacity) == (1234, 99) and tuple(two.submap_capacity) == (1234, 99)
