"""CPU: the cases of tests/graph_structure_cases.py (the pose graph at its structural limits) against the model's stored results
(tests/golden/graph_structure_model_v1.npz, written by tests/golden/make_graph_structure_golden.py).  No GPU, no reference.

Every case must meet the three conditions of graph_structure_cases: the model's two step solvers agree on the trace, at least two
steps are accepted, some free pose moves by at least 1 cm.  The cases up to 300 nodes are solved again here, both variants, and held
against the stored results at the bounds of tests/test_graph_model.py; for the larger ones the stored figures are checked."""
import os

import numpy as np
import pytest

from tests import graph_numpy as gn
from tests import graph_structure_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "graph_structure_model_v1.npz")
TERMINATION = ("empty", "gradient", "max_iterations", "min_radius", "invalid_steps", "parameter", "function")
SMALL = tuple(c for c in sc.CASES if sc.n_nodes(c) <= sc.DENSE_LIMIT)
LIVE_X = ("n4097", "cg2050")               # solutions the golden file has no room for


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(PATH))


@pytest.mark.parametrize("name", SMALL)
def test_dense_and_sparse_agree_and_match_the_golden_file(name, golden):
    prob = sc.make_case(name)
    x, tr, same, d = sc.solve(name)
    assert same, "the two variants disagree on the trace"
    assert tr.successful_steps >= 2 and tr.accepted.count(1) >= 2
    assert sc.moved(prob, x) >= 0.01
    assert d <= 1e-6
    assert [TERMINATION.index(tr.termination), tr.iterations, tr.successful_steps] == golden["tr_" + name].tolist()
    assert tr.accepted == golden["acc_" + name].tolist()
    assert np.allclose([tr.initial_cost, tr.final_cost], golden["cost_" + name], rtol=1e-12, atol=0)
    assert np.allclose(tr.cost, golden["cand_" + name], rtol=1e-9, atol=0)
    assert gn.pose_distance(x, golden["x_" + name]) <= max(1e-12, 10 * float(golden["d_" + name]))
    fixed = prob["fixed"]
    assert np.array_equal(x[fixed], prob["poses"][fixed])


def test_golden_file_holds_every_case_within_the_conditions(golden):
    for name in sc.CASES:
        prob = sc.make_case(name)
        shape = [len(prob["poses"]), int((~prob["fixed"]).sum()), gn.n_long(prob)]
        assert golden["shape_" + name].tolist() == shape and tuple(shape[1:]) == sc.EXPECT[name], name
        term, its, ok = (int(v) for v in golden["tr_" + name])
        acc = golden["acc_" + name].tolist()
        assert len(acc) == its == len(golden["cand_" + name]) and acc.count(1) == ok >= 2, name
        assert float(golden["moved_" + name]) >= 0.01 and float(golden["d_" + name]) <= 1e-6, name
        assert golden["cost_" + name][1] < golden["cost_" + name][0], name
        # a final cost that is not rounding noise: the suite compares costs to 1e-9 relative
        assert golden["cost_" + name][1] > 1e-4, name
        if name in LIVE_X:
            assert "x_" + name not in golden
        else:
            assert golden["x_" + name].shape == prob["poses"].shape
            assert abs(sc.moved(prob, golden["x_" + name]) - float(golden["moved_" + name])) <= 1e-12
    assert os.path.getsize(PATH) < 1 << 20


def test_the_cases_sit_where_the_layout_changes():
    """The sizes are the ones at which the reduction's level list, the launched levels and the number of partial sums change."""
    assert [sc.global_levels(f) for f in (1, 1023, 1024, 1025, 2048, 2049, 4096, 4097)] == [0, 0, 0, 1, 1, 2, 2, 3]
    free = sorted({sc.EXPECT[c][0] for c in sc.CASES})
    for f in (1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097):
        assert f in free
    for c in sc.CG_LADDER:
        assert sc.EXPECT["cg%d" % c] == (c - 1, 2)
    # levels of exactly one block past a 64-lane and a 256-lane workgroup: 2 049 -> 1 025 = 16 x 64 + 1, 4 097 -> 2 049 = 8 x 256 + 1
    assert (2049 + 1) // 2 == 16 * 64 + 1 and (4097 + 1) // 2 == 8 * 256 + 1


def test_structure_cases_are_what_their_names_say():
    fr = lambda p: gn.free_index(p["fixed"])[0]
    p = sc.make_case("span")
    f = fr(p)
    assert np.nonzero(p["fixed"])[0].tolist() == [10, 11, 20] and f[12] - f[9] == 1 and f[21] - f[19] == 1 and gn.n_long(p) == 0
    assert (9, 12) in zip(p["ei"].tolist(), p["ej"].tolist()) and (19, 21) in zip(p["ei"].tolist(), p["ej"].tolist())
    assert (9, 12) in zip(p["fi"].tolist(), p["fj"].tolist())
    p = sc.make_case("ends")
    assert np.nonzero(p["fixed"])[0].tolist() == [0, 39]
    p = sc.make_case("runs")
    assert np.nonzero(p["fixed"])[0].tolist() == [0, 1, 2, 20, 21]
    assert (20, 21) in zip(p["ei"].tolist(), p["ej"].tolist()) and (21, 20) in zip(p["ei"].tolist(), p["ej"].tolist())
    assert (20, 21) in zip(p["fi"].tolist(), p["fj"].tolist())
    p = sc.make_case("reversed")
    back = p["ei"] > p["ej"]
    assert back.sum() == 14 and np.all(np.abs(p["ei"] - p["ej"]) == 1) and not p["fixed"].any()
    pairs = list(zip(p["ei"].tolist(), p["ej"].tolist()))
    assert (7, 8) in pairs and (8, 7) in pairs
    # a reversed edge measures the inverse: at the start poses (the odometry integrated) it has no residual either
    _, blk = gn.blocks(p, p["poses"], gn.Options, False)
    assert np.abs(blk[0][0][:39]).max() <= 1e-9
    a, b = sc.make_case("signs"), sc.make_case("signs_twin")
    assert np.array_equal(a["poses"][1::2, 3:], -b["poses"][1::2, 3:]) and np.array_equal(a["poses"][::2], b["poses"][::2])
    assert all(np.array_equal(a[k], b[k]) for k in a if k != "poses") and a["fixed"][0] and len(a["poses"]) == 37
    p = sc.make_case("all_but_one")
    assert np.nonzero(~p["fixed"])[0].tolist() == [17]
    a, b = sc.make_case("hub_across_fixed"), sc.make_case("hub_across_fixed_twin")
    assert (gn.n_long(a), gn.n_long(b)) == (1, 0) and not a["fixed"].any() and np.nonzero(b["fixed"])[0].tolist() == [15]
    assert fr(a)[16] - fr(a)[14] == 2 and fr(b)[16] - fr(b)[14] == 1
    assert all(np.array_equal(a[k], b[k]) for k in a if k != "fixed")


def test_the_model_does_not_see_the_sign_of_a_quaternion(golden):
    """`signs` hands every second pose over as -q.  In the model the iterations, costs and poses are those of its twin."""
    xa, ta, _, _ = sc.solve("signs")
    xb, tb, _, _ = sc.solve("signs_twin")
    assert (ta.termination, ta.iterations, ta.successful_steps, ta.accepted) == (tb.termination, tb.iterations, tb.successful_steps, tb.accepted)
    assert np.allclose(ta.cost, tb.cost, rtol=1e-12, atol=0)
    assert gn.pose_distance(xa, xb) <= max(1e-12, 10 * float(golden["d_signs"]))
