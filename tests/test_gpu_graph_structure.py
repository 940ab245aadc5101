"""GPU: the pose graph's solve (msfl_graph_*, docs/kernels/graph.md) at its structural limits, against the numpy model
(tests/graph_numpy.py) on the cases of tests/graph_structure_cases.py, whose model results are stored in
tests/golden/graph_structure_model_v1.npz (tests/golden/make_graph_structure_golden.py).

The bars are those of tests/test_gpu_graph.py, none is new: termination, iterations, successful steps and the accept list exact, costs
and candidate costs to 1e-9 relative, poses within max(1e-9, 10 x d_case) of the model, no unconverged step solve, fixed poses byte-equal
to the input.  `build`, `records` and `summary_tuple` are test_gpu_graph's own.  The figures are printed (run with -s).

    1. parity per case                         the whole solve
    2. one LM step per case                    max_num_iterations = 1: T^-1 b itself, which a full solve partly heals when it is off
    3. one object across a change of layout    1 024 -> 1 025 -> 1 024 -> 1 025 and 2 048 -> 2 049 free nodes, bytes against fresh graphs
    4. marginals on the new seams              F = 1 024 and 2 049 under CG, and `span`
    5. the sign of a quaternion                `signs` against its twin
"""
import functools
import os

import numpy as np
import pytest

from tests import graph_info_numpy as gi
from tests import graph_marginals_numpy as gm
from tests import graph_numpy as gn
from tests import graph_structure_cases as sc
from tests import test_gpu_graph as tg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERMINATION = ("empty", "gradient", "max_iterations", "min_radius", "invalid_steps", "parameter", "function")


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "graph_structure_model_v1.npz")))


@functools.lru_cache(maxsize=None)
def model_poses(name):
    """The model's solution: stored, or for the two cases the golden file has no room for solved here and held against the stored trace."""
    gold = golden()
    if "x_" + name in gold:
        return gold["x_" + name]
    x, tr = gn.solve_sparse(sc.make_case(name))
    assert [TERMINATION.index(tr.termination), tr.iterations, tr.successful_steps] == gold["tr_" + name].tolist()
    assert tr.accepted == gold["acc_" + name].tolist() and np.allclose(tr.cost, gold["cand_" + name], rtol=1e-12, atol=0)
    return x


def pose_bound(name):
    return max(1e-9, 10.0 * float(golden()["d_" + name]))


# ---- 1. parity per case --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.CASES)
def test_parity_with_the_model(name):
    gold, prob = golden(), sc.make_case(name)
    g = tg.build(prob)
    s = g.optimize()
    acc, cand = g.trace()
    x = g.poses()
    term, its, ok = (int(v) for v in gold["tr_" + name])
    dev = gn.pose_distance(x, model_poses(name))
    print("case %s: F %d global levels %d  termination %s iterations %d cg %d unconverged %d long %d  pose deviation %.3g (d_case %.3g)  cost %.12g -> %.12g" %
          (name, s.n_free, sc.global_levels(s.n_free), s.termination, s.iterations, s.cg_iterations, s.cg_unconverged, s.n_long_edges, dev,
           float(gold["d_" + name]), s.initial_cost, s.final_cost))
    assert (s.termination, s.iterations, s.successful_steps) == (term, its, ok)
    assert acc.tolist() == gold["acc_" + name].tolist()
    assert (s.n_free, s.n_long_edges) == sc.EXPECT[name] == (int((~prob["fixed"]).sum()), gn.n_long(prob))
    assert abs(s.initial_cost - gold["cost_" + name][0]) <= 1e-9 * gold["cost_" + name][0]
    assert abs(s.final_cost - gold["cost_" + name][1]) <= 1e-9 * gold["cost_" + name][1]
    assert np.allclose(cand, gold["cand_" + name], rtol=1e-9, atol=0)
    assert dev <= pose_bound(name)
    assert s.cg_unconverged == 0
    if s.n_long_edges == 0:
        assert s.cg_iterations == s.iterations          # the tridiagonal solve is the step
    fixed = np.nonzero(prob["fixed"])[0]
    assert np.array_equal(x[fixed], prob["poses"][fixed])


# ---- 2. one LM step ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.CASES)
def test_one_step_follows_the_model(name):
    """One iteration, then max_iterations: the poses are the start plus one step T^-1 b.  The model takes that step here (the sparse
    variant, an exact solve at any size); the bar on the poses is the case's."""
    prob = sc.make_case(name)
    xm, tm = gn.solve_sparse(prob, sc.OneStep)
    assert (tm.termination, tm.iterations, tm.accepted) == ("max_iterations", 1, [1])
    g = tg.build(prob, max_num_iterations=1)
    s = g.optimize()
    acc, cand = g.trace()
    x = g.poses()
    dev = gn.pose_distance(x, xm)
    print("case %s, one step: cg %d  pose deviation %.3g (d_case %.3g)  step %.3g" %
          (name, s.cg_iterations, dev, float(golden()["d_" + name]), sc.moved(prob, xm)))
    assert (TERMINATION[s.termination], s.iterations, s.successful_steps) == ("max_iterations", 1, 1) and acc.tolist() == [1]
    assert np.allclose(cand, tm.cost, rtol=1e-9, atol=0)
    assert abs(s.initial_cost - tm.initial_cost) <= 1e-9 * tm.initial_cost and abs(s.final_cost - tm.final_cost) <= 1e-9 * tm.final_cost
    assert sc.moved(prob, xm) >= 1e-3                    # a step to speak of
    assert dev <= pose_bound(name)
    assert s.cg_unconverged == 0
    fixed = np.nonzero(prob["fixed"])[0]
    assert np.array_equal(x[fixed], prob["poses"][fixed])


# ---- 3. one object across a change of the level layout ---------------------------------------------------------------------------

def _first_nodes(prob, n):
    """The sub-problem over nodes 0 .. n - 1: the factors whose two ends are among them, in their order."""
    out = {k: np.array(v) for k, v in prob.items()}
    out["poses"], out["fixed"] = out["poses"][:n], out["fixed"][:n]
    for keys in (("ei", "ej", "ez", "esr", "est"), ("fi", "fj", "ft", "fp", "fst")):
        keep = (prob[keys[0]] < n) & (prob[keys[1]] < n)
        for k in keys:
            out[k] = prob[k][keep]
    return out


def _state(g, s):
    return (tg.summary_tuple(s), g.poses().tobytes(), [t.tobytes() for t in g.trace()])


@pytest.mark.parametrize("n", (1025, 2049))
def test_one_object_across_a_change_of_layout(n):
    """A graph of n - 1 free nodes grows by one node (the reduction gains a launched level), then node 0 is fixed (it loses it again)
    and freed.  Before every optimize the poses are set back to the start, so that each one is a whole solve; after it the summary,
    the poses and the trace are the bytes a fresh graph of the same records gives.  A marginals call, which borrows the reduction's
    buffers, sits between two of the solves."""
    full = sc.make_case("n%d" % n)
    sub = _first_nodes(full, n - 1)
    assert len(sub["ei"]) == n - 2 and len(sub["fi"]) == len(full["fi"])
    levels = []
    g = tg.build(sub, max_nodes=n + 75, max_edges=n + 75, max_fixes=len(full["fi"]) + 1)

    def stage(prob):
        g.set_poses(prob["poses"])
        s = g.optimize()
        fresh = tg.build(prob)
        assert _state(g, s) == _state(fresh, fresh.optimize())
        assert s.iterations >= 3 and s.n_free == int((~prob["fixed"]).sum())
        levels.append(sc.global_levels(s.n_free))

    stage(sub)
    assert g.add_nodes(full["poses"][n - 1:]) == n - 1
    e, _ = tg.records(full)
    assert (e["i"][-1], e["j"][-1]) == (n - 2, n - 1)
    g.add_edges(e[-1:])
    stage(full)
    S, sm = g.marginals(gm.request(gi.with_info(full)))
    assert sm.n_columns > 0 and sm.singular == 0 and np.isfinite(S).all()
    anchored = {k: np.array(v) for k, v in full.items()}
    anchored["fixed"][0] = True
    g.set_fixed(0)
    stage(anchored)
    g.set_fixed(0, False)
    stage(full)
    assert levels == ([0, 1, 0, 1] if n == 1025 else [1, 2, 1, 2])


# ---- 4. marginals on the new seams ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("cg1025", "cg2050", "span", "n2049"))
def test_marginals_on_the_new_seams(name):
    """graph_marginals_numpy's model and metric at the start poses and at the model's solution: F = 1 024 (the last one-workgroup size)
    and 2 049 (two launched levels) under CG, `span`, and F = 2 049 with no long factor.  Under CG the reduction is the preconditioner,
    and one that is slightly off still converges to the right columns; in the last case the six-column reduction IS the answer.  The
    model's blocks are computed here, two ways; their whitened difference is d_case, which must stay within the 1e-9 the stored
    marginals cases are held to.  The second request goes one column node per chunk."""
    plain = sc.make_case(name)
    prob = gi.with_info(plain)
    pairs = gm.request(prob)
    g = tg.build(plain)
    for tag, x, options in (("start", prob["poses"], {}), ("solved", model_poses(name), dict(scratch_bytes=1))):
        H = gm.hessian(prob, x)
        want, sd = gm.blocks(prob, x, pairs, H=H)
        alt, _ = gm.blocks(prob, x, pairs, scaled=True, H=H)
        d_case = gm.whitened(want, alt, sd)
        g.set_poses(x)
        S, sm = g.marginals(pairs, **options)
        dev = gm.whitened(S, want, sd)
        print("case %s poses %s: whitened deviation %.3g (d_case %.3g)  columns %d  cg %d unconverged %d  pivot ratio %.3g" %
              (name, tag, dev, d_case, sm.n_columns, sm.cg_iterations, sm.cg_unconverged, sm.min_pivot_ratio))
        assert d_case <= 1e-9
        free_cols = {int(b) for a, b in pairs if not prob["fixed"][a] and not prob["fixed"][b]}
        assert (sm.n_pairs, sm.n_columns, sm.singular, sm.cg_unconverged) == (len(pairs), 6 * len(free_cols), 0, 0)
        assert dev <= max(1e-9, 10.0 * d_case)
        if options:
            whole, smw = g.marginals(pairs)
            assert whole.tobytes() == S.tobytes() and smw.cg_iterations == sm.cg_iterations
    assert g.poses().tobytes() == np.ascontiguousarray(model_poses(name)).tobytes()


# ---- 5. the sign of a quaternion -----------------------------------------------------------------------------------------------

def test_the_sign_of_a_pose_quaternion_changes_nothing():
    """`signs` is `signs_twin` with every second pose handed over as -q.  The plain edge takes vec(E.q) as it comes, and E.q keeps its
    sign when q_i and q_j both flip or neither does; where one flips, r and J flip together, and J^T J, J^T r and |r|^2 do not see it.
    Counters, accept list and costs are therefore equal; the poses, where bytes are promised for information edges only, lie within the
    case's bound of each other by pose_distance, which does not see the sign."""
    out = {}
    for name in ("signs", "signs_twin"):
        g = tg.build(sc.make_case(name))
        s = g.optimize()
        out[name] = (s, g.trace(), g.poses())
    (sa, (acca, canda), xa), (sb, (accb, candb), xb) = out["signs"], out["signs_twin"]
    dev = gn.pose_distance(xa, xb)
    print("signs against its twin: pose deviation %.3g, final cost %.17g / %.17g" % (dev, sa.final_cost, sb.final_cost))
    assert (sa.status, sa.termination, sa.iterations, sa.successful_steps, sa.cg_iterations, sa.cg_unconverged, sa.n_long_edges, sa.n_free) == \
           (sb.status, sb.termination, sb.iterations, sb.successful_steps, sb.cg_iterations, sb.cg_unconverged, sb.n_long_edges, sb.n_free)
    assert acca.tolist() == accb.tolist()
    assert canda.tolist() == candb.tolist()
    assert (sa.initial_cost, sa.final_cost) == (sb.initial_cost, sb.final_cost)
    assert dev <= pose_bound("signs")
