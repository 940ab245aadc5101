"""GPU: a loss per factor (msfl_graph_set_losses / get_losses / factor_weights; docs/kernels/graph.md, "A loss per factor") against the
numpy model (tests/graph_loss_numpy.py) whose results are stored in tests/golden/graph_loss_model_v1.npz
(tests/golden/make_graph_loss_golden.py), and graphs that never set a loss against what the parent commit returned for them
(tests/golden/graph_loss_parent_v1.npz, tests/golden/make_graph_loss_parent_golden.py).

The bars are those of tests/test_gpu_graph_info.py: termination, iterations, successful steps and the accept list exact, costs to 1e-9
relative, poses within max(1e-9, 10 x d_case) of the model, no unconverged step solve.  The figures are printed (run with -s)."""
import functools
import os

import numpy as np
import pytest

from tests import graph_info_numpy as gi
from tests import graph_loss_numpy as gl
from tests import graph_loss_parent_cases as pc
from tests import graph_marginals_numpy as gm
from tests import graph_numpy as gn
from tests import test_gpu_graph_info as tgi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
summary_tuple = tgi.summary_tuple


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "graph_loss_model_v1.npz")))


def case(name):
    g = golden()
    return {k: g["%s_%s" % (k, name)] for k in gl.KEYS}


def loss_records(prob, fk):
    from msf_loam_amd import capi
    lk, la = gl.LOSS_KEYS[fk]
    return capi.PoseGraph.loss_records(prob[lk], prob[la])


def apply_losses(g, prob, chunk=None, order=(0, 1, 2, 3)):
    """msfl_graph_set_losses for every factor kind that holds a factor; chunk: records per call (None: one call per kind)."""
    for fk in order:
        rec = loss_records(prob, fk)
        step = chunk or max(1, len(rec))
        for a in range(0, len(rec), step):
            g.set_losses(fk, rec[a:a + step], first=a, n=len(rec[a:a + step]))


def build(prob, **kw):
    g = tgi.build(prob, **kw)
    apply_losses(g, prob)
    return g


def check_parity(name, g, s, gold, prob):
    acc, x = g.trace()[0], g.poses()
    term, its, ok = (int(v) for v in gold["tr_" + name])
    d_case = float(gold["d_" + name])
    dev = gn.pose_distance(x, gold["x_" + name])
    print("case %s: termination %s iterations %d cg %d unconverged %d long %d  pose deviation %.3g (d_case %.3g)  cost %.12g -> %.12g" %
          (name, s.termination, s.iterations, s.cg_iterations, s.cg_unconverged, s.n_long_edges, dev, d_case, s.initial_cost, s.final_cost))
    assert (s.termination, s.iterations, s.successful_steps) == (term, its, ok)
    assert acc.tolist() == gold["acc_" + name].tolist()
    assert s.n_long_edges == gi.n_long(prob) and s.n_free == int((~prob["fixed"]).sum())
    assert abs(s.initial_cost - gold["cost_" + name][0]) <= 1e-9 * gold["cost_" + name][0]
    assert abs(s.final_cost - gold["cost_" + name][1]) <= 1e-9 * gold["cost_" + name][1]
    assert dev <= max(1e-9, 10.0 * d_case)
    assert s.cg_unconverged == 0
    fixed = np.nonzero(prob["fixed"])[0]
    assert np.array_equal(x[fixed], prob["poses"][fixed])


# ---- 1. parity with the stored model ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def solved(name):
    prob = case(name)
    g = build(prob)
    s = g.optimize()
    return g, s, g.poses()


@pytest.mark.parametrize("name", gl.CASES)
def test_parity_with_the_model(name):
    g, s, _ = solved(name)
    check_parity(name, g, s, golden(), case(name))


def test_the_wrong_closure_is_switched_off_and_the_weights_say_so():
    from msf_loam_amd import capi
    gold, prob = golden(), case("v_gm")
    g, _, x = solved("v_gm")
    g.set_poses(x)
    w = g.weights(capi.GRAPH_FACTOR_EDGE_INFO)
    chi = g.chi2(capi.GRAPH_FACTOR_EDGE_INFO)
    ate, ref = gi.ate(x, gold["truth_v"]), float(gold["table_ate"][1])
    print("Geman-McClure a = 1 on the device: ATE %.3f m (wrong closure removed by hand: %.3f m, start %.3f m), closure weights %s, chi-square %s" %
          (ate, ref, float(gold["ate_start"]), w, chi))
    assert w[gl.WRONG_CLOSURE] < 1e-3 and np.all(np.delete(w, gl.WRONG_CLOSURE) > 0.9)
    assert abs(ate - ref) <= 0.05 * ref
    assert np.all(np.abs(w - gl.weights(prob, x)[2]) <= 1e-12)


# ---- 2. grid tails --------------------------------------------------------------------------------------------------------------

CHI2_ROW_ROUNDING = tgi.CHI2_ROW_ROUNDING


@functools.lru_cache(maxsize=None)
def chain(n_edges):
    """A chain of n_edges plain edges, node 0 fixed, the start poses 3 cm / 3 mrad off the odometry's so that |r|^2 spreads over both
    sides of every b; the six kinds alternate, a = 0.5 .. 2."""
    truth, odo, poses, rng = gn.drive(n_edges + 1, 90 + n_edges)
    noise = np.concatenate([rng.normal(0.0, 0.03, (n_edges + 1, 3)), gn._small_rot(rng, n_edges + 1, 0.003)], -1)
    fixed = np.zeros(n_edges + 1, bool); fixed[0] = True
    prob = gi.problem(gn.pose_mul(poses, noise), fixed)
    gn._chain(prob, odo)
    prob = gl.with_losses(prob)
    k = np.arange(n_edges)
    prob["elk"][:] = k % 6
    prob["ela"][:] = np.where(k % 6 >= gl.HUBER, 0.5 * (1 + (k // 6) % 4), 0.0)
    return prob


@pytest.mark.parametrize("n_edges", (63, 64, 65, 257))
def test_grid_tails_cost_chi2_and_weights_equal_the_model(n_edges):
    from msf_loam_amd import capi
    prob = chain(n_edges)
    g = build(prob)
    x = prob["poses"]
    before = g.poses()
    cost, want_cost = g.cost(), gl.cost(prob, x)
    chi, want_chi = g.chi2(capi.GRAPH_FACTOR_EDGE), gi.chi2(prob, x)[0]
    w, want_w = g.weights(capi.GRAPH_FACTOR_EDGE), gl.weights(prob, x)[0]
    tol = np.maximum(1e-9 * want_chi, 2.0 * np.sqrt(want_chi) * CHI2_ROW_ROUNDING + CHI2_ROW_ROUNDING ** 2)
    print("%d edges: cost %.15g (model %.15g, relative %.3g); chi-square difference / bar %.3g; largest weight difference %.3g; weights %.3g .. %.3g" %
          (n_edges, cost, want_cost, abs(cost - want_cost) / want_cost, np.max(np.abs(chi - want_chi) / tol), np.max(np.abs(w - want_w)), w.min(), w.max()))
    assert len(chi) == len(w) == n_edges
    assert abs(cost - want_cost) <= 1e-9 * want_cost
    assert np.all(np.abs(chi - want_chi) <= tol)
    assert np.all(np.abs(w - want_w) <= 1e-12)
    assert w.min() < 0.5 and w.max() == 1.0
    assert np.array_equal(g.weights(capi.GRAPH_FACTOR_EDGE, n_edges - 3, 3), w[-3:])            # a sub-range at the tail
    assert g.poses().tobytes() == before.tobytes() and g.cost() == cost                           # nothing changed
    for kind, first, cnt in ((4, 0, 1), (-1, 0, 1), (0, -1, 1), (0, 0, n_edges + 1), (0, n_edges, 1), (1, 0, 1), (0, 0, -1)):
        assert g.weights(kind, first, cnt, allow=(capi.BAD_ARG,)) == capi.BAD_ARG
    assert len(g.weights(0, n_edges, 0)) == 0


# ---- 3. broadcast, round trip, clear, later factors, refusals -------------------------------------------------------------------------

def test_broadcast_equals_n_equal_records_and_get_returns_what_was_set():
    from msf_loam_amd import capi
    prob = case("v_gm")
    _, want_s, want_x = solved("v_gm")
    n = len(prob["gi"])
    g = tgi.build(prob, max_edges=len(prob["ei"]) + n + 1)
    assert np.all(g.losses(capi.GRAPH_FACTOR_EDGE_INFO)["kind"] == capi.GRAPH_LOSS_DEFAULT)         # never given one
    assert g.set_losses(capi.GRAPH_FACTOR_EDGE_INFO, (capi.GRAPH_LOSS_GEMAN_MCCLURE, 1.0)) == capi.OK   # one record over the range
    got = g.losses(capi.GRAPH_FACTOR_EDGE_INFO)
    assert got.tobytes() == loss_records(prob, 2).tobytes() and len(got) == n
    assert np.all(g.losses(capi.GRAPH_FACTOR_EDGE)["kind"] == capi.GRAPH_LOSS_DEFAULT) and len(g.losses(capi.GRAPH_FACTOR_EDGE)) == len(prob["ei"])
    assert summary_tuple(g.optimize()) == summary_tuple(want_s) and g.poses().tobytes() == want_x.tobytes()
    # set again: a sub-range, and `a` of a kind that reads none comes back as 0
    rec = capi.PoseGraph.loss_records([capi.GRAPH_LOSS_NONE, capi.GRAPH_LOSS_CAUCHY], [7.0, 0.25])
    assert g.set_losses(capi.GRAPH_FACTOR_EDGE_INFO, rec, first=1, n=2) == capi.OK
    got = g.losses(capi.GRAPH_FACTOR_EDGE_INFO)
    assert got["kind"].tolist() == [5, 1, 4, 5] and got["a"].tolist() == [1.0, 0.0, 0.25, 1.0] and not got["reserved"].any()
    # factors added later start at DEFAULT, in their own kind's numbering
    x = g.poses()
    assert g.add_edges(g.edges(0, 40, gn.relative_pose(x[0], x[40]))) == capi.OK
    assert g.losses(capi.GRAPH_FACTOR_EDGE)["kind"].tolist() == [0] * (len(prob["ei"]) + 1)
    assert g.losses(capi.GRAPH_FACTOR_EDGE_INFO).tobytes() == got.tobytes()
    assert g.weights(capi.GRAPH_FACTOR_EDGE, len(prob["ei"]), 1)[0] == 1.0
    # clear forgets the records
    g.clear()
    assert g.add_nodes(prob["poses"]) == 0
    g.set_fixed(0)
    e, _, ge, _ = tgi.records(prob)
    g.add_edges(e); g.add_edges_info(ge)
    assert np.all(g.losses(capi.GRAPH_FACTOR_EDGE_INFO)["kind"] == capi.GRAPH_LOSS_DEFAULT)
    plain = tgi.build(prob)
    assert summary_tuple(g.optimize()) == summary_tuple(plain.optimize()) and g.poses().tobytes() == plain.poses().tobytes()


def test_refused_calls_leave_the_graph_unchanged():
    from msf_loam_amd import capi
    prob = case("v_gm")
    _, want_s, want_x = solved("v_gm")
    g = build(prob)
    n = len(prob["gi"])
    R = capi.PoseGraph.loss_records
    K = capi.GRAPH_FACTOR_EDGE_INFO
    bad = [
        (K, R(6, 1.0), 0, 1), (K, R(-1, 1.0), 0, 1),                                                          # unknown loss kind
        (K, R(capi.GRAPH_LOSS_HUBER, 0.0), 0, 1), (K, R(capi.GRAPH_LOSS_CAUCHY, -1.0), 0, 1),
        (K, R(capi.GRAPH_LOSS_SOFT_L_ONE, np.nan), 0, 1), (K, R(capi.GRAPH_LOSS_GEMAN_MCCLURE, np.inf), 0, 1),
        (K, R([capi.GRAPH_LOSS_NONE, capi.GRAPH_LOSS_HUBER], [1.0, -np.inf]), 0, 2),                           # a good record in front of a bad one
        (4, R(1), 0, 1), (-1, R(1), 0, 1), (K, R(1), -1, 1), (K, R(1), 0, n + 1), (K, R(1), n, 1), (1, R(1), 0, 1), (K, R(1), 0, -1),
        (K, R([1, 1]), 0, 3), (K, R([1, 1, 1]), 0, 2),                                                         # n_losses neither n nor 1
    ]
    before = g.losses(K)
    for fk, rec, first, cnt in bad:
        assert g.set_losses(fk, rec, first=first, n=cnt, allow=(capi.BAD_ARG,)) == capi.BAD_ARG, (fk, rec, first, cnt)
        assert g.last_error()
    assert g.losses(K, n, 1, allow=(capi.BAD_ARG,)) == capi.BAD_ARG and g.losses(4, 0, 1, allow=(capi.BAD_ARG,)) == capi.BAD_ARG
    assert g.losses(K).tobytes() == before.tobytes()
    assert g.set_losses(K, R(capi.GRAPH_LOSS_NONE, np.nan), first=0, n=0) == capi.OK                          # an empty range reads no record
    assert g.set_losses(K, R(capi.GRAPH_LOSS_NONE, np.nan), first=n - 1, n=1) == capi.OK                      # NONE reads no a
    assert g.set_losses(K, loss_records(prob, 2)) == capi.OK
    assert summary_tuple(g.optimize()) == summary_tuple(want_s)
    assert g.poses().tobytes() == want_x.tobytes()
    # a graph that only ever saw refused calls has no records and returns the bytes of one that saw none
    plain, refused = tgi.build(prob), tgi.build(prob)
    for fk, rec, first, cnt in bad:
        refused.set_losses(fk, rec, first=first, n=cnt, allow=(capi.BAD_ARG,))
    assert summary_tuple(refused.optimize()) == summary_tuple(plain.optimize()) and refused.poses().tobytes() == plain.poses().tobytes()


# ---- 4. a graph that never sets a loss returns the parent's bytes -----------------------------------------------------------------------

def test_graphs_without_a_loss_record_return_the_parents_bytes():
    from msf_loam_amd import capi
    want = dict(np.load(os.path.join(ROOT, "tests", "golden", "graph_loss_parent_v1.npz")))
    got = pc.run(capi)
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k].tobytes() == want[k].tobytes(), k


# ---- 5. HUBER at huber_delta on every factor is the graph's own loss -------------------------------------------------------------------------

def test_huber_at_huber_delta_on_every_factor_against_no_records():
    from msf_loam_amd import capi
    info = dict(np.load(os.path.join(ROOT, "tests", "golden", "graph_info_model_v1.npz")))
    for name in ("iii", "v"):
        prob = gl.with_losses({k: info["%s_%s" % (k, name)] for k in gi.KEYS})
        for fk in range(4):
            gl.set_losses(prob, fk, gl.HUBER, gl.Options.huber_delta)
        g, plain = build(prob), tgi.build(prob)
        assert g.cost() == pytest.approx(plain.cost(), rel=1e-9)
        s, sp = g.optimize(), plain.optimize()
        check_parity(name, g, s, info, prob)
        same = summary_tuple(s) == summary_tuple(sp) and g.poses().tobytes() == plain.poses().tobytes()
        print("case %s: HUBER(a = huber_delta) on every factor and no records give %s bytes" % (name, "the same" if same else "different"))
        for fk in range(4):
            assert np.all(np.abs(g.weights(fk) - plain.weights(fk)) <= 1e-12)


# ---- 6. marginals see the records -------------------------------------------------------------------------------------------------------

def test_marginals_under_a_loss_per_factor():
    """Case (v) at the model's Geman-McClure result: the whitened difference to the model's blocks within max(1e-9, 10 x d_case), the bar
    of tests/test_gpu_graph_marginals.py; the same request under Huber on the closures is far away (0.29 whitened in the model)."""
    gold, prob = golden(), case("v_gm")
    g = build(prob)
    g.set_poses(gold["x_v_gm"])
    pairs, want, sd, d_case = gold["pairs_v_gm"], gold["S_v_gm"], gold["sd_v_gm"], float(gold["dm_v_gm"])
    S, sm = g.marginals(pairs)
    dev = gm.whitened(S, want, sd)
    plain = tgi.build(prob)
    plain.set_poses(gold["x_v_gm"])
    far = gm.whitened(plain.marginals(pairs)[0], want, sd)
    print("marginals of (v) under Geman-McClure: whitened deviation %.3g (d_case %.3g), columns %d, cg %d; without the records %.3g" %
          (dev, d_case, sm.n_columns, sm.cg_iterations, far))
    assert (sm.n_pairs, sm.singular, sm.cg_unconverged) == (len(pairs), 0, 0)
    assert dev <= max(1e-9, 10.0 * d_case)
    assert far > 1e-3


# ---- 7. bit reproducibility -------------------------------------------------------------------------------------------------------------

def test_same_records_and_losses_same_bits_however_they_arrive():
    prob = case("mixed")
    _, sa, xa = solved("mixed")
    for kw, lkw in ((dict(chunk=1), dict(chunk=1)), (dict(order=(3, 2, 1, 0)), dict(order=(2, 0, 3, 1), chunk=7)),
                    (dict(chunk=5, order=(2, 0, 3, 1), interleave=True), dict(chunk=64))):
        b = tgi.build(prob, **kw)
        apply_losses(b, prob, **lkw)
        sb = b.optimize()
        assert summary_tuple(sb) == summary_tuple(sa), (kw, lkw)
        assert b.poses().tobytes() == xa.tobytes(), (kw, lkw)
    # losses first set to something else, then to the case's; and set_losses between add_* calls
    from msf_loam_amd import capi
    recs = tgi.records(prob)
    b = capi.PoseGraph(max_nodes=len(prob["poses"]), max_edges=len(recs[0]) + len(recs[2]), max_fixes=len(recs[1]) + len(recs[3]))
    b.add_nodes(prob["poses"])
    b.add_edges(recs[0])
    b.set_losses(0, (capi.GRAPH_LOSS_CAUCHY, 3.0))
    b.add_fixes_info(recs[3]); b.add_edges_info(recs[2])
    b.set_losses(2, loss_records(prob, 2))
    b.add_fixes(recs[1])
    for fk in (3, 1, 0):
        b.set_losses(fk, loss_records(prob, fk))
    assert summary_tuple(b.optimize()) == summary_tuple(sa) and b.poses().tobytes() == xa.tobytes()
    b.set_poses(prob["poses"])
    assert summary_tuple(b.optimize()) == summary_tuple(sa) and b.poses().tobytes() == xa.tobytes()
