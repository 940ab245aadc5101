"""GPU: information-weighted factors of the pose graph (msfl_graph_add_edges_info / add_fixes_info / factor_chi2 and the two host
helpers; docs/kernels/graph.md) against the numpy model (tests/graph_info_numpy.py) whose results are stored in
tests/golden/graph_info_model_v1.npz (tests/golden/make_graph_info_golden.py), and graphs WITHOUT an information factor against what
the parent commit returned for them (tests/golden/graph_parent_v1.npz, tests/golden/make_graph_parent_golden.py).

The bars are those of tests/test_gpu_graph.py: termination, iterations, successful steps and the accept list exact, costs to 1e-9
relative, poses within max(1e-9, 10 x d_case) of the model, no unconverged step solve.  The figures are printed (run with -s)."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import common
from tests import graph_info_numpy as gi
from tests import graph_numpy as gn
from tests import graph_parent_cases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDERS = ("edges", "fixes", "edges_info", "fixes_info")


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "graph_info_model_v1.npz")))


def case(name):
    g = golden()
    return {k: g["%s_%s" % (k, name)] for k in gi.KEYS}


def records(prob):
    """The four record arrays of a problem, in the order of ADDERS."""
    from msf_loam_amd import capi
    G = capi.PoseGraph
    return (G.edges(prob["ei"], prob["ej"], prob["ez"], prob["esr"], prob["est"]) if len(prob["ei"]) else np.zeros(0, capi.GRAPH_EDGE_DTYPE),
            G.fixes(prob["fi"], prob["fj"], prob["ft"], prob["fp"], prob["fst"]) if len(prob["fi"]) else np.zeros(0, capi.GRAPH_FIX_DTYPE),
            G.edges_info(prob["gi"], prob["gj"], prob["gz"], prob["gL"]) if len(prob["gi"]) else np.zeros(0, capi.GRAPH_EDGE_INFO_DTYPE),
            G.fixes_info(prob["hi"], prob["hj"], prob["ht"], prob["hp"], prob["hL"]) if len(prob["hi"]) else np.zeros(0, capi.GRAPH_FIX_INFO_DTYPE))


def build(prob, chunk=None, order=(0, 1, 2, 3), interleave=False, device_nodes=False, recs=None, **cfg):
    """A PoseGraph holding `prob`.  chunk: records per add_* call (None: one call per kind); order: the kinds' call order; interleave: the
    kinds take turns, one chunk each; device_nodes: poses handed over from device memory."""
    from msf_loam_amd import capi
    n = len(prob["poses"])
    recs = records(prob) if recs is None else recs
    cfg.setdefault("max_nodes", n)
    cfg.setdefault("max_edges", max(1, len(recs[0]) + len(recs[2])))
    cfg.setdefault("max_fixes", max(1, len(recs[1]) + len(recs[3])))
    g = capi.PoseGraph(**cfg)
    p = np.ascontiguousarray(prob["poses"])
    if device_nodes:
        import torch
        p = torch.from_numpy(p).cuda()
    assert g.add_nodes(p) == 0
    for k in np.nonzero(prob["fixed"])[0]:
        g.set_fixed(int(k))
    calls = []
    for q in order:
        step = chunk or max(1, len(recs[q]))
        calls.append([(q, a, a + step) for a in range(0, len(recs[q]), step)])
    if interleave:
        flat = [c[k] for k in range(max(len(c) for c in calls)) for c in calls if k < len(c)]
    else:
        flat = [x for c in calls for x in c]
    for q, a, b in flat:
        getattr(g, "add_" + ADDERS[q])(recs[q][a:b])
    return g


def summary_tuple(s):
    return (s.status, s.termination, s.iterations, s.successful_steps, s.initial_cost, s.final_cost, s.cg_iterations, s.cg_unconverged,
            s.n_long_edges, s.n_free)


# ---- 1. parity with the stored model ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def solved(name):
    """One optimize per case, shared by the tests that look at its result."""
    prob = case(name)
    g = build(prob)
    s = g.optimize()
    return g, s, g.trace()[0], g.poses()


@pytest.mark.parametrize("name", gi.CASES)
def test_parity_with_the_model(name):
    gold, prob = golden(), case(name)
    g, s, acc, x = solved(name)
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


def test_corridor_relations_hold_for_the_device_poses():
    gold = golden()
    truth = gold["truth_iv"]
    odometry = gi.ate(case("iv_rank5")["poses"], truth)
    plain, isotropic, rank5 = (gi.ate(solved("iv_" + f)[3], truth) for f in gi.CORRIDOR_FORMS)
    print("corridor ATE on the device: odometry %.3f, plain %.3f, isotropic %.3f, rank 5 %.3f (model %s)" % (odometry, plain, isotropic, rank5, gold["ate_iv"]))
    assert rank5 < odometry
    assert plain > 5 * rank5 and isotropic > 5 * rank5


# ---- 2. nothing changes for graphs without an information factor ------------------------------------------------------------

def test_plain_graphs_return_the_parents_bytes():
    from msf_loam_amd import capi
    want = dict(np.load(os.path.join(ROOT, "tests", "golden", "graph_parent_v1.npz")))
    got = pc.run(capi)
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k].tobytes() == want[k].tobytes(), k


# ---- 3. isotropic information edges cost what plain edges cost ----------------------------------------------------------------

def test_cost_of_isotropic_information_edges_equals_the_plain_cost():
    gold = dict(np.load(os.path.join(ROOT, "tests", "golden", "graph_model_v1.npz")))
    prob = gi.with_info({k: gold["%s_d" % k] for k in pc.KEYS})
    info = gi.edges_as_info(prob)
    a, b = build(prob), build(info)
    for x in (prob["poses"], gold["x_d"]):
        a.set_poses(x); b.set_poses(x)
        ca, cb = a.cost(), b.cost()
        print("msfl_graph_cost: plain %.15g, information %.15g, relative difference %.3g" % (ca, cb, abs(ca - cb) / ca))
        assert abs(ca - cb) <= 1e-10 * ca


# ---- 4. the sign of z.q ---------------------------------------------------------------------------------------------------------

def test_negated_measurement_quaternion_gives_the_same_bits():
    prob = case("iii")
    _, s, _, x = solved("iii")
    neg = dict(prob)
    neg["gz"] = prob["gz"].copy(); neg["gz"][:, 3:] *= -1.0
    g = build(neg)
    assert g.cost() == build(prob).cost()
    assert summary_tuple(g.optimize()) == summary_tuple(s)
    assert g.poses().tobytes() == x.tobytes()


# ---- 5. bit reproducibility -------------------------------------------------------------------------------------------------------

def test_same_records_same_bits_however_they_arrive():
    prob = case("iii")
    a, sa, _, xa = solved("iii")
    for kw in (dict(chunk=1), dict(order=(3, 2, 1, 0)), dict(chunk=5, order=(2, 0, 3, 1), interleave=True), dict(device_nodes=True)):
        b = build(prob, **kw)
        sb = b.optimize()
        assert summary_tuple(sb) == summary_tuple(sa), kw
        assert b.poses().tobytes() == xa.tobytes(), kw
    b.set_poses(prob["poses"])
    assert summary_tuple(b.optimize()) == summary_tuple(sa)
    assert b.poses().tobytes() == xa.tobytes()


# ---- 6. chi-square read-back --------------------------------------------------------------------------------------------------------

CHI2_ROW_ROUNDING = 1e-11     # a residual row: poses up to ~30 m through weights up to 200, some 15 operations at eps 1.1e-16


@pytest.mark.parametrize("name", ("iii", "v"))
def test_factor_chi2_equals_the_model_and_changes_nothing(name):
    """1e-9 relative on |r|^2.  At the start poses the chain factors' residuals are rounding alone (the poses are the odometry
    integrated), and a relative bar on the square of a rounding error checks nothing: there the bar is the rounding's own size,
    2 |r| d + d^2 with d = CHI2_ROW_ROUNDING, which is below 1e-9 |r|^2 for every |r| > 2e-2."""
    from msf_loam_amd import capi
    prob = case(name)
    g = build(prob)
    for x in (prob["poses"], golden()["x_" + name]):
        g.set_poses(x)
        before, cost = g.poses(), g.cost()
        want = gi.chi2(prob, x)
        for kind in range(4):
            got = g.chi2(kind)
            assert got.shape == want[kind].shape
            tol = np.maximum(1e-9 * want[kind], 2.0 * np.sqrt(want[kind]) * CHI2_ROW_ROUNDING + CHI2_ROW_ROUNDING ** 2)
            if len(got):
                big = want[kind] > 1e-3
                print("case %s kind %d: largest relative difference %.3g over %d factors with |r|^2 > 1e-3; largest difference / bar %.3g" %
                      (name, kind, np.max(np.abs(got - want[kind])[big] / want[kind][big], initial=0.0), big.sum(), np.max(np.abs(got - want[kind]) / tol)))
            assert np.all(np.abs(got - want[kind]) <= tol)
        if len(want[2]) > 3:                              # a sub-range
            assert np.array_equal(g.chi2(capi.GRAPH_FACTOR_EDGE_INFO, 2, 2), g.chi2(capi.GRAPH_FACTOR_EDGE_INFO)[2:4])
        if name == "v":
            assert int(np.argmax(g.chi2(capi.GRAPH_FACTOR_EDGE_INFO))) == 2       # the closure that is 5 m wrong
        assert g.poses().tobytes() == before.tobytes() and g.cost() == cost
    n = len(prob["gi"])
    for kind, first, cnt in ((4, 0, 1), (-1, 0, 1), (2, -1, 1), (2, 0, n + 1), (2, n, 1), (3, 0, len(prob["hi"]) + 1), (2, 0, -1)):
        assert g.chi2(kind, first, cnt, allow=(capi.BAD_ARG,)) == capi.BAD_ARG
    assert len(g.chi2(2, n, 0)) == 0


# ---- 7. refusals and capacities -------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_graph_unchanged():
    from msf_loam_amd import capi
    prob = case("ii")
    _, want_s, _, want_x = solved("ii")
    want_cost = build(prob).cost()
    n = len(prob["poses"])
    g = build(prob, max_edges=len(prob["ei"]) + len(prob["gi"]) + 2, max_fixes=3)
    before = g.poses()
    z, L = prob["gz"][0], prob["gL"][0]
    E = g.edges_info
    bad_L = [L.copy() for _ in range(3)]
    bad_L[0][2, 3] = np.nan; bad_L[1][5, 5] = np.inf; bad_L[2][:] = 0.0
    bad_edges = [
        E(n, 0, z, L), E(-1, 0, z, L), E(0, n, z, L), E(0, -1, z, L), E(3, 3, z, L),
        E(0, 5, np.r_[np.nan, z[1:]], L), E(0, 5, np.r_[z[:6], np.inf], L), E(0, 5, np.r_[z[:3], 0, 0, 0, 0], L),
        E(0, 5, z, bad_L[0]), E(0, 5, z, bad_L[1]), E(0, 5, z, bad_L[2]),
        np.concatenate([E(0, 5, z, L), E(0, n, z, L)]),                    # a good record in front of a bad one: nothing is added
    ]
    for rec in bad_edges:
        assert g.add_edges_info(rec, allow=(capi.BAD_ARG,)) == capi.BAD_ARG
        assert g.last_error()
    F = g.fixes_info
    L3 = np.diag([100.0, 100.0, 20.0])
    bad_fixes = [
        F(0, n, 0.5, [0, 0, 0], L3), F(-1, 1, 0.5, [0, 0, 0], L3), F(2, 2, 0.5, [0, 0, 0], L3),
        F(0, 1, -1e-9, [0, 0, 0], L3), F(0, 1, 1.0 + 1e-9, [0, 0, 0], L3), F(0, 1, np.nan, [0, 0, 0], L3),
        F(0, 1, 0.5, [0, np.inf, 0], L3), F(0, 1, 0.5, [0, 0, 0], np.zeros((3, 3))), F(0, 1, 0.5, [0, 0, 0], np.where(np.eye(3) > 0, np.nan, 0.0)),
        np.concatenate([F(0, 1, 0.5, [0, 0, 0], L3), F(0, 1, 2.0, [0, 0, 0], L3)]),
    ]
    for rec in bad_fixes:
        assert g.add_fixes_info(rec, allow=(capi.BAD_ARG,)) == capi.BAD_ARG
        assert g.last_error()
    # capacity: the whole call is refused
    assert g.add_edges_info(np.concatenate([E(0, 5, z, L)] * 3), allow=(capi.CAPACITY,)) == capi.CAPACITY
    assert g.add_fixes_info(np.concatenate([F(0, 1, 0.5, [0, 0, 0], L3)] * 4), allow=(capi.CAPACITY,)) == capi.CAPACITY
    assert g.poses().tobytes() == before.tobytes() and g.cost() == want_cost
    assert summary_tuple(g.optimize()) == summary_tuple(want_s)
    assert g.poses().tobytes() == want_x.tobytes()


def test_plain_and_information_factors_share_a_capacity():
    from msf_loam_amd import capi
    prob = case("iii")
    e, f, ge, gf = records(prob)
    g = capi.PoseGraph(max_nodes=len(prob["poses"]), max_edges=4, max_fixes=2)
    g.add_nodes(prob["poses"])
    assert g.add_edges(e[:3]) == capi.OK and g.add_edges_info(ge[:1]) == capi.OK                 # E - 1 plain + 1 information: exactly full
    assert g.add_edges(e[3:4], allow=(capi.CAPACITY,)) == capi.CAPACITY
    assert g.add_edges_info(ge[1:2], allow=(capi.CAPACITY,)) == capi.CAPACITY
    assert g.add_fixes(f[:1]) == capi.OK and g.add_fixes_info(gf[:1]) == capi.OK
    assert g.add_fixes(f[1:2], allow=(capi.CAPACITY,)) == capi.CAPACITY
    assert g.add_fixes_info(gf[1:2], allow=(capi.CAPACITY,)) == capi.CAPACITY
    assert len(g.chi2(capi.GRAPH_FACTOR_EDGE)) == 3 and len(g.chi2(capi.GRAPH_FACTOR_EDGE_INFO)) == 1
    assert g.optimize().status == capi.OK
    g.clear()                                                                                      # frees both
    assert g.num_nodes() == 0 and g.add_nodes(prob["poses"]) == 0
    assert g.chi2(capi.GRAPH_FACTOR_EDGE_INFO, 0, 1, allow=(capi.BAD_ARG,)) == capi.BAD_ARG
    assert g.add_edges_info(ge[:4]) == capi.OK and g.add_fixes_info(gf[:2]) == capi.OK
    assert g.add_edges(e[:1], allow=(capi.CAPACITY,)) == capi.CAPACITY and g.add_fixes(f[:1], allow=(capi.CAPACITY,)) == capi.CAPACITY


# ---- 8. one real registration -----------------------------------------------------------------------------------------------------------

def test_edge_from_a_real_registration(gpu, oracle):
    from msf_loam_amd import capi
    _, mc, ms = common.small_world()
    pts, ring, truth, guess = common.scans(1)[0]
    _, corner, surf = common.features_from_oracle(oracle, pts, ring)
    h = capi.Handle(0)
    h.set_map(mc, ms)
    h.set_uncertainty(1)
    status, pose, _ = h.match_scan2map(corner, surf, guess)
    u = h.uncertainty(1)[0]
    h.close()
    assert status == 0 and u["valid"] == 1 and u["n_degenerate"] == 0 and u["sigma2"] > 0.0
    pose = np.asarray(pose, np.float64)
    pose_i = np.r_[truth[:3] + [0.4, -0.3, 0.1], gn.qmul(truth[3:], np.array([0.0, 0.0, np.sin(0.1), np.cos(0.1)]))]
    s, rec = capi.edge_from_uncertainty(0, 1, pose_i, pose, u, u["sigma2"])
    assert s == capi.OK
    z, want = gi.edge_from_uncertainty(pose_i, pose, u["information"], 0, u["sigma2"])
    L = rec["sqrt_information"][0]
    # the record's own eigen-decomposition reproduces its information matrix to 1e-12 (tests/test_gpu_uncertainty.py); the helper adds
    # the rounding of one 6 x 6 product: the bound of the CPU helper test
    dev = np.abs(L.T @ L - want).max() / (np.abs(u["information"]).max() / u["sigma2"])
    print("L^T L against the numpy formula: %.3g of max|H| / scale" % dev)
    assert dev <= 1e-12
    assert np.abs(rec["z"][0] - z).max() <= 5e-14
    g = capi.PoseGraph(max_nodes=2, max_edges=1, max_fixes=1)
    off = pose.copy(); off[:3] += [0.06, -0.06, 0.053]                      # 0.1 m off
    g.add_nodes(np.stack([pose_i, off]))
    g.set_fixed(0)
    g.add_edges_info(rec)
    sm = g.optimize()
    end = g.poses()[1]
    print("two-node graph: %s after %d iterations, node 1 ends %.3g m from the registered pose, chi-square %.3g" %
          (capi.GRAPH_TERMINATION[sm.termination], sm.iterations, np.linalg.norm(end[:3] - pose[:3]), g.chi2(capi.GRAPH_FACTOR_EDGE_INFO)[0]))
    assert np.linalg.norm(end[:3] - pose[:3]) <= 1e-6
    assert np.array_equal(g.poses()[0], pose_i)


# ---- 9. the C++ face ----------------------------------------------------------------------------------------------------------------------

def test_cpp_face_equals_the_ctypes_path(tmp_path):
    """Case (ii) with its two closures handed over as registrations (a synthetic record whose information is the closure's L^T L, about the
    relative pose itself) and one information fix, through msfl::PoseGraphEdgeInfo / AddEdgesInfo / AddFixesInfo / Chi2 and through ctypes."""
    from msf_loam_amd import capi
    exe = str(tmp_path / "graph_info_face_check")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "graph_info_face_check.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "msf_loam_amd"), "-lmsfl_hip", "-Wl,-rpath," + os.path.join(ROOT, "msf_loam_amd")])
    prob = case("ii")
    e = records(prob)[0]
    ident = np.array([0, 0, 0, 0, 0, 0, 1.0])
    unc = np.zeros(len(prob["gi"]), capi.UNCERTAINTY_DTYPE)
    for k, L in enumerate(prob["gL"]):
        H = L.T @ L
        lam, V = np.linalg.eigh(H)
        unc["information"][k], unc["eigenvalues"][k], unc["eigenvectors"][k] = H, lam, V.T
        unc["n_degenerate"][k], unc["valid"][k], unc["sigma2"][k] = 6 - np.linalg.matrix_rank(L), 1, 1.0
    assert unc["n_degenerate"].tolist() == [0, 1]
    s, fx = capi.fix_from_covariance(20, 21, 0.25, golden()["x_ii"][20, :3] + [0.01, 0.0, -0.02], np.diag([1e-4, 2e-4, 9e-4]))
    assert s == capi.OK
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(prob["poses"]), len(e), len(unc), 1], np.int32).tobytes())
        f.write(np.ascontiguousarray(prob["poses"]).tobytes())
        f.write(prob["fixed"].astype(np.int32).tobytes())
        f.write(e.tobytes())
        for k in range(len(unc)):
            f.write(np.array([prob["gi"][k], prob["gj"][k]], np.int32).tobytes())
            f.write(np.r_[ident, prob["gz"][k], 1.0].tobytes())
            f.write(unc[k:k + 1].tobytes())
        f.write(fx.tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw = open(tmp_path / "out.bin", "rb").read()
    at = 0

    def take(dtype, n):
        nonlocal at
        a = np.frombuffer(raw, dtype, n, at)
        at += a.nbytes
        return a

    n = len(prob["poses"])
    ce, cx, cs = take(capi.GRAPH_EDGE_INFO_DTYPE, len(unc)), take(np.float64, n * 7), take(np.uint8, 48)
    chi = [take(np.float64, len(e)), take(np.float64, len(unc)), take(np.float64, 1)]
    assert at == len(raw)
    ge = np.concatenate([capi.edge_from_uncertainty(prob["gi"][k], prob["gj"][k], ident, prob["gz"][k], unc[k], 1.0)[1] for k in range(len(unc))])
    assert ge.tobytes() == ce.tobytes()
    for k, L in enumerate(prob["gL"]):
        assert np.abs(ge["sqrt_information"][k].T @ ge["sqrt_information"][k] - L.T @ L).max() <= 1e-12 * np.abs(L.T @ L).max()
    g = build(prob, recs=(e, np.zeros(0, capi.GRAPH_FIX_DTYPE), ge, fx))
    s = g.optimize()
    assert bytes(s) == cs.tobytes() and s.iterations > 0
    assert g.poses().tobytes() == cx.tobytes()
    for kind, c in zip((capi.GRAPH_FACTOR_EDGE, capi.GRAPH_FACTOR_EDGE_INFO, capi.GRAPH_FACTOR_FIX_INFO), chi):
        assert g.chi2(kind).tobytes() == c.tobytes()
