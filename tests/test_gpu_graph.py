"""GPU: the pose graph (msfl_graph_*, docs/kernels/graph.md) against the numpy model (tests/graph_numpy.py) whose results for the
parity cases are stored in tests/golden/graph_model_v1.npz (tests/golden/make_graph_golden.py).

Per case: termination, iterations, successful steps and the accept list are exact, the costs agree to 1e-9 relative, the poses lie
within max(1e-9, 10 x d_case) of the model (d_case: the distance between the model's two exact step solvers; the device's cyclic
reduction + PCG is a third with its own summation order).  The largest pose deviation per case is printed (run with -s).

Case (f) (one closure 5 m wrong, no anchor): Huber is active in it; with the seeded drives tried every step was accepted.  Its
step systems grow ill-conditioned as the trust region opens (no node or fix holds the gauge), and PCG then needs up to ~140
iterations per solve where the default cap 16 n_long + 8 allows 72: at the default cap 8 of its 10 solves end unconverged and the
poses end 2.8e-4 from the model (trace and costs still equal the model's); with max_cg_iterations = 256 every solve converges and
the poses are 1.3e-10 from the model.  The parity test therefore runs (f) with max_cg_iterations = 256, and
test_default_cap_hands_over_and_counts pins what the default cap does on it."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import graph_numpy as gn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("poses", "fixed", "ei", "ej", "ez", "esr", "est", "fi", "fj", "ft", "fp", "fst")


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "graph_model_v1.npz")))


def case(name):
    g = golden()
    return {k: g["%s_%s" % (k, name)] for k in KEYS}


def records(prob):
    from msf_loam_amd import capi
    e = capi.PoseGraph.edges(prob["ei"], prob["ej"], prob["ez"], prob["esr"], prob["est"]) if len(prob["ei"]) else np.zeros(0, capi.GRAPH_EDGE_DTYPE)
    f = capi.PoseGraph.fixes(prob["fi"], prob["fj"], prob["ft"], prob["fp"], prob["fst"]) if len(prob["fi"]) else np.zeros(0, capi.GRAPH_FIX_DTYPE)
    return e, f


def build(prob, chunk=None, device_nodes=False, **cfg):
    """A PoseGraph holding `prob`; chunk: records per add_* call (None: one call each); device_nodes: poses handed over from device memory."""
    from msf_loam_amd import capi
    n = len(prob["poses"])
    e, f = records(prob)
    cfg.setdefault("max_nodes", n); cfg.setdefault("max_edges", max(1, len(e))); cfg.setdefault("max_fixes", max(1, len(f)))
    g = capi.PoseGraph(**cfg)
    step = chunk or max(1, n)
    for a in range(0, n, step):
        p = np.ascontiguousarray(prob["poses"][a:a + step])
        if device_nodes:
            import torch
            p = torch.from_numpy(p).cuda()
        assert g.add_nodes(p) == a
    for k in np.nonzero(prob["fixed"])[0]:
        g.set_fixed(int(k))
    for rec, add in ((e, g.add_edges), (f, g.add_fixes)):
        step = chunk or max(1, len(rec))
        for a in range(0, len(rec), step):
            add(rec[a:a + step])
    return g


def summary_tuple(s):
    return (s.status, s.termination, s.iterations, s.successful_steps, s.initial_cost, s.final_cost, s.cg_iterations, s.cg_unconverged,
            s.n_long_edges, s.n_free)


# ---- 1. parity with the golden model results ------------------------------------------------------------------------------

CONFIG = dict(f=dict(max_cg_iterations=256))        # see the module docstring; every other case runs the default config


@pytest.mark.parametrize("name", gn.CASES)
def test_parity_with_the_model(name):
    gold, prob = golden(), case(name)
    g = build(prob, **CONFIG.get(name, {}))
    s = g.optimize()
    acc, _ = g.trace()
    x = g.poses()
    term, its, ok = (int(v) for v in gold["tr_" + name])
    d_case = float(gold["d_" + name])
    dev = gn.pose_distance(x, gold["x_" + name])
    print("case %s: termination %s iterations %d cg %d unconverged %d long %d  pose deviation %.3g (d_case %.3g)  cost %.12g -> %.12g" %
          (name, s.termination, s.iterations, s.cg_iterations, s.cg_unconverged, s.n_long_edges, dev, d_case, s.initial_cost, s.final_cost))
    assert (s.termination, s.iterations, s.successful_steps) == (term, its, ok)
    assert acc.tolist() == gold["acc_" + name].tolist()
    assert s.n_long_edges == gn.n_long(prob) and s.n_free == int((~prob["fixed"]).sum())
    assert abs(s.initial_cost - gold["cost_" + name][0]) <= 1e-9 * gold["cost_" + name][0]
    assert abs(s.final_cost - gold["cost_" + name][1]) <= 1e-9 * gold["cost_" + name][1]
    assert dev <= max(1e-9, 10.0 * d_case)
    assert s.cg_unconverged == 0
    if s.n_long_edges == 0:
        assert s.cg_iterations == s.iterations          # the tridiagonal solve is the step
    fixed = np.nonzero(prob["fixed"])[0]
    assert np.array_equal(x[fixed], prob["poses"][fixed])


def test_default_cap_hands_over_and_counts():
    """(f) at the default cap of 16 * 4 + 8 CG iterations: solves that end there are counted, their iterates are used, and the
    trust-region trace and the costs (1e-9 relative) still equal the model's."""
    gold, prob = golden(), case("f")
    g = build(prob)
    s = g.optimize()
    assert s.cg_unconverged > 0 and s.cg_iterations <= s.iterations * 72
    assert (s.termination, s.iterations, s.successful_steps) == tuple(int(v) for v in gold["tr_f"])
    assert g.trace()[0].tolist() == gold["acc_f"].tolist()
    assert abs(s.final_cost - gold["cost_f"][1]) <= 1e-9 * gold["cost_f"][1]
    assert np.all(np.isfinite(g.poses()))


def test_rejected_steps_follow_the_model():
    """The reject branch, which no golden case reaches: case (h) with min_relative_decrease = 1.1.  Its steps have a step quality of
    1.97, then 1.003 .. 1.000 (the problem is almost linear), so the first is accepted and every later one rejected, far from the
    threshold, with the radius divided by 2, 4, 8, ... until the parameter tolerance ends the solve.  The model runs here, both variants."""
    class Opt(gn.Options):
        min_relative_decrease = 1.1
    prob = case("h")
    xd, td = gn.solve_dense(prob, Opt)
    xs, ts = gn.solve_sparse(prob, Opt)
    assert td.accepted == ts.accepted and td.termination == ts.termination == "parameter"
    assert td.accepted.count(1) == 1 and td.accepted.count(0) >= 5
    g = build(prob, min_relative_decrease=1.1)
    s = g.optimize()
    acc, cand = g.trace()
    from msf_loam_amd import capi
    assert (capi.GRAPH_TERMINATION[s.termination], s.iterations, s.successful_steps) == (td.termination, td.iterations, td.successful_steps)
    assert acc.tolist() == td.accepted
    assert np.allclose(cand, td.cost, rtol=1e-9, atol=0)
    assert abs(s.final_cost - td.final_cost) <= 1e-9 * td.final_cost
    assert gn.pose_distance(g.poses(), xd) <= max(1e-9, 10.0 * gn.pose_distance(xd, xs))


# ---- 2. bit reproducibility -----------------------------------------------------------------------------------------------

def test_same_records_same_bits_however_they_arrive():
    prob = case("d")
    a = build(prob)
    sa = a.optimize()
    xa = a.poses()
    for kw in (dict(chunk=7), dict(device_nodes=True), dict(chunk=1, device_nodes=True)):
        b = build(prob, **kw)
        sb = b.optimize()
        assert summary_tuple(sb) == summary_tuple(sa)
        assert b.poses().tobytes() == xa.tobytes()
    a.set_poses(prob["poses"])
    assert summary_tuple(a.optimize()) == summary_tuple(sa)
    assert a.poses().tobytes() == xa.tobytes()


# ---- 3. msfl_graph_cost ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("a", "e", "f"))
def test_cost_equals_the_model_and_changes_nothing(name):
    prob = case(name)
    g = build(prob)
    before = g.poses()
    want = gn.cost(prob)
    got = g.cost()
    assert abs(got - want) <= 1e-12 * want
    assert g.poses().tobytes() == before.tobytes() == np.ascontiguousarray(prob["poses"]).tobytes()
    assert g.cost() == got


# ---- 4. refusals and edge states ------------------------------------------------------------------------------------------

def test_refusals_leave_the_graph_unchanged():
    from msf_loam_amd import capi
    prob = case("b")
    ref = build(prob)
    want_s, want_x = summary_tuple(ref.optimize()), ref.poses()
    n = len(prob["poses"])
    g = build(prob, max_nodes=n + 2, max_edges=len(prob["ei"]) + 2, max_fixes=4)
    before = g.poses()
    z = prob["ez"][0]
    bad_edges = [
        g.edges(n, 0, z), g.edges(-1, 0, z), g.edges(0, n, z), g.edges(3, 3, z),
        g.edges(0, 5, np.r_[np.nan, z[1:]]), g.edges(0, 5, np.r_[z[:3], 0, 0, 0, 0]), g.edges(0, 5, np.r_[z[:6], np.inf]),
        g.edges(0, 5, z, sr=0.0), g.edges(0, 5, z, st=-1.0), g.edges(0, 5, z, sr=np.nan),
        np.concatenate([g.edges(0, 5, z), g.edges(0, n, z)]),                     # a good record in front of a bad one: nothing is added
    ]
    for rec in bad_edges:
        assert g.add_edges(rec, allow=(capi.BAD_ARG,)) == capi.BAD_ARG
        assert g.last_error()
    bad_fixes = [
        g.fixes(0, n, 0.5, [0, 0, 0]), g.fixes(-1, 1, 0.5, [0, 0, 0]), g.fixes(2, 2, 0.5, [0, 0, 0]),
        g.fixes(0, 1, -1e-9, [0, 0, 0]), g.fixes(0, 1, 1.0 + 1e-9, [0, 0, 0]), g.fixes(0, 1, np.nan, [0, 0, 0]),
        g.fixes(0, 1, 0.5, [0, np.inf, 0]), g.fixes(0, 1, 0.5, [0, 0, 0], st=0.0), g.fixes(0, 1, 0.5, [0, 0, 0], st=np.nan),
    ]
    for rec in bad_fixes:
        assert g.add_fixes(rec, allow=(capi.BAD_ARG,)) == capi.BAD_ARG
    p = prob["poses"][:2].copy()
    for bad in (np.nan, np.inf):
        q = p.copy(); q[1, 2] = bad
        assert g.add_nodes(q, allow=(capi.BAD_ARG,)) == capi.BAD_ARG
        assert g.set_poses(q, first=3, allow=(capi.BAD_ARG,)) == capi.BAD_ARG
    q = p.copy(); q[0, 3:] = 0.0
    assert g.add_nodes(q, allow=(capi.BAD_ARG,)) == capi.BAD_ARG
    assert g.set_poses(q, first=0, allow=(capi.BAD_ARG,)) == capi.BAD_ARG
    assert g.set_poses(p, first=n - 1, allow=(capi.BAD_ARG,)) == capi.BAD_ARG     # range past the last node
    assert g.set_fixed(n, True, allow=(capi.BAD_ARG,)) == capi.BAD_ARG
    assert g.set_fixed(-1, True, allow=(capi.BAD_ARG,)) == capi.BAD_ARG
    # capacity: the whole call is refused
    assert g.add_nodes(np.tile(p[:1], (3, 1)), allow=(capi.CAPACITY,)) == capi.CAPACITY
    assert g.add_edges(np.concatenate([g.edges(0, 5, z)] * 3), allow=(capi.CAPACITY,)) == capi.CAPACITY
    assert g.add_fixes(np.concatenate([g.fixes(0, 1, 0.5, [0, 0, 0])] * 5), allow=(capi.CAPACITY,)) == capi.CAPACITY
    assert g.num_nodes() == n
    assert g.poses().tobytes() == before.tobytes()
    assert summary_tuple(g.optimize()) == want_s
    assert g.poses().tobytes() == want_x.tobytes()


def test_capacity_exactly_reached_and_exceeded_by_one():
    from msf_loam_amd import capi
    prob = case("a")
    e, f = records(prob)
    g = capi.PoseGraph(max_nodes=3, max_edges=2, max_fixes=2)
    assert g.add_nodes(prob["poses"][:2]) == 0 and g.add_nodes(prob["poses"][2:]) == 2           # exactly full
    assert g.add_nodes(prob["poses"][:1], allow=(capi.CAPACITY,)) == capi.CAPACITY
    assert g.add_edges(e) == capi.OK and g.add_edges(e[:1], allow=(capi.CAPACITY,)) == capi.CAPACITY
    assert g.add_fixes(f) == capi.OK and g.add_fixes(f[:1], allow=(capi.CAPACITY,)) == capi.CAPACITY
    assert g.num_nodes() == 3
    s = g.optimize()
    gold = golden()
    assert (s.termination, s.iterations) == tuple(int(v) for v in gold["tr_a"][:2])
    g.clear()
    assert g.num_nodes() == 0 and g.add_nodes(prob["poses"]) == 0


def test_empty_termination_leaves_the_poses():
    from msf_loam_amd import capi
    prob = case("a")
    e, f = records(prob)
    g = capi.PoseGraph(max_nodes=3)
    s = g.optimize()                                     # nothing at all
    assert s.termination == capi.GRAPH_TERMINATION.index("empty") and s.iterations == 0
    g.add_nodes(prob["poses"])
    s = g.optimize()                                     # no residual block
    assert s.termination == 0 and s.n_free == 3 and g.cost() == 0.0
    g.add_edges(e); g.add_fixes(f)
    for k in range(3):
        g.set_fixed(k)
    s = g.optimize()                                     # no free node
    assert s.termination == 0 and s.n_free == 0
    assert g.poses().tobytes() == np.ascontiguousarray(prob["poses"]).tobytes()
    assert g.trace()[0].tolist() == []
    for k in range(3):
        g.set_fixed(k, False)
    assert g.optimize().termination == int(golden()["tr_a"][0])


# ---- 5. the C++ face ------------------------------------------------------------------------------------------------------

def test_cpp_gps_fusion_and_pose_graph_equal_the_ctypes_path(tmp_path):
    from msf_loam_amd import capi
    exe = str(tmp_path / "graph_check")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "graph_check.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "msf_loam_amd"), "-lmsfl_hip", "-Wl,-rpath," + os.path.join(ROOT, "msf_loam_amd")])
    c, d = case("c"), case("d")
    nc, nx = len(c["poses"]), len(c["fi"])
    times = c["fi"] + c["ft"]                            # pose k is stamped k seconds
    times[-1] = float(nc - 1)                            # the last fixed point exactly at the last pose: (N - 2, N - 1, t = 1)
    de, df = records(d)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([nc, nx], np.int32).tobytes())
        f.write(np.ascontiguousarray(c["poses"]).tobytes())
        f.write(np.ascontiguousarray(np.c_[times, c["fp"]]).tobytes())
        f.write(np.array([len(d["poses"]), len(de), len(df)], np.int32).tobytes())
        f.write(np.ascontiguousarray(d["poses"]).tobytes())
        f.write(d["fixed"].astype(np.int32).tobytes())
        f.write(de.tobytes()); f.write(df.tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw = open(tmp_path / "out.bin", "rb").read()
    at = 0

    def take(dtype, n):
        nonlocal at
        a = np.frombuffer(raw, dtype, n, at)
        at += a.nbytes
        return a

    ce, cf = take(capi.GRAPH_EDGE_DTYPE, nc - 1), take(capi.GRAPH_FIX_DTYPE, nx)
    cx, cs = take(np.float64, nc * 7).reshape(nc, 7), take(np.uint8, 48)
    dx, ds = take(np.float64, len(d["poses"]) * 7), take(np.uint8, 48)
    assert at == len(raw)
    # what GpsFusion built: consecutive edges measured by the local poses themselves, fixes bracketed by upper_bound
    assert ce["i"].tolist() == list(range(nc - 1)) and ce["j"].tolist() == list(range(1, nc))
    assert np.all(ce["sr"] == 0.01) and np.all(ce["st"] == 0.1) and np.all(cf["st"] == 0.01)
    want_z = np.stack([capi.relative_pose(c["poses"][k], c["poses"][k + 1]) for k in range(nc - 1)])
    # two roundings of the same formula: coordinates up to ~30 m, some 15 operations each, eps 1.1e-16: 15 * 30 * 1.1e-16 = 5e-14
    assert np.abs(ce["z"] - want_z).max() <= 5e-14
    assert cf["i"].tolist() == c["fi"][:-1].tolist() + [nc - 2] and cf["j"].tolist() == c["fj"][:-1].tolist() + [nc - 1]
    assert np.abs(cf["t"][:-1] - c["ft"][:-1]).max() <= 1e-12 and cf["t"][-1] == 1.0
    assert np.array_equal(cf["p"], c["fp"])
    # the same records through ctypes give the same bytes
    g = capi.PoseGraph(max_nodes=nc, max_edges=nc, max_fixes=nx)
    g.add_nodes(c["poses"]); g.add_edges(ce); g.add_fixes(cf)
    s = g.optimize()
    assert bytes(s) == cs.tobytes() and s.iterations > 0 and s.cg_iterations == s.iterations
    assert g.poses().tobytes() == cx.tobytes()
    g = build(d)
    s = g.optimize()
    assert bytes(s) == ds.tobytes()
    assert g.poses().tobytes() == dx.tobytes()
