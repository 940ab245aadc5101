"""GPU: msfl_graph_marginals (docs/kernels/graph.md, "Marginals") against the numpy model (tests/graph_marginals_numpy.py) whose results
are stored in tests/golden/graph_marginals_model_v1.npz (tests/golden/make_graph_marginals_golden.py).

The bar is the solver's: the whitened difference max |A_ij - B_ij| / (sd_i sd_j) within max(1e-9, 10 x d_case) of the model, no singular
flag, no unconverged column.  Blocks are asked for at the start poses and again after an optimize; for the second request the poses are
set to the ones the MODEL's optimisation ended at (stored), so that both sides linearise at the same point and the bar measures the
marginals alone, not the 1e-9 by which two optimisers' end poses differ.  The figures are printed (run with -s)."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import graph_marginals_numpy as gm
from tests import test_gpu_graph_info as tgi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_MIN_PIVOT_RATIO = 1e-7


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "graph_marginals_model_v1.npz")))


@functools.lru_cache(maxsize=None)
def case(name):
    return gm.make_case(name)


def summary_tuple(s):
    return (s.n_pairs, s.n_columns, s.cg_iterations, s.cg_unconverged, s.singular, s.min_pivot_ratio)


def n_columns(prob, pairs):
    fixed = prob["fixed"]
    return 6 * len({int(b) for a, b in pairs if not fixed[a] and not fixed[b]})


# ---- 1. parity with the stored model --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", gm.CASES)
def test_parity_with_the_model(name):
    gold, prob = golden(), case(name)
    pairs, d_case = gold["pairs_" + name], float(gold["d_" + name])
    g = tgi.build(prob)
    for tag in ("0", "1"):
        if tag == "1":
            assert g.optimize().iterations >= 0
            g.set_poses(gold["x1_" + name])
        S, sm = g.marginals(pairs)
        want, sd = gold["S%s_%s" % (tag, name)], gold["sd%s_%s" % (tag, name)]
        dev = gm.whitened(S, want, sd)
        print("case %s poses %s: whitened deviation %.3g (d_case %.3g)  columns %d  cg %d unconverged %d  pivot ratio %.3g (model %.3g)" %
              (name, tag, dev, d_case, sm.n_columns, sm.cg_iterations, sm.cg_unconverged, sm.min_pivot_ratio, gold["piv_" + name][int(tag)]))
        assert (sm.n_pairs, sm.n_columns, sm.singular, sm.cg_unconverged) == (len(pairs), n_columns(prob, pairs), 0, 0)
        assert dev <= max(1e-9, 10.0 * d_case)
        assert abs(sm.min_pivot_ratio - gold["piv_" + name][int(tag)]) <= 1e-6 * sm.min_pivot_ratio
        seen = {}
        for k, (a, b) in enumerate(pairs.tolist()):
            if prob["fixed"][a] or prob["fixed"][b]:
                assert not S[k].any()
            if a == b:
                assert np.array_equal(S[k], S[k].T)
            assert seen.setdefault((a, b), S[k].tobytes()) == S[k].tobytes()              # a duplicate is the same bytes
        assert len(seen) < len(pairs)


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", gm.UNANCHORED)
def test_an_unanchored_graph_is_refused_and_nothing_is_written(name):
    from msf_loam_amd import capi
    prob = case(name)
    g = tgi.build(prob)
    mark = np.arange(72.0).reshape(2, 6, 6) + 1000.0
    out = mark.copy()
    assert g.marginals([(1, 1), (2, 5)], out=out, allow=(capi.BAD_ARG,)) == capi.BAD_ARG
    assert np.array_equal(out, mark) and g.last_error()


@pytest.mark.parametrize("name", gm.SINGULAR)
def test_a_free_gauge_direction_is_flagged_and_every_block_is_nan(name):
    from msf_loam_amd import capi
    prob = case(name)
    g = tgi.build(prob)
    S, sm = g.marginals([(0, 0), (1, 2), (2, 2)])
    print("case %s: pivot ratio %.3g on the device, %.3g in the model" % (name, sm.min_pivot_ratio, golden()["piv_" + name]))
    assert sm.singular == 1 and sm.min_pivot_ratio < DEFAULT_MIN_PIVOT_RATIO and np.isnan(S).all()
    import torch
    out = torch.zeros(3 * 36, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()                              # the graph works on a stream of its own
    _, sm2 = g.marginals([(0, 0), (1, 2), (2, 2)], out=out)
    g.synchronize()
    assert sm2.singular == 1 and bool(torch.isnan(out).all())
    # the threshold is the caller's: at zero nothing is flagged (the blocks are then what the arithmetic gives)
    _, sm3 = g.marginals([(0, 0)], min_pivot_ratio=0.0)
    assert sm3.singular == (1 if sm3.min_pivot_ratio < 0.0 else 0)
    assert g.optimize().status == capi.OK


def test_bad_requests():
    from msf_loam_amd import capi
    prob = case("b")
    n = len(prob["poses"])
    g = tgi.build(prob)
    mark = np.arange(72.0).reshape(2, 6, 6) + 1000.0
    for pairs in ([(0, n), (1, 1)], [(1, 1), (-1, 2)], [(n, n), (1, 1)]):
        out = mark.copy()
        assert g.marginals(pairs, out=out, allow=(capi.BAD_ARG,)) == capi.BAD_ARG
        assert np.array_equal(out, mark) and g.last_error()
    for bad in (dict(min_pivot_ratio=np.nan), dict(min_pivot_ratio=-1.0), dict(max_cg_iterations=-1)):
        assert g.marginals([(1, 1)], allow=(capi.BAD_ARG,), **bad) == capi.BAD_ARG
    S, sm = g.marginals(np.zeros((0, 2), np.int32))
    assert S.shape == (0, 6, 6) and summary_tuple(sm) == (0, 0, 0, 0, 0, 0.0)
    # free nodes but no factor
    e = capi.PoseGraph(max_nodes=3, max_edges=1, max_fixes=1)
    e.add_nodes(prob["poses"][:3])
    e.set_fixed(0)
    assert e.marginals([(1, 1)], allow=(capi.BAD_ARG,)) == capi.BAD_ARG
    # every node fixed: zero variance
    e.set_fixed(1); e.set_fixed(2)
    S, sm = e.marginals([(1, 1), (0, 2)])
    assert not S.any() and sm.n_columns == 0 and sm.singular == 0
    # a cap that is too low is reported, and the blocks are delivered as they are
    S, sm = g.marginals([(5, 5)], max_cg_iterations=2)
    assert sm.cg_unconverged == 6 and sm.cg_iterations == 2 and np.isfinite(S).all()


# ---- 3. bytes -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("iii", "free4"))
def test_a_block_does_not_depend_on_what_else_is_asked(name):
    """One call, one pair per call, reversed order, a byte budget that holds one column node at a time, device output: the same bytes
    per pair (iii: CG with 8 long factors; free4: the direct solve)."""
    import torch
    prob = case(name)
    pairs = golden()["pairs_" + name]
    g = tgi.build(prob)
    S, sm = g.marginals(pairs)
    for k, p in enumerate(pairs):
        one, _ = g.marginals([p])
        assert one[0].tobytes() == S[k].tobytes(), (k, p)
    R, _ = g.marginals(pairs[::-1])
    assert R[::-1].tobytes() == S.tobytes()
    C, smc = g.marginals(pairs, scratch_bytes=1)
    assert C.tobytes() == S.tobytes() and summary_tuple(smc) == summary_tuple(sm)
    out = torch.zeros(len(pairs) * 36, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()                              # the graph works on a stream of its own
    _, smd = g.marginals(pairs, out=out)
    g.synchronize()
    assert out.cpu().numpy().tobytes() == S.tobytes() and summary_tuple(smd) == summary_tuple(sm)


# ---- 4. the call changes nothing ---------------------------------------------------------------------------------------------------

def test_marginals_leave_the_graph_and_the_next_optimize_as_they_were():
    from msf_loam_amd import capi
    prob = case("iii")
    pairs = golden()["pairs_iii"]
    a, b = tgi.build(prob), tgi.build(prob)
    sa, sb = a.optimize(), b.optimize()
    assert tgi.summary_tuple(sa) == tgi.summary_tuple(sb)
    before = (b.poses().tobytes(), b.cost(), [b.chi2(k).tobytes() for k in range(4)], [t.tobytes() for t in b.trace()])
    S, sm = b.marginals(pairs)
    assert sm.singular == 0 and np.isfinite(S).all()
    assert before == (b.poses().tobytes(), b.cost(), [b.chi2(k).tobytes() for k in range(4)], [t.tobytes() for t in b.trace()])
    sa, sb = a.optimize(), b.optimize()
    assert bytes(sa) == bytes(sb) and sa.status == capi.OK
    assert a.poses().tobytes() == b.poses().tobytes()
    assert [t.tobytes() for t in a.trace()] == [t.tobytes() for t in b.trace()]
    # a structure change after the call is picked up: the freed node's block appears
    b.set_fixed(int(pairs[0][0]))
    S2, _ = b.marginals(pairs[:1])
    assert not S2.any()


# ---- 5. the C++ face -----------------------------------------------------------------------------------------------------------------

def test_cpp_face_equals_the_ctypes_path(tmp_path):
    """Case (ii) at its start poses through msfl::PoseGraph::Marginals / msfl::RelativeCovariance and through ctypes: equal bytes."""
    from msf_loam_amd import capi
    exe = str(tmp_path / "graph_marginals_face_check")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "graph_marginals_face_check.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "msf_loam_amd"), "-lmsfl_hip", "-Wl,-rpath," + os.path.join(ROOT, "msf_loam_amd")])
    prob = case("ii")
    e, _, ge, _ = tgi.records(prob)
    free = np.nonzero(~prob["fixed"])[0]
    a, b = int(free[2]), int(free[-1])
    pairs = np.concatenate([np.array([(a, a), (a, b), (b, b)], np.int32), golden()["pairs_ii"]])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(prob["poses"]), len(e), len(ge), len(pairs)], np.int32).tobytes())
        f.write(np.ascontiguousarray(prob["poses"]).tobytes())
        f.write(prob["fixed"].astype(np.int32).tobytes())
        f.write(e.tobytes()); f.write(ge.tobytes()); f.write(pairs.tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw = open(tmp_path / "out.bin", "rb").read()
    n = len(pairs)
    assert len(raw) == n * 288 + 32 + 288
    g = tgi.build(prob)
    S, sm = g.marginals(pairs)
    assert sm.singular == 0 and sm.n_columns > 0
    assert raw[:n * 288] == S.tobytes() and raw[n * 288:n * 288 + 32] == bytes(sm)
    s, C = capi.relative_covariance(prob["poses"][a], prob["poses"][b], S[0], S[1], S[2])
    assert s == capi.OK and raw[n * 288 + 32:] == C.tobytes()
