"""CPU: the model of the pose graph's marginal covariances (tests/graph_marginals_numpy.py) against itself, against its stored results
(tests/golden/graph_marginals_model_v1.npz, written by tests/golden/make_graph_marginals_golden.py) and against closed forms; and the
host helper msfl_graph_relative_covariance through the library (it touches no GPU) and as a stand-alone program under the host
sanitizers.  No GPU, no reference."""
import os
import subprocess

import numpy as np
import pytest

from tests import graph_info_numpy as gi
from tests import graph_marginals_numpy as gm
from tests import graph_numpy as gn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "graph_marginals_model_v1.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def chain(n, seed, closure=False):
    truth, odo, poses, rng = gn.drive(n, seed)
    fixed = np.zeros(n, bool); fixed[0] = True
    prob = gi.problem(poses, fixed)
    gn._chain(prob, odo)
    if closure:
        gn._closures(prob, truth, rng, [(0, n - 1)])
    return prob


@pytest.mark.parametrize("name", gm.CASES)
def test_the_stored_file_is_what_the_model_builds(name, golden):
    """Same pairs; blocks within max(1e-12, d_case) whitened (another LAPACK may round differently, by what the two evaluations differ
    by); H Sigma_columns = E to 1e-9 of the largest entry (measured: at most 1.5e-12)."""
    prob = gm.make_case(name)
    pairs = gm.request(prob)
    assert np.array_equal(pairs, golden["pairs_" + name])
    fr, nf = gn.free_index(prob["fixed"])
    d_case = float(golden["d_" + name])
    assert d_case <= 1e-9
    for tag, x in (("0", prob["poses"]), ("1", golden["x1_" + name])):
        H = gm.hessian(prob, x)
        S, sd = gm.blocks(prob, x, pairs, H=H)
        S2, _ = gm.blocks(prob, x, pairs, scaled=True, H=H)
        assert np.allclose(sd, golden["sd%s_%s" % (tag, name)], rtol=1e-9, atol=0)
        assert gm.whitened(S, golden["S%s_%s" % (tag, name)], sd) <= max(1e-12, d_case)
        assert gm.whitened(S, S2, sd) <= max(1e-12, 2.0 * d_case)
        nodes = sorted({int(k) for k in pairs.ravel() if fr[k] >= 0})
        worst = 0.0
        for b, X in gm._columns(prob, nodes, H, False).items():
            E = np.zeros((6 * nf, 6)); E[6 * fr[b] + np.arange(6), np.arange(6)] = 1.0
            worst = max(worst, float(np.abs(H @ X - E).max()))
        print("case %s poses %s: residual of H Sigma = E %.3g" % (name, tag, worst))
        assert worst <= 1e-9
    assert np.allclose(golden["piv_" + name], [gm.cr_min_pivot(gm.hessian(prob, x), nf) for x in (prob["poses"], golden["x1_" + name])], rtol=1e-6, atol=0)


def test_pivot_ratios_separate_anchored_from_gauge_free(golden):
    """The pivot test's default threshold (1e-7) lies between what the anchored cases show and what the two gauge-free ones show."""
    anchored = min(float(golden["piv_" + n].min()) for n in gm.CASES)
    free = max(float(golden["piv_" + n]) for n in gm.SINGULAR)
    print("smallest pivot ratio: anchored cases %.3g, gauge-free cases at most %.3g" % (anchored, free))
    assert anchored >= 1e-2 and free <= 1e-9
    for n in gm.SINGULAR:
        prob = gm.make_case(n)
        H = gm.hessian(prob, prob["poses"])
        ev = np.linalg.eigvalsh(H.toarray())
        assert ev[0] <= 1e-14 * ev[-1]
        assert gm.cr_min_pivot(H, gn.free_index(prob["fixed"])[1]) <= 1e-9
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("name", ("free3", "ii", "iii", "v"))
def test_joint_marginals_are_positive_semidefinite_and_transposes_agree(name, golden):
    prob = gm.make_case(name)
    free = np.nonzero(~prob["fixed"])[0]
    x = golden["x1_" + name]
    H = gm.hessian(prob, x)
    for a, b in ((free[0], free[-1]), (free[1], free[len(free) // 2]), (free[len(free) // 2], free[len(free) // 2 - 1])):
        S, sd = gm.blocks(prob, x, [(a, a), (a, b), (b, a), (b, b)], H=H)
        assert gm.whitened(S[1:2], S[2:3].transpose(0, 2, 1), sd[1:2]) <= 1e-9
        w = np.r_[sd[0, 0], sd[3, 0]]
        joint = np.block([[S[0], S[1]], [S[1].T, S[3]]]) / np.outer(w, w)
        assert np.linalg.eigvalsh(joint).min() >= -1e-9


def test_two_node_graph_equals_the_hand_written_inverse():
    """Node 0 fixed, one information edge L, node 1 at the measurement: e's derivative in the delivered coordinates of node 1 is
    D = diag(R_0^T, R_1^T), so S_11 = (D^T L^T L D)^-1."""
    prob = gm.make_case("two")
    S, sd = gm.blocks(prob, prob["poses"], [(1, 1)])
    D = np.zeros((6, 6))
    D[:3, :3] = gn.quat_to_R(prob["poses"][0, 3:]).T; D[3:, 3:] = gn.quat_to_R(prob["poses"][1, 3:]).T
    L = prob["gL"][0]
    want = np.linalg.inv(D.T @ L.T @ L @ D)
    assert gm.whitened(S, want[None], sd) <= 1e-10


def test_variance_grows_along_an_open_chain_and_peaks_mid_chain_with_a_closure():
    n = 30
    for closure in (False, True):
        prob = chain(n, 51, closure)
        S, _ = gm.blocks(prob, prob["poses"], [(k, k) for k in range(1, n)])
        tr = np.trace(S, axis1=1, axis2=2)
        if closure:
            peak = 1 + int(np.argmax(tr))
            assert n // 3 <= peak <= 2 * n // 3 and tr[-1] < 0.2 * tr.max()
        else:
            assert np.all(np.diff(tr) > 0.0)


def test_relative_covariance_analytic_against_central_differences(golden):
    """h = 1e-6: truncation O(h^2) ~ 1e-12, rounding eps |t| / h ~ 1e-8 of a Jacobian entry of order |u| ~ 40: 1e-6 of the largest entry."""
    prob = gm.make_case("b")
    x = golden["x1_b"]
    for a, b in ((1, 36), (20, 3), (10, 11)):
        Ja, Jb = gm.relative_jacobians(x[a], x[b])
        Na, Nb = gm.relative_jacobians_numeric(x[a], x[b])
        big = max(np.abs(Ja).max(), np.abs(Jb).max())
        assert np.abs(Ja - Na).max() <= 1e-6 * big and np.abs(Jb - Nb).max() <= 1e-6 * big
        S, _ = gm.blocks(prob, x, [(a, a), (a, b), (b, b)])
        C, N = gm.relative_covariance(x[a], x[b], *S), gm.relative_covariance(x[a], x[b], *S, jacobians=gm.relative_jacobians_numeric)
        assert np.abs(C - N).max() <= 1e-6 * np.abs(C).max()
        assert np.array_equal(C, C.T) and np.linalg.eigvalsh(C).min() > 0.0


def test_relative_covariance_across_an_information_edge_gives_the_edges_own_tangent_back():
    """Two nodes, node 0 fixed, one information edge: the covariance of T_0^-1 T_1 is (L^T L)^-1.  This pins the convention."""
    prob = gm.make_case("two")
    x = prob["poses"]
    S, _ = gm.blocks(prob, x, [(0, 0), (0, 1), (1, 1)])
    assert not S[0].any() and not S[1].any()
    L = prob["gL"][0]
    want = np.linalg.inv(L.T @ L)
    C = gm.relative_covariance(x[0], x[1], *S)
    assert np.abs(C - want).max() <= 1e-10 * np.abs(want).max()


def _records(golden):
    """Stored inputs for the C helper: three pairs of case b at its solved poses."""
    x, pairs, S = golden["x1_b"], golden["pairs_b"].tolist(), golden["S1_b"]
    at = lambda a, b: S[pairs.index([a, b])]
    free = [int(k) for k in np.nonzero(~gm.make_case("b")["fixed"])[0]]
    a, b = free[0], free[-1]
    return [(x[a], x[b], at(a, a), at(a, b), at(b, b)), (x[b], x[a], at(b, b), at(b, a), at(a, a))]


def test_the_library_helper_equals_the_model_and_refuses_without_writing(golden):
    from msf_loam_amd import capi
    for pa, pb, Saa, Sab, Sbb in _records(golden):
        s, C = capi.relative_covariance(pa, pb, Saa, Sab, Sbb)
        want = gm.relative_covariance(pa, pb, Saa, Sab, Sbb)
        assert s == capi.OK and np.abs(C - want).max() <= 1e-12 * np.abs(want).max()
        mark = np.arange(36.0).reshape(6, 6) + 1000.0
        for bad in (np.nan, np.inf):
            out = mark.copy()
            s, _ = capi.relative_covariance(np.r_[bad, pa[1:]], pb, Saa, Sab, Sbb, out=out)
            assert s == capi.BAD_ARG and np.array_equal(out, mark)
            Sx = Sab.copy(); Sx[2, 3] = bad
            s, _ = capi.relative_covariance(pa, pb, Saa, Sx, Sbb, out=out)
            assert s == capi.BAD_ARG and np.array_equal(out, mark)
        s, _ = capi.relative_covariance(pa, np.r_[pb[:3], 0, 0, 0, 0], Saa, Sab, Sbb, out=out)
        assert s == capi.BAD_ARG and np.array_equal(out, mark)


def test_helper_arithmetic_under_the_host_sanitizers(tmp_path, golden):
    """msfl_graph_relative_covariance's arithmetic (msfl_graph_host.h) as a stand-alone program built with -fsanitize=address,undefined,
    run on the CPU: what it prints equals the numpy value to 1e-12 of the largest entry, and its refusals leave `out` untouched."""
    exe = str(tmp_path / "graph_marginals_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "msf_loam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "graph_marginals_check.cpp"), "-o", exe])
    recs = _records(golden)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(recs)], np.int64).tobytes())
        for r in recs:
            f.write(np.concatenate([np.asarray(v, np.float64).ravel() for v in r]).tobytes())
    out = subprocess.run([exe, str(tmp_path / "in.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0 and "graph marginals ok" in out.stdout, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    for r, line in zip(recs, lines):
        got = np.array([float(v) for v in line.split()]).reshape(6, 6)
        want = gm.relative_covariance(*r)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
