"""CPU: the model of the pose graph with information-weighted factors (tests/graph_info_numpy.py) against itself, against its stored
results (tests/golden/graph_info_model_v1.npz, written by tests/golden/make_graph_info_golden.py) and against graph_numpy where the
two must agree; and the host helpers msfl_graph_edge_from_uncertainty / msfl_graph_fix_from_covariance through the library (they touch
no GPU) and as a stand-alone program under the host sanitizers.  No GPU, no reference."""
import os
import subprocess

import numpy as np
import pytest

from tests import graph_info_numpy as gi
from tests import graph_numpy as gn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERMINATION = ("empty", "gradient", "max_iterations", "min_radius", "invalid_steps", "parameter", "function")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "graph_info_model_v1.npz")))


class NoLoss(gi.Options):
    huber_delta = 0.0


@pytest.mark.parametrize("opt", (NoLoss, gi.Options))
def test_jacobians_against_central_differences(opt):
    """Analytic tangent Jacobian of every block of (iii) (all four kinds, ranks 4 and 6) and (v) (Huber active on the wrong closure)
    against central differences through plus_poses, h = 1e-6; bound and reasoning of tests/test_graph_model.py: truncation
    O(h^2 |J'''|) ~ 1e-9 relative, rounding eps |r| / h ~ 1e-8 of the largest residual row; 1e-6 of the largest Jacobian entry."""
    for name in ("iii", "v"):
        prob = gi.make_case(name)
        ev, pl, x0, nt, _ = gi.dense_fns(prob)
        _, r0, J = ev(None, x0, opt)
        _, raw0, _ = ev(None, x0, NoLoss)
        # the corrector's scale is held at its value at x0: Ceres differentiates the residual, then scales
        scale = np.divide(r0, raw0, out=np.ones_like(r0), where=raw0 != 0)
        assert name != "v" or opt is NoLoss or scale.min() < 0.5          # Huber is active in (v)
        h = 1e-6
        worst = 0.0
        for k in range(nt):
            d = np.zeros(nt); d[k] = h
            num = (ev(None, pl(x0, d), NoLoss)[1] - ev(None, pl(x0, -d), NoLoss)[1]) / (2 * h)
            worst = max(worst, float(np.abs(J[:, k] - scale * num).max()))
        print("case %s: largest difference %.3g on entries up to %.3g" % (name, worst, np.abs(J).max()))
        assert worst <= 1e-6 * np.abs(J).max(), (name, worst)


@pytest.mark.parametrize("name", gi.CASES)
def test_dense_and_sparse_agree_and_match_the_golden_file(name, golden):
    prob = gi.make_case(name)
    for k in gi.KEYS:
        assert np.array_equal(prob[k], golden["%s_%s" % (k, name)]), "the stored case is not what make_case builds"
    xd, td = gi.solve_dense(prob)
    xs, ts = gi.solve_sparse(prob)
    assert (td.termination, td.iterations, td.successful_steps, td.accepted) == (ts.termination, ts.iterations, ts.successful_steps, ts.accepted)
    assert gn.pose_distance(xd, xs) <= 1e-6
    assert [TERMINATION.index(td.termination), td.iterations, td.successful_steps] == golden["tr_" + name].tolist()
    assert td.accepted == golden["acc_" + name].tolist()
    assert np.allclose([td.initial_cost, td.final_cost], golden["cost_" + name], rtol=1e-12, atol=0)
    assert gn.pose_distance(xd, golden["x_" + name]) <= max(1e-12, 10 * float(golden["d_" + name]))


def test_golden_file_holds_every_case_within_the_condition(golden):
    for name in gi.CASES:
        assert float(golden["d_" + name]) <= 1e-6
        assert golden["x_" + name].shape == golden["poses_" + name].shape
        assert len(golden["acc_" + name]) == int(golden["tr_" + name][1])
    iii = gi.make_case("iii")
    n_plain = len(iii["ei"]) + len(iii["fi"])
    assert len(iii["ei"]) > 64 and len(iii["gi"]) > 64 and n_plain % 64 != 0 and len(iii["fi"]) == len(iii["hi"]) == 2
    assert sorted(np.linalg.matrix_rank(L) for L in iii["gL"][-4:]) == [4, 4, 6, 6]
    i = gi.make_case("i")
    assert len(i["ei"]) == len(i["fi"]) == 0 and not i["fixed"].any()
    ii = gi.make_case("ii")
    assert [np.linalg.matrix_rank(L) for L in ii["gL"]] == [6, 5] and gi.n_long(ii) == 2
    assert gi.n_long(gi.make_case("v")) == 4 and golden["tr_v"].tolist()[0] == TERMINATION.index("max_iterations")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "graph_info_model_v1.npz")) < 1 << 20


def test_isotropic_information_edges_cost_what_plain_edges_cost():
    """Case (d) of graph_numpy against the same graph with every edge rewritten as an information edge with
    L = diag(1/st x 3, 1/(2 sr) x 3): the old residual is T_ij^-1 Z, the new one Z^-1 T_ij, whose norms agree.  1e-10 relative, at the
    start and at the solved poses: room for the rounding of 141 blocks and nothing else (a single edge gives ~1e-13)."""
    prob = gn.make_case("d")
    info = gi.edges_as_info(prob)
    assert len(info["ei"]) == 0 and len(info["gi"]) == len(prob["ei"]) == 137
    solved = dict(np.load(os.path.join(ROOT, "tests", "golden", "graph_model_v1.npz")))["x_d"]
    for x in (prob["poses"], solved):
        for opt in (gi.Options, NoLoss):
            a, b = gn.cost(prob, x, opt), gi.cost(info, x, opt)
            print("plain %.15g information %.15g relative difference %.3g" % (a, b, abs(a - b) / a))
            assert abs(a - b) <= 1e-10 * a
        assert np.allclose(gi.chi2(info, x)[2], gi.chi2(gi.with_info(prob), x)[0], rtol=1e-9, atol=1e-18)


def test_corridor_rank_deficient_closures_beat_isotropic_ones(golden):
    """Three closures that slid 2 m along the corridor axis: weighted isotropically they pull the trajectory along; with the row of the
    unobservable direction zeroed they still correct the rest."""
    odometry, plain, isotropic, rank5 = golden["ate_iv"]
    truth = golden["truth_iv"]
    assert [gi.ate(golden["x_iv_" + f], truth) for f in gi.CORRIDOR_FORMS] == [plain, isotropic, rank5]
    assert gi.ate(golden["poses_iv_rank5"], truth) == odometry
    print("corridor ATE: odometry %.3f, plain %.3f, isotropic %.3f, rank 5 %.3f" % (odometry, plain, isotropic, rank5))
    assert rank5 < odometry
    assert plain > 5 * rank5 and isotropic > 5 * rank5
    for f in gi.CORRIDOR_FORMS:                         # the zero row is the corridor axis, in the frame the measurement lives in
        prob = {k: golden["%s_iv_%s" % (k, f)] for k in gi.KEYS}
        assert gi.n_long(prob) == 3
    L = golden["gL_iv_rank5"]
    for k, (i, j) in enumerate(gi.CORRIDOR_PAIRS):
        axis = gn.quat_to_R(truth[i, 3:]).T @ [1.0, 0.0, 0.0]
        assert np.linalg.matrix_rank(L[k]) == 5 and np.abs(L[k] @ np.r_[axis, 0, 0, 0]).max() <= 1e-12 * np.abs(L[k]).max()


def test_wrong_closure_has_the_largest_chi_square(golden):
    prob = gi.make_case("v")
    for x in (prob["poses"], golden["x_v"]):
        c = gi.chi2(prob, x)[2]
        assert int(np.argmax(c)) == 2


# ---- the helpers, through the library (no GPU call behind them) --------------------------------------------------------------

def _unit(rng):
    q = rng.normal(0.0, 1.0, 4)
    return q / np.linalg.norm(q)


def _record(rng, n_degenerate, flip=False):
    from msf_loam_amd import capi
    A = rng.normal(0.0, 1.0, (6, 6))
    H = A @ np.diag(10.0 ** rng.uniform(0, 4, 6)) @ A.T
    H = 0.5 * (H + H.T)
    lam, V = np.linalg.eigh(H)
    u = np.zeros(1, capi.UNCERTAINTY_DTYPE)
    u["information"][0], u["eigenvalues"][0], u["eigenvectors"][0] = H, lam, (-V.T if flip else V.T)
    u["n_degenerate"], u["valid"], u["sigma2"], u["n_residuals"] = n_degenerate, 1, 0.7, 100
    return H, u


@pytest.mark.parametrize("n_degenerate", (0, 1, 3))
def test_edge_from_uncertainty_equals_the_formula(n_degenerate):
    from msf_loam_amd import capi
    rng = np.random.default_rng(50 + n_degenerate)
    for _ in range(20):
        H, u = _record(rng, n_degenerate)
        pose_i, pose_j = np.r_[rng.normal(0, 10, 3), _unit(rng)], np.r_[rng.normal(0, 10, 3), _unit(rng)]
        scale = float(rng.uniform(0.1, 3.0))
        s, rec = capi.edge_from_uncertainty(4, 9, pose_i, pose_j, u[0], scale)
        assert s == capi.OK and (rec["i"][0], rec["j"][0]) == (4, 9)
        z, want = gi.edge_from_uncertainty(pose_i, pose_j, H, n_degenerate, scale)
        L = rec["sqrt_information"][0]
        assert np.abs(L.T @ L - want).max() <= 1e-12 * np.abs(H).max() / scale
        assert np.all(L[:n_degenerate] == 0.0) and np.linalg.matrix_rank(L) == 6 - n_degenerate
        # two roundings of the same formula on coordinates up to ~40 m
        assert np.abs(rec["z"][0] - gn.relative_pose(pose_i, pose_j)).max() <= 5e-14 and np.array_equal(gn.relative_pose(pose_i, pose_j), z)
        # negating every eigenvector changes nothing in L^T L
        u2 = u.copy(); u2["eigenvectors"] *= -1.0
        s2, rec2 = capi.edge_from_uncertainty(4, 9, pose_i, pose_j, u2[0], scale)
        L2 = rec2["sqrt_information"][0]
        assert s2 == capi.OK and np.array_equal(L2, -L) and np.array_equal(L2.T @ L2, L.T @ L)
    # identity pose_i: the record is about the relative pose itself
    s, rec = capi.edge_from_uncertainty(0, 1, [0, 0, 0, 0, 0, 0, 1.0], pose_j, u[0], 1.0)
    assert s == capi.OK and np.array_equal(rec["z"][0], pose_j)
    lam, V = u["eigenvalues"][0], u["eigenvectors"][0]
    assert np.allclose(rec["sqrt_information"][0][n_degenerate:], np.sqrt(lam[n_degenerate:])[:, None] * V[n_degenerate:], rtol=1e-15, atol=0)


def test_fix_from_covariance_inverts_to_the_covariance():
    from msf_loam_amd import capi
    """Sigmas of 1 .. 5 cm per axis, as a GPS receiver's (vertical several times worse than horizontal): condition <= 25, some 20
    operations per entry at eps 1.1e-16 give 6e-14 relative, inside the 1e-12."""
    rng = np.random.default_rng(60)
    for _ in range(50):
        cov = gi._gps_cov(rng, rng.uniform(0.01, 0.05, 3))
        cov = 0.5 * (cov + cov.T)
        s, rec = capi.fix_from_covariance(3, 4, 0.25, [1.0, 2.0, 3.0], cov)
        L3 = rec["sqrt_information"][0]
        assert s == capi.OK and (rec["i"][0], rec["j"][0], rec["t"][0]) == (3, 4, 0.25) and rec["p"][0].tolist() == [1.0, 2.0, 3.0]
        assert np.all(np.tril(L3, -1) == 0.0) and np.all(np.diag(L3) > 0.0)
        assert np.abs(np.linalg.inv(L3.T @ L3) - cov).max() <= 1e-12 * np.abs(cov).max()
        assert np.abs((L3.T @ L3) @ cov - np.eye(3)).max() <= 1e-12
        assert np.allclose(L3, gi.fix_from_covariance(cov), rtol=1e-10, atol=1e-12 * np.abs(L3).max())


def test_helper_refusals_leave_the_record_untouched():
    from msf_loam_amd import capi
    rng = np.random.default_rng(70)
    H, u = _record(rng, 1)
    pose_i, pose_j = np.r_[rng.normal(0, 10, 3), _unit(rng)], np.r_[rng.normal(0, 10, 3), _unit(rng)]
    mark = np.frombuffer(bytes(range(1, 177)) * 2, np.uint8)

    def edge(i=0, j=1, pi=pose_i, pj=pose_j, rec=u, scale=1.0, **field):
        r = rec.copy()
        for k, v in field.items():
            r[k] = v
        out = np.zeros(1, capi.GRAPH_EDGE_INFO_DTYPE)
        out.view(np.uint8)[:] = mark
        s, _ = capi.edge_from_uncertainty(i, j, pi, pj, r[0], scale, out=out)
        assert s != capi.BAD_ARG or np.array_equal(out.view(np.uint8), mark), "a refusal wrote to *out"
        return s

    assert edge() == capi.OK
    assert edge(valid=0) == capi.BAD_ARG
    assert edge(n_degenerate=6) == capi.BAD_ARG and edge(n_degenerate=7) == capi.BAD_ARG and edge(n_degenerate=-1) == capi.BAD_ARG
    assert edge(i=2, j=2) == capi.BAD_ARG
    for bad in (np.nan, np.inf, -np.inf):
        assert edge(scale=bad) == capi.BAD_ARG
        assert edge(pi=np.r_[bad, pose_i[1:]]) == capi.BAD_ARG and edge(pj=np.r_[pose_j[:6], bad]) == capi.BAD_ARG
        lam = u["eigenvalues"].copy(); lam[0, 3] = bad
        V = u["eigenvectors"].copy(); V[0, 2, 2] = bad
        assert edge(eigenvalues=lam) == capi.BAD_ARG and edge(eigenvectors=V) == capi.BAD_ARG
    assert edge(scale=0.0) == capi.BAD_ARG and edge(scale=-1.0) == capi.BAD_ARG
    assert edge(pi=np.r_[pose_i[:3], 0, 0, 0, 0]) == capi.BAD_ARG and edge(pj=np.r_[pose_j[:3], 0, 0, 0, 0]) == capi.BAD_ARG

    fmark = np.frombuffer(bytes(range(1, 113)), np.uint8)
    cov = gi._gps_cov(rng, [0.01, 0.02, 0.05])
    cov = 0.5 * (cov + cov.T)

    def fix(i=0, j=1, t=0.5, p=(1.0, 2.0, 3.0), c=cov):
        out = np.zeros(1, capi.GRAPH_FIX_INFO_DTYPE)
        out.view(np.uint8)[:] = fmark
        s, _ = capi.fix_from_covariance(i, j, t, p, c, out=out)
        assert s != capi.BAD_ARG or np.array_equal(out.view(np.uint8), fmark), "a refusal wrote to *out"
        return s

    assert fix() == capi.OK
    asym = cov.copy(); asym[0, 1] += 1e-3 * cov[0, 0]
    indef = cov - 2.0 * np.linalg.eigvalsh(cov)[1] * np.eye(3)
    for c in (asym, indef, -cov, np.zeros((3, 3)), np.ones((3, 3)), np.where(np.eye(3) > 0, np.nan, cov), np.where(np.eye(3) > 0, np.inf, cov)):
        assert fix(c=c) == capi.BAD_ARG
    assert fix(i=1, j=1) == capi.BAD_ARG and fix(t=-0.1) == capi.BAD_ARG and fix(t=1.1) == capi.BAD_ARG and fix(t=np.nan) == capi.BAD_ARG
    assert fix(p=(np.nan, 0, 0)) == capi.BAD_ARG


def test_helper_arithmetic_under_the_host_sanitizers(tmp_path):
    """The arithmetic of both helpers (msfl_graph_host.h): a stand-alone program built with -fsanitize=address,undefined, run on the CPU."""
    exe = str(tmp_path / "graph_info_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "msf_loam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "graph_info_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0 and "graph info ok" in out.stdout, out.stderr
