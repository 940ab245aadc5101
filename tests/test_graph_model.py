"""CPU: the pose-graph model (tests/graph_numpy.py) against itself and against its stored results
(tests/golden/graph_model_v1.npz, written by tests/golden/make_graph_golden.py).  No GPU, no reference."""
import os

import numpy as np
import pytest

from tests import graph_numpy as gn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERMINATION = ("empty", "gradient", "max_iterations", "min_radius", "invalid_steps", "parameter", "function")
SMALL = tuple(c for c in gn.CASES if c != "g")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "graph_model_v1.npz")))


class NoLoss(gn.Options):
    huber_delta = 0.0


@pytest.mark.parametrize("opt", (NoLoss, gn.Options))
def test_jacobians_against_central_differences(opt):
    """Analytic tangent Jacobian of every block of case (f) (Huber active on the wrong closure) and (h) against central differences
    through plus_poses, h = 1e-6: the truncation error is O(h^2 |J'''|) ~ 1e-9 relative, the rounding error eps |r| / h ~ 1e-8 of the
    largest residual row; the bound is 1e-6 of the largest Jacobian entry."""
    for name in ("f", "h"):
        prob = gn.make_case(name)
        ev, pl, x0, nt, _ = gn.dense_fns(prob)
        _, blk = gn.blocks(prob, prob["poses"], opt, False)
        # the corrector's scale is held at its value at x0: Ceres differentiates the residual, then scales
        s = np.concatenate([np.repeat(np.sqrt((b[0] ** 2).sum(-1)), b[0].shape[1]) for b in blk])
        _, r0, J = ev(None, x0, opt)
        _, raw0, _ = ev(None, x0, NoLoss)
        scale = np.divide(r0, raw0, out=np.ones_like(r0), where=raw0 != 0)
        h = 1e-6
        worst = 0.0
        for k in range(nt):
            d = np.zeros(nt); d[k] = h
            num = (ev(None, pl(x0, d), NoLoss)[1] - ev(None, pl(x0, -d), NoLoss)[1]) / (2 * h)
            worst = max(worst, float(np.abs(J[:, k] - scale * num).max()))
        assert s.shape == r0.shape
        assert worst <= 1e-6 * np.abs(J).max(), (name, worst)


@pytest.mark.parametrize("name", SMALL)
def test_dense_and_sparse_agree_and_match_the_golden_file(name, golden):
    prob = gn.make_case(name)
    for k in ("poses", "ez", "fp", "ei", "ej", "fi", "fj", "ft", "fixed"):
        assert np.array_equal(prob[k], golden["%s_%s" % (k, name)]), "the stored case is not what make_case builds"
    xd, td = gn.solve_dense(prob)
    xs, ts = gn.solve_sparse(prob)
    assert (td.termination, td.iterations, td.successful_steps, td.accepted) == (ts.termination, ts.iterations, ts.successful_steps, ts.accepted)
    d = gn.pose_distance(xd, xs)
    assert name == "f" or d <= 1e-6
    assert [TERMINATION.index(td.termination), td.iterations, td.successful_steps] == golden["tr_" + name].tolist()
    assert td.accepted == golden["acc_" + name].tolist()
    assert np.allclose([td.initial_cost, td.final_cost], golden["cost_" + name], rtol=1e-12, atol=0)
    assert gn.pose_distance(xd, golden["x_" + name]) <= max(1e-12, 10 * float(golden["d_" + name]))


def test_golden_file_holds_every_case_within_the_condition(golden):
    for name in gn.CASES:
        assert name == "f" or float(golden["d_" + name]) <= 1e-6
        assert golden["x_" + name].shape == golden["poses_" + name].shape
        assert len(golden["acc_" + name]) == int(golden["tr_" + name][1])
    assert gn.n_long(gn.make_case("c")) == 0 and gn.n_long(gn.make_case("e")) == 70
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "graph_model_v1.npz")) < 1 << 20


def test_fixed_nodes_stay_and_empty_problems_terminate_empty():
    prob = gn.make_case("b")
    x, tr = gn.solve_sparse(prob)
    assert np.array_equal(x[0], prob["poses"][0]) and tr.termination == "function"
    prob["fixed"][:] = True
    x, tr = gn.solve_dense(prob)
    assert tr.termination == "empty" and np.array_equal(x, prob["poses"])


def test_host_bookkeeping_under_the_host_sanitizers(tmp_path):
    """The adjacency lists, the long / chain classification and the reduction's level sizes for any N (msfl_graph_host.h): a
    stand-alone program built with -fsanitize=address,undefined, run on the CPU."""
    import subprocess
    exe = str(tmp_path / "graph_structure_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "msf_loam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "graph_structure_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0 and "graph structure ok" in out.stdout, out.stderr
