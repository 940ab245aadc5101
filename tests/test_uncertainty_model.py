"""CPU: the numpy model of msfl_match_uncertainty (tests/uncertainty_numpy.py) on problems with known answers and on the
three synthetic worlds, and the plumbing of the C ABI (header, exports, ctypes record)."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc_mod
from tests import ceres_numpy as cn
from tests import common
from tests import uncertainty_numpy as un

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_EIG = 150.0      # between the corridor's lambda_0 (~40-50) and its lambda_1 (~310-380); room / outdoor: lambda_0 ~ 900-1 150


def _axis_planes(pose, axes, per_axis, seed):
    """Plane correspondences with unit normals along the given axes and ZERO residual at `pose` (so rho' = 1)."""
    rng = np.random.default_rng(seed)
    R, t = cn.quat_to_R(pose[3:7]), pose[:3]
    corr = np.zeros(per_axis * len(axes), dtype=orc_mod.CORR)
    k = 0
    for a in axes:
        for _ in range(per_axis):
            p = rng.uniform(-10, 10, 3)
            corr[k]["p"], corr[k]["C"], corr[k]["kind"] = p, R @ p + t, 2
            corr[k]["N"][a] = 1.0
            k += 1
    return corr


POSE = np.array([0.3, -0.2, 0.1, 0.02, -0.03, 0.05, 0.0])
POSE[6] = np.sqrt(1.0 - POSE[3:6] @ POSE[3:6])


def test_axis_planes_give_the_sum_of_normal_outer_products_exactly():
    corr = _axis_planes(POSE, (0, 1, 2), 7, 1)
    H, cost, m = un.information(corr, POSE)
    assert m == 21 and cost < 1e-25
    assert np.array_equal(H[:3, :3], np.diag([7.0, 7.0, 7.0]))
    assert np.array_equal(H, H.T)


def test_deleting_a_family_makes_exactly_one_direction_degenerate():
    corr = _axis_planes(POSE, (1, 2), 9, 2)              # no plane sees x
    rec = un.record(corr, POSE)
    H, cov = rec["information"], rec["covariance"]
    assert np.all(H[0] == 0.0) and np.all(H[:, 0] == 0.0)
    assert abs(rec["eigenvalues"][0]) <= 1e-12 * rec["eigenvalues"][5] and rec["eigenvalues"][1] > 1e-6 * rec["eigenvalues"][5]
    assert rec["n_degenerate"] == 1
    assert int(np.argmax(np.abs(rec["eigenvectors"][0]))) == 0 and rec["eigenvectors"][0][0] > 0.999999
    # the dropped direction is absent from the pseudo-inverse (to the rounding of the kept eigenvectors' x components)
    assert np.abs(cov[0]).max() <= 1e-12 * np.abs(cov).max() and np.abs(cov[:, 0]).max() <= 1e-12 * np.abs(cov).max()
    assert np.abs(H @ cov @ H - H).max() <= 1e-9 * np.abs(H).max()


def test_full_rank_covariance_is_the_inverse():
    corr = _axis_planes(POSE, (0, 1, 2), 12, 3)
    rec = un.record(corr, POSE)
    H, cov = rec["information"], rec["covariance"]
    assert rec["n_degenerate"] == 0
    assert np.abs(H @ cov @ H - H).max() <= 1e-9 * np.abs(H).max()
    assert np.abs(cov - np.linalg.inv(H)).max() <= 1e-9 * np.abs(cov).max()
    V = rec["eigenvectors"]
    assert np.abs(V @ V.T - np.eye(6)).max() <= 1e-12
    for k in range(6):
        assert V[k, int(np.argmax(np.abs(V[k])))] > 0


def test_sign_convention_takes_the_lowest_index_on_ties():
    rows = un.fix_signs([[-0.5, 0.5, 0, 0, 0, 0], [0.1, -0.9, 0, 0, 0, 0], [0.5, -0.5, 0, 0, 0, 0]])
    assert rows[0][0] == 0.5 and rows[0][1] == -0.5 and rows[1][1] == 0.9 and rows[2][0] == 0.5


def test_variance_factor_and_parent_frame():
    assert un.sigma2(3.0, 6) == 0.0 and un.sigma2(3.0, 9) == 2.0
    rng = np.random.default_rng(4)
    M = rng.normal(size=(6, 6))
    cov = M @ M.T
    out = un.covariance_in_parent_frame(POSE, cov, 2.5)
    R = cn.quat_to_R(POSE[3:7])
    assert np.allclose(out[:3, :3], 2.5 * cov[:3, :3], rtol=0, atol=1e-14 * np.abs(cov).max())
    assert np.allclose(out[3:, 3:], 2.5 * R @ cov[3:, 3:] @ R.T, rtol=1e-13)
    assert np.allclose(out[:3, 3:], 2.5 * cov[:3, 3:] @ R.T, rtol=1e-13)
    ident = np.array([0, 0, 0, 0, 0, 0, 1.0])
    assert np.array_equal(un.covariance_in_parent_frame(ident, cov, 1.0), cov)


@pytest.mark.parametrize("kind,expect_degenerate", [("room", 0), ("outdoor", 0), ("corridor", 1)])
def test_worlds_separate_by_one_eigenvalue(oracle, kind, expect_degenerate):
    _, mc, ms = common.other_world(kind)
    for pts, ring, truth, guess in common.other_scans(kind, 2):
        _, corner, surf = common.features_from_oracle(oracle, pts, ring)
        corr, pose, summ = un.oracle_last_problem(oracle, mc, ms, corner, surf, guess)
        rec = un.record(corr, pose, MIN_EIG)
        w = rec["eigenvalues"]
        print(kind, "eigenvalues", w, "cond", w[5] / w[0], "v0", rec["eigenvectors"][0])
        assert rec["n_degenerate"] == expect_degenerate, w
        assert w[5] / w[0] <= 1e4                                   # the GPU test's covariance tolerance rests on this
        assert abs(summ.final_cost - un.information(corr, pose)[1]) <= 1e-9 * summ.final_cost
        if kind == "corridor":
            assert int(np.argmax(np.abs(rec["eigenvectors"][0]))) == 0       # the weak direction is x-translation


def test_header_library_and_ctypes_record_agree():
    from msf_loam_amd import capi
    text = open(os.path.join(ROOT, "include", "msfl_c_api.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"typedef struct msfl_match_uncertainty \{(.*?)\} msfl_match_uncertainty;", code, flags=re.S)
    assert m, "the header does not declare msfl_match_uncertainty"
    fields = re.findall(r"\b(double|int)\s+(\w+)(?:\[(\d+)\])?\s*;", m.group(1))
    assert [(t, n, int(c or 1)) for t, n, c in fields] == [
        ("double", "information", 36), ("double", "eigenvalues", 6), ("double", "eigenvectors", 36), ("double", "covariance", 36),
        ("double", "sigma2", 1), ("int", "n_residuals", 1), ("int", "n_degenerate", 1), ("int", "valid", 1), ("int", "reserved_", 1)]
    assert [n for n, _ in capi.MatchUncertainty._fields_] == [n for _, n, _ in fields]
    assert ctypes.sizeof(capi.MatchUncertainty) == 936 and capi.UNCERTAINTY_DTYPE.itemsize == 936
    assert ctypes.sizeof(capi.SlamResult) == 496                      # msfl_slam_result is untouched: its size before this feature
    assert re.search(r"#define MSFL_API_VERSION 1\b", text)
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in ("msfl_set_uncertainty", "msfl_slam_set_uncertainty", "msfl_slam_get_uncertainty"):
        assert re.search(r"\bmsfl_status\s+" + name + r"\s*\(", code), name + " is not declared"
        assert hasattr(lib, name), "missing export: " + name
        assert name in capi.EXPORTED
