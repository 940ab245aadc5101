"""CPU: the numpy model of the degeneracy-aware solve (tests/degeneracy_numpy.py) and its case table.

What is asserted comes from the definition (docs/kernels/degeneracy.md), not from a run of the kernel:
  * with V = I and nothing held the model IS ceres_numpy.solve (exact equality; so it is for any V with nothing held, because
    a solve that holds nothing keeps the identity basis);
  * the tangent step of every candidate of a reduced solve has no component along a held eigenvector.  V is orthonormal to
    rounding only, so "zero" is |v_held . step| <= 1e-14 |step| here (a few ulps of a sum of six products of unit-size factors);
    for the axis case, whose held eigenvector is exactly e_x, it is exactly zero;
  * every case of the table keeps each eigenvalue of H0 a factor 2 away from its threshold, so that the held set is the same
    under any rounding;
  * the record mirror is 688 bytes.
"""
import ctypes as C

import numpy as np
import pytest

from tests import ceres_numpy as cn
from tests import degeneracy_numpy as dn


def _by_name(name):
    return next(c for c in dn.cases() if c.name == name)


def test_identity_basis_and_nothing_held_is_the_plain_solve():
    c = _by_name("nothing_held")
    x_ref, tr_ref = cn.solve(c.corr, c.guess)
    lam, V = dn.decompose(dn.entry_matrix(c.corr, c.guess)[2])
    for basis in (np.eye(6), V):
        x, tr = dn.solve(c.corr, c.guess, basis, 0)
        assert np.array_equal(x, x_ref)
        assert (tr.iterations, tr.successful_steps, tr.initial_cost, tr.final_cost) == \
               (tr_ref.iterations, tr_ref.successful_steps, tr_ref.initial_cost, tr_ref.final_cost)
        assert tr.cost == tr_ref.cost and tr.accepted == tr_ref.accepted


@pytest.mark.parametrize("name", ["axis", "two_held", "seam-ns831-nc0"])
def test_held_coordinates_of_every_step_are_zero(name):
    c = _by_name(name)
    lam, V = dn.decompose(dn.entry_matrix(c.corr, c.guess)[2])
    assert dn.classify(lam, c.min_eig) == c.n_held > 0
    steps = []
    x, tr = dn.solve(c.corr, c.guess, V, c.n_held, steps=steps)
    assert tr.successful_steps >= 1 and len(steps) >= tr.iterations
    for d in steps:
        for k in range(c.n_held):
            assert abs(V[k] @ d) <= 1e-14 * np.linalg.norm(d), (name, k)
    x_plain, _ = cn.solve(c.corr, c.guess)
    assert not np.array_equal(x, x_plain)
    if name == "axis":
        assert np.array_equal(V[0], [1, 0, 0, 0, 0, 0]) and lam[0] == 3.0          # an exact eigenpair, by construction
        assert all(d[0] == 0.0 for d in steps) and x[0] == c.guess[0]
        assert abs(x_plain[0] - c.guess[0]) > 1e-3                                 # the plain solve follows the weak rows


def test_all_held_is_no_step():
    c = _by_name("all_held")
    assert c.n_held == 6
    x, tr = dn.solve(c.corr, c.guess, np.eye(6), 6)
    assert tr is None and np.array_equal(x, c.guess)


def test_every_case_keeps_its_eigenvalues_a_factor_two_from_the_threshold():
    names = {c.name for c in dn.cases()}
    assert {"axis", "two_held", "nothing_held", "all_held"} <= names and sum(n.startswith("seam-") for n in names) >= 4
    for c in dn.cases():
        lam = np.linalg.eigvalsh(dn.entry_matrix(c.corr, c.guess)[2])
        m = dn.margin(lam, c.min_eig)
        print(dn.case_id(c), "n_held", c.n_held, "margin %.2f" % m)
        assert m >= 2.0, (dn.case_id(c), m)
        assert dn.classify(lam, c.min_eig) == c.n_held
    assert _by_name("two_held").n_held == 2 and _by_name("axis").n_held == 1 and _by_name("nothing_held").n_held == 0


def test_classification_rule():
    lam = np.array([0.0, 1e-3, 5.0, 5.0, 7.0, 100.0])
    assert dn.classify(lam, 5.0) == 2                    # strictly below: an eigenvalue AT the threshold is kept
    assert dn.classify(lam, 0.0) == 1                    # the relative floor 1e-14 * lambda_max holds an exact zero only
    big = np.array([0.0, 1e-3, 5.0, 5.0, 7.0, 1e15])     # the floor is 10 here and overrides a smaller min_eigenvalue
    assert dn.threshold(big, 5.0) == 10.0 and dn.classify(big, 5.0) == 5


def test_record_mirror_size():
    from msf_loam_amd import capi
    assert C.sizeof(capi.DegeneracyRecord) == 688
    assert capi.DEGENERACY_DTYPE.itemsize == 688
