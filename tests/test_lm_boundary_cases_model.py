"""CPU: what tests/test_gpu_lm_boundaries.py takes for granted about its own case table (tests/lm_boundary_cases.py).

The GPU file compares the solve kernels with two references at chosen row counts.  That only means something if
  * the two references agree with each other far below the GPU tolerance (the oracle's final cost against the numpy
    evaluation at the oracle's pose: 1e-12 relative, three orders under the GPU's 1e-9; measured <= 5e-14),
  * every case takes a successful step, so that a pass other than the first one produces final_cost,
  * one missing row is visible: removing a single accepted row moves H by at least 1e-6 of max|H|, 1 000 x the GPU
    tolerance on H (measured minimum 2.5e-6; typical 4e-5 .. 1e-3).  A seed that falls under the floor is replaced, the
    floor stays.
The sampled rows are every ceil(n / 20)-th accepted row plus the rows at the seams (plane cache, edge list, last rows).
Removing row i from the stacked Jacobian J changes H = J^T J by exactly J_i^T J_i, which is what is measured here.
"""
import numpy as np
import pytest

from tests import ceres_numpy as cn
from tests import lm_boundary_cases as lb

SOLVED = [c for c in lb.CASES if not lb.is_void(c)] + [lb.WIDTH_PAIR]


def _row_slices(corr):
    """Rows of the stacked Jacobian that record i owns (3 per edge, 1 per plane, none when rejected)."""
    n_rows = np.where(corr["kind"] == 1, 3, np.where(corr["kind"] == 2, 1, 0))
    start = np.concatenate([[0], np.cumsum(n_rows)])
    return start, n_rows


@pytest.mark.parametrize("case", SOLVED, ids=lb.case_id)
def test_references_agree_and_every_row_counts(oracle, case):
    p = lb.problem(case.k)
    pose_o, summ = lb.oracle_solution(case.k)
    cost, r, J = cn.evaluate(p.corr, np.asarray(pose_o), cn.Options)
    rel = abs(summ.final_cost - cost) / cost
    assert summ.successful_steps >= 1, (case, summ.iterations, summ.successful_steps)
    start, n_rows = _row_slices(p.corr)
    assert len(r) == start[-1]
    H = J.T @ J
    scale = np.abs(H).max()
    acc = p.accepted
    step = -(-len(acc) // 20)
    rows = sorted(set(acc[::step].tolist()) | (set(lb.seam_rows(case)) & set(acc.tolist())))
    floor = min(np.abs(J[start[i]:start[i] + n_rows[i]].T @ J[start[i]:start[i] + n_rows[i]]).max() / scale for i in rows)
    print("%s: iterations %d successful %d  cost rel %.3e  %d rows sampled, least |dH| / max|H| %.3e"
          % (lb.case_id(case), summ.iterations, summ.successful_steps, rel, len(rows), floor))
    assert rel <= 1e-12, (case, rel)
    assert floor >= 1e-6, (case, floor)


def test_void_cases_have_no_accepted_row_and_the_table_is_the_issue_s():
    for c in lb.CASES:
        p = lb.problem(c.k) if lb.is_void(c) else None
        if p is not None:
            assert len(p.accepted) == 0 and not p.rec.any()
    # every pattern at both widths, the prior form at cache -+ 1 and one past the edge list
    for block in lb.BLOCKS:
        assert {c.pattern for c in lb.CASES if c.block == block} == set(lb.PATTERNS) | {"none"}
        assert {(c.ns, c.nc) for c in lb.CASES if c.block == block and c.prior} == \
            {(lb.CACHE[block] - 1, 0), (lb.CACHE[block] + 1, 0), (300, lb.EDGE_LIST_MAX + 1)}
    # the seam patterns reject / keep exactly rows cache - 2 .. cache + 1
    for c in lb.CASES:
        cache = lb.CACHE[c.block]
        kinds = lb.problem(c.k).corr["kind"] if c.pattern.startswith("plane_seam") else None
        if c.pattern == "plane_seam_rejected":
            assert np.flatnonzero(kinds == 0).tolist() == list(range(cache - 2, cache + 2))
        if c.pattern == "plane_seam_only":
            assert np.flatnonzero(kinds[cache - 32:cache + 32] != 0).tolist() == [30, 31, 32, 33] and kinds[:cache - 32].all() and kinds[cache + 32:].all()
