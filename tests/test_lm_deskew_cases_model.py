"""CPU: what tests/test_gpu_lm_deskew.py takes for granted about its own case table (tests/lm_deskew_cases.py).

The GPU file compares the de-skew branch of the solve kernels (points read as f64 p' from global memory, no plane cache, an edge
loop of its own) with two references at chosen row counts.  That only means something if, for every case,
  * the two references agree with each other far below the GPU tolerance (the oracle's final cost against the numpy evaluation
    at the oracle's pose: 1e-12 relative) and the solve takes a successful step, so that a later pass produces final_cost;
  * reading the WRONG POINTS is visible: evaluating the model with f32(p) -- what the staged clouds hold -- in place of p' moves
    H or the cost by at least 1e-6 relative (p' is decimetres to metres from p, so this moves them by percents and more);
  * one missing or doubled row is visible: removing a single accepted row changes H = J^T J by exactly J_i^T J_i and counting it
    twice by exactly the same amount with the other sign, at least 1e-6 of max|H|, 1 000 x the GPU tolerance on H.  The sampled
    rows are every ceil(n / 20)-th accepted row plus the rows at the seams (BLOCK, edge list, the plain branch's cache, last rows).
A seed that falls under a floor is replaced, the floors stay.  The sibling problems also assert the margin of their threshold
rejection (every squared residual at least rejection_numpy.MARGIN relative from the cut), a condition on the inputs.
"""
import numpy as np
import pytest

from tests import ceres_numpy as cn
from tests import lm_deskew_cases as ld
from tests import rejection_numpy as rn
from tests.test_lm_boundary_cases_model import _row_slices

SOLVED = [c for c in ld.CASES if not ld.is_void(c)] + [ld.SIBLINGS[b] for b in ld.BLOCKS]


@pytest.mark.parametrize("case", SOLVED, ids=ld.case_id)
def test_references_agree_and_wrong_points_or_rows_would_show(oracle, case):
    p = ld.problem(case.k)
    pose_o, summ = ld.oracle_solution(case.k)
    cost, r, J = cn.evaluate(p.corr, np.asarray(pose_o), cn.Options)
    rel = abs(summ.final_cost - cost) / cost
    assert summ.successful_steps >= 1, (case, summ.iterations, summ.successful_steps)
    start, n_rows = _row_slices(p.corr)
    assert len(r) == start[-1]
    H = J.T @ J
    scale = np.abs(H).max()
    # the cloud's f32 points in place of p'
    cost_c, _, J_c = cn.evaluate(ld.with_cloud_points(p), np.asarray(pose_o), cn.Options)
    d_points = max(np.abs(J_c.T @ J_c - H).max() / scale, abs(cost_c - cost) / cost)
    # the original points really are somewhere else, and p' is not an f32 point
    moved = np.linalg.norm(p.points - np.concatenate([p.corner[:, :3], p.surf[:, :3]]), axis=1)
    assert moved.max() <= 20 * np.sqrt(3) * ld.MAX_ANGLE + np.sqrt(3) * ld.MAX_SHIFT + 1e-5
    assert np.any(p.points != p.points.astype(np.float32))
    # one row dropped (H - J_i^T J_i) or doubled (H + J_i^T J_i)
    acc = p.accepted
    step = -(-len(acc) // 20)
    rows = sorted(set(acc[::step].tolist()) | (set(ld.seam_rows(case)) & set(acc.tolist())))
    floor = min(np.abs(J[start[i]:start[i] + n_rows[i]].T @ J[start[i]:start[i] + n_rows[i]]).max() / scale for i in rows)
    print("%s: iterations %d successful %d  cost rel %.3e  cloud points instead of p': %.3e  %d rows sampled, least |dH| / max|H| %.3e"
          % (ld.case_id(case), summ.iterations, summ.successful_steps, rel, d_points, len(rows), floor))
    assert rel <= 1e-12, (case, rel)
    assert d_points >= 1e-6, (case, d_points)
    assert floor >= 1e-6, (case, floor)


@pytest.mark.parametrize("block", ld.BLOCKS)
def test_sibling_problems_keep_their_rejection_margin(block):
    p = ld.problem(ld.SIBLINGS[block].k)
    m = rn.margin(p.corr, np.asarray(p.guess), rn.THRESHOLD, threshold=rn.SEAM_THRESHOLD)
    mask, want = rn.decide(p.corr, np.asarray(p.guess), rn.THRESHOLD, threshold=rn.SEAM_THRESHOLD)
    print("sibling problem, %d threads: rejection margin %.3e, %d of %d rows rejected" % (block, m, int(mask.sum()), len(mask)))
    assert m >= rn.MARGIN, (block, m)
    assert 0 < int(mask.sum()) < len(mask)
    assert want["n_edge_rejected"] > 0 and want["n_plane_rejected"] > 0
    # rows survive on both sides of the edge list and of the plain branch's plane cache
    keep = np.flatnonzero(~mask)
    nc, cache = ld.SIBLINGS[block].nc, ld.CACHE[block]
    assert (keep < ld.EDGE_LIST_MAX).any() and ((keep >= ld.EDGE_LIST_MAX) & (keep < nc)).any()
    assert ((keep >= nc) & (keep < nc + cache)).any() and (keep >= nc + cache).any()


def test_the_table_is_the_issue_s():
    for block in ld.BLOCKS:
        cache = ld.CACHE[block]
        mine = [c for c in ld.CASES if c.block == block]
        assert {c.nc for c in mine if c.pattern == "none" and c.ns == 300} == \
            {1, 31, 32, 33, block - 1, block, block + 1, 1023, 1024, 1025, 1536, 2600}
        planes = {(c.ns, c.nc) for c in mine if c.pattern == "none" and c.ns != 300}
        assert planes == {(1, 40), (block - 1, 40 if block - 1 < 200 else 0), (block, 40 if block < 200 else 0),
                          (block + 1, 40 if block + 1 < 200 else 0), (cache - 1, 0), (cache, 0), (cache + 1, 0),
                          (cache + ld.GROUP[block] * block + 1, 0)}
        assert {c.pattern for c in mine} == set(ld.PATTERNS) | {"none"}
        assert (ld.SIBLINGS[block].ns, ld.SIBLINGS[block].nc) == (cache + 200, 1100)
    for c in ld.CASES:
        if ld.is_void(c):
            p = ld.problem(c.k)
            assert len(p.accepted) == 0 and not p.rec.any()
