"""GPU: the LM solve and uncertainty kernels at the structural limits of evaluate_pass<BLOCK, FILL> (msfl_kernels.cuh), at both
solve workgroups: 128 threads (kLmBlock, every batched site) and 512 threads (kSlamLmBlock, the SLAM step's scan-to-map solve,
reached on fixed records through MSFL_SOLVE_RECORDS_BLOCK=512).

The case table is tests/lm_boundary_cases.py: row counts on both sides of the LDS plane cache (832 / 3 072 rows), of the dense
edge list (1 024 entries behind a 32 x 32-bit mask, a checked tail after it) and of the grouped, index-clamped loads (8 / 4
plane trips, 4 / 1 edge trips), and rejected records (kind 0, N = C = 0) placed at those seams.  A row dropped, read from the
wrong cache slot or counted twice there moves the pose by microns; it moves H and the costs by >= 1e-6 relative
(tests/test_lm_boundary_cases_model.py asserts that floor on the CPU), so the checks are on H and the costs:

  counts          info.n_edge / n_plane equal the accepted rows exactly; n_residuals = 3 n_edge + n_plane
  information     against tests/uncertainty_numpy.information (explicit stacked Jacobian) AT THE POSE THE GPU RETURNED, max-norm
                  <= 1e-9 * max|H| (the bar of tests/test_gpu_uncertainty.py): the FILL walk of the uncertainty kernel
  initial_cost    against the numpy cost at the guess, 1e-9 relative: the FILL walk of the solve kernel
  final_cost      against the numpy cost at the returned pose, 1e-9 relative: a later pass (cached head, edge list, tail,
                  streamed rest), the only output of that order -- so every case must take a successful step
  trajectory      lm_iterations / lm_successful equal oracle.ceres_solve's, pose within 1e-6 of it
  decomposition   _check_eigen of tests/test_gpu_uncertainty.py on the record
  nothing accepted / no rows      pose bit-identical, uncertainty record all zero bytes, status 0
  prior form      lm_solve_prior_kernel against tests/prior_numpy.solve: equal counts, costs 1e-9 relative, pose 1e-6; posterior
                  information = lidar H + Jp^T Jp within 1e-9
  both widths     one problem (3 500 planes, 1 100 edges): equal counts (the oracle's), poses within 1e-9 of each other; not
                  bit-equal, the two widths sum in different orders by design

None of the bars comes from what the kernels deliver.  The de-skew branch of evaluate_pass (pprime != nullptr: no plane cache, an
edge loop of its own, f64 points) is held to the same bars by tests/test_gpu_lm_deskew.py through msfl_solve_records_deskew.
"""
import numpy as np
import pytest

from msf_loam_amd import synth
from tests import ceres_numpy as cn
from tests import lm_boundary_cases as lb
from tests import prior_numpy as pn
from tests import uncertainty_numpy as un
from tests.test_gpu_uncertainty import _check_eigen, _is_zero

pytestmark = pytest.mark.gpu

PLAIN = [c for c in lb.CASES if not c.prior and not lb.is_void(c)]
VOID = [c for c in lb.CASES if lb.is_void(c)]
PRIOR = [c for c in lb.CASES if c.prior]


@pytest.fixture(scope="module")
def handles(gpu):
    """One fresh handle per solve workgroup (the knob is read when the handle is created), each with a one-record host sink."""
    from msf_loam_amd import capi
    hs = {}
    for block in lb.BLOCKS:
        with pytest.MonkeyPatch.context() as monkeypatch:
            monkeypatch.setenv("MSFL_SOLVE_RECORDS_BLOCK", str(block))
            hs[block] = capi.Handle(0)
        hs[block].set_uncertainty(1)
    yield hs
    for h in hs.values():
        h.close()


def _rel(a, b):
    return abs(a - b) / abs(b)


def _solve(h, p):
    pose, info = h.solve_records(p.corner, p.surf, p.rec, p.guess)
    return pose, info, h.uncertainty(1)[0]


def _check_counts(p, info, u):
    kinds = p.corr["kind"]
    assert info.status == 0
    assert info.n_edge[0] == int((kinds == 1).sum()) and info.n_plane[0] == int((kinds == 2).sum()), (info.n_edge[0], info.n_plane[0])
    assert u["n_residuals"] == 3 * info.n_edge[0] + info.n_plane[0]
    assert u["sigma2"] == un.sigma2(info.final_cost[0], int(u["n_residuals"])) and u["reserved_"] == 0


@pytest.mark.parametrize("case", PLAIN, ids=lb.case_id)
def test_seam_sizes_and_rejected_rows_match_both_references(handles, oracle, case):
    p = lb.problem(case.k)
    pose_o, summ = lb.oracle_solution(case.k)
    pose_g, info, u = _solve(handles[case.block], p)
    H, cost_f, m = un.information(p.corr, pose_g)
    cost_i = cn.evaluate(p.corr, np.asarray(p.guess), cn.Options, want_jacobian=False)[0]
    d_h = np.abs(u["information"] - H).max() / np.abs(H).max()
    d_i, d_f = _rel(info.initial_cost[0], cost_i), _rel(info.final_cost[0], cost_f)
    dt, dr = synth.pose_error(pose_g, pose_o)
    print("width %d ns %d nc %d pattern %s: H rel %.3e  initial cost rel %.3e  final cost rel %.3e  iterations %d/%d successful %d/%d  pose %.3e m %.3e rad"
          % (case.block, case.ns, case.nc, case.pattern, d_h, d_i, d_f, info.lm_iterations[0], summ.iterations,
             info.lm_successful[0], summ.successful_steps, dt, dr))
    _check_counts(p, info, u)
    assert m == u["n_residuals"]
    assert d_h <= 1e-9, d_h
    assert d_i <= 1e-9 and d_f <= 1e-9, (d_i, d_f)
    assert info.lm_successful[0] >= 1                                        # else final_cost is the first pass's sum again
    assert info.lm_iterations[0] == summ.iterations and info.lm_successful[0] == summ.successful_steps
    assert dt < 1e-6 and dr < 1e-6, (dt, dr)
    _check_eigen(u, lb.case_id(case))


@pytest.mark.parametrize("case", VOID, ids=lb.case_id)
def test_nothing_to_solve_leaves_pose_and_a_zero_record(handles, case):
    h = handles[case.block]
    _, _, before = _solve(h, lb.problem(0))                                  # the sink now holds a record: zeros below are written, not left over
    assert not _is_zero(before)
    p = lb.problem(case.k)
    pose_g, info, u = _solve(h, p)
    print("width %d ns %d nc %d pattern %s: pose kept, record zero" % (case.block, case.ns, case.nc, case.pattern))
    assert np.array_equal(pose_g, p.guess) and pose_g.tobytes() == np.asarray(p.guess).tobytes()
    assert _is_zero(u)
    assert info.status == 0 and info.n_edge[0] == 0 and info.n_plane[0] == 0 and info.lm_iterations[0] == 0


@pytest.mark.parametrize("case", PRIOR, ids=lb.case_id)
def test_prior_kernel_at_the_cache_seam_and_past_the_edge_list(handles, case):
    h = handles[case.block]
    p = lb.problem(case.k)
    prior = lb.prior_of(case.k)
    h.set_pose_prior([prior[0]], [prior[1]])
    try:
        pose_g, info, u = _solve(h, p)
    finally:
        h.clear_pose_prior()
    pose_n, tr = pn.solve(p.corr, np.asarray(p.guess), prior)
    H, _, m = un.information(p.corr, pose_g)
    Jp = pn.prior_rows(pose_g, prior)[2]
    d_h = np.abs(u["information"] - Jp.T @ Jp - H).max() / np.abs(H).max()
    d_i, d_f = _rel(info.initial_cost[0], tr.initial_cost), _rel(info.final_cost[0], tr.final_cost)
    dt, dr = synth.pose_error(pose_g, pose_n)
    print("width %d ns %d nc %d pattern prior: H rel %.3e  initial cost rel %.3e  final cost rel %.3e  iterations %d/%d successful %d/%d  pose %.3e m %.3e rad"
          % (case.block, case.ns, case.nc, d_h, d_i, d_f, info.lm_iterations[0], tr.iterations, info.lm_successful[0],
             tr.successful_steps, dt, dr))
    kinds = p.corr["kind"]
    assert info.status == 0 and info.n_edge[0] == int((kinds == 1).sum()) and info.n_plane[0] == int((kinds == 2).sum())
    assert u["n_residuals"] == m + 6, (u["n_residuals"], m)                  # the prior's six rows count (docs/kernels/prior.md)
    assert info.lm_iterations[0] == tr.iterations and info.lm_successful[0] == tr.successful_steps and info.lm_successful[0] >= 1
    assert d_i <= 1e-9 and d_f <= 1e-9, (d_i, d_f)
    assert dt < 1e-6 and dr < 1e-6, (dt, dr)
    assert d_h <= 1e-9, d_h
    _check_eigen(u, lb.case_id(case))


def test_one_problem_at_both_widths(handles, oracle):
    c = lb.WIDTH_PAIR
    p = lb.problem(c.k)
    pose_o, summ = lb.oracle_solution(c.k)
    got = {}
    for block in lb.BLOCKS:
        pose_g, info, u = _solve(handles[block], p)
        H, cost_f, _ = un.information(p.corr, pose_g)
        d_h = np.abs(u["information"] - H).max() / np.abs(H).max()
        d_f = _rel(info.final_cost[0], cost_f)
        print("width %d ns %d nc %d pattern both_widths: H rel %.3e  final cost rel %.3e  iterations %d successful %d"
              % (block, c.ns, c.nc, d_h, d_f, info.lm_iterations[0], info.lm_successful[0]))
        _check_counts(p, info, u)
        assert d_h <= 1e-9 and d_f <= 1e-9, (block, d_h, d_f)
        assert info.lm_iterations[0] == summ.iterations and info.lm_successful[0] == summ.successful_steps, block
        dt, dr = synth.pose_error(pose_g, pose_o)
        assert dt < 1e-6 and dr < 1e-6, (block, dt, dr)
        got[block] = (pose_g, info, u)
    (pa, ia, ua), (pb, ib, ub) = got[128], got[512]
    dt, dr = synth.pose_error(pa, pb)
    print("128 vs 512: pose %.3e m %.3e rad" % (dt, dr))
    assert dt < 1e-9 and dr < 1e-9, (dt, dr)
    # the widths partition the same 4 600 rows differently, so their sums differ in the last bits: equal bytes everywhere would
    # mean the knob never reached the 512-thread kernels
    assert (ua["information"].tobytes(), ia.initial_cost[0], ia.final_cost[0]) != (ub["information"].tobytes(), ib.initial_cost[0], ib.final_cost[0])
