"""GPU: the DE-SKEW branch of the LM solve, rejection and uncertainty kernels (evaluate_pass<BLOCK, FILL> with pprime != nullptr,
msfl_kernels.cuh) at its structural seams, at both solve workgroups, through msfl_solve_records_deskew on handles created under
MSFL_SOLVE_RECORDS_BLOCK.

That branch is other code than the plain one tests/test_gpu_lm_boundaries.py pins: an edge loop of its own (`k += BLOCK` over the
dense list of kEdgeListMax = 1 024 entries plus the checked tail, no grouped loads), the plain plane loop (`i += BLOCK`) with no
LDS cache, and the points read as f64 p' from global memory.  The case table is tests/lm_deskew_cases.py: every row has a motion
of its own (up to 0.3 rad, 0.2 m), the records are generated from p' and the staged clouds carry the ORIGINAL points, so a kernel
that reads the cloud, or a cache of f32 points, is off by decimetres.  tests/test_lm_deskew_cases_model.py asserts on the CPU that
such a fault, and one row dropped or doubled, moves H or the costs by >= 1e-6 relative.

Bars (those of tests/test_gpu_lm_boundaries.py; none comes from what the kernels deliver):
  counts          info.n_edge / n_plane equal the accepted rows exactly; n_residuals = 3 n_edge + n_plane
  information     against tests/uncertainty_numpy.information AT THE POSE THE GPU RETURNED, max-norm <= 1e-9 * max|H|
  costs           initial_cost (numpy cost at the guess) and final_cost (numpy cost at the returned pose), 1e-9 relative
  trajectory      lm_iterations / lm_successful equal oracle.ceres_solve's, >= 1 successful step, pose within 1e-6 of it
  decomposition   _check_eigen of tests/test_gpu_uncertainty.py on the record
  nothing accepted / no rows      pose bit-identical, uncertainty record all zero bytes, status 0
Relations:
  (a) the clouds' xyz are not an input: other finite values there leave pose, info and every record byte-identical, plain and
      with prior + rejection + uncertainty on
  (b) with points = f64(cloud xyz) the entry agrees with msfl_solve_records in counts and iteration counts and in pose within
      1e-9 (not bit-equal: the later passes sum in different orders)
Siblings, one problem per width (CACHE + 200 planes, 1 100 edges), with the bars of their own GPU tests:
  lm_solve_prior_kernel against tests/prior_numpy.solve; threshold rejection against tests/rejection_numpy (bitwise equal to the
  solve on the model's survivors); lm_solve_degen_kernel against tests/degeneracy_numpy.
"""
import numpy as np
import pytest

from msf_loam_amd import synth
from tests import ceres_numpy as cn
from tests import degeneracy_numpy as dn
from tests import lm_boundary_cases as lb
from tests import lm_deskew_cases as ld
from tests import prior_numpy as pn
from tests import rejection_numpy as rn
from tests import uncertainty_numpy as un
from tests.test_gpu_degeneracy import _check_decomposition, _compare_solve
from tests.test_gpu_rejection import _check_record, _slice_is_zero
from tests.test_gpu_uncertainty import _check_eigen, _is_zero

pytestmark = pytest.mark.gpu

PLAIN = [c for c in ld.CASES if not ld.is_void(c)]
VOID = [c for c in ld.CASES if ld.is_void(c)]
TIGHT = 1e-7


@pytest.fixture(scope="module")
def handles(gpu):
    """One fresh handle per solve workgroup (the knob is read when the handle is created), each with a one-record host sink."""
    from msf_loam_amd import capi
    hs = {}
    for block in ld.BLOCKS:
        with pytest.MonkeyPatch.context() as monkeypatch:
            monkeypatch.setenv("MSFL_SOLVE_RECORDS_BLOCK", str(block))
            hs[block] = capi.Handle(0)
        hs[block].set_uncertainty(1)
    yield hs
    for h in hs.values():
        h.close()


def _rel(a, b):
    return abs(a - b) / abs(b)


def _solve(h, p, corner=None, surf=None, rec=None):
    pose, info = h.solve_records_deskew(p.corner if corner is None else corner, p.surf if surf is None else surf,
                                        p.rec if rec is None else rec, p.points, p.guess)
    return pose, info, h.uncertainty(1)[0]


def _prior_of(k):
    """(mean pose, sqrt information): full rank, mean a few centimetres off the truth (lm_boundary_cases.prior_of's recipe)."""
    rng = np.random.default_rng(lb.PRIOR_SEED + 500 + k)
    mean = synth.perturb_pose(np.array(ld.problem(k).truth), rng, max_t=0.05, max_deg=0.5)
    return mean, pn.random_spd_sqrt(rng)


def _check_counts(p, info, u):
    kinds = p.corr["kind"]
    assert info.status == 0
    assert info.n_edge[0] == int((kinds == 1).sum()) and info.n_plane[0] == int((kinds == 2).sum()), (info.n_edge[0], info.n_plane[0])
    assert u["n_residuals"] == 3 * info.n_edge[0] + info.n_plane[0]
    assert u["sigma2"] == un.sigma2(info.final_cost[0], int(u["n_residuals"])) and u["reserved_"] == 0


@pytest.mark.parametrize("case", PLAIN, ids=ld.case_id)
def test_deskew_seam_sizes_and_rejected_rows_match_both_references(handles, oracle, case):
    p = ld.problem(case.k)
    pose_o, summ = ld.oracle_solution(case.k)
    pose_g, info, u = _solve(handles[case.block], p)
    H, cost_f, m = un.information(p.corr, pose_g)
    cost_i = cn.evaluate(p.corr, np.asarray(p.guess), cn.Options, want_jacobian=False)[0]
    d_h = np.abs(u["information"] - H).max() / np.abs(H).max()
    d_i, d_f = _rel(info.initial_cost[0], cost_i), _rel(info.final_cost[0], cost_f)
    dt, dr = synth.pose_error(pose_g, pose_o)
    print("deskew width %d ns %d nc %d pattern %s: H rel %.3e  initial cost rel %.3e  final cost rel %.3e  iterations %d/%d successful %d/%d  pose %.3e m %.3e rad"
          % (case.block, case.ns, case.nc, case.pattern, d_h, d_i, d_f, info.lm_iterations[0], summ.iterations,
             info.lm_successful[0], summ.successful_steps, dt, dr))
    _check_counts(p, info, u)
    assert m == u["n_residuals"]
    assert d_h <= 1e-9, d_h
    assert d_i <= 1e-9 and d_f <= 1e-9, (d_i, d_f)
    assert info.lm_successful[0] >= 1                                        # else final_cost is the first pass's sum again
    assert info.lm_iterations[0] == summ.iterations and info.lm_successful[0] == summ.successful_steps
    assert dt < 1e-6 and dr < 1e-6, (dt, dr)
    _check_eigen(u, ld.case_id(case))


@pytest.mark.parametrize("case", VOID, ids=ld.case_id)
def test_nothing_to_solve_leaves_pose_and_a_zero_record(handles, case):
    h = handles[case.block]
    _, _, before = _solve(h, ld.problem(0))                                  # the sink now holds a record: zeros below are written, not left over
    assert not _is_zero(before)
    p = ld.problem(case.k)
    pose_g, info, u = _solve(h, p)
    print("deskew width %d ns %d nc %d pattern %s: pose kept, record zero" % (case.block, case.ns, case.nc, case.pattern))
    assert np.array_equal(pose_g, p.guess) and pose_g.tobytes() == np.asarray(p.guess).tobytes()
    assert _is_zero(u)
    assert info.status == 0 and info.n_edge[0] == 0 and info.n_plane[0] == 0 and info.lm_iterations[0] == 0


# ---- relations -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("options", ["plain", "prior_rejection_uncertainty"])
@pytest.mark.parametrize("block", ld.BLOCKS)
def test_the_clouds_xyz_are_not_an_input(handles, block, options):
    h = handles[block]
    k = ld.SIBLINGS[block].k
    p = ld.problem(k)
    rng = np.random.default_rng(9000 + block)
    other_c, other_s = np.array(p.corner), np.array(p.surf)
    other_c[:, :3] = rng.uniform(-50, 50, (len(other_c), 3)).astype(np.float32)
    other_s[:, :3] = rng.uniform(-50, 50, (len(other_s), 3)).astype(np.float32)
    assert not np.array_equal(other_c, p.corner) and not np.array_equal(other_s, p.surf)
    on = options != "plain"
    if on:
        prior = _prior_of(k)
        h.set_pose_prior([prior[0]], [prior[1]])
        h.set_outlier_rejection(threshold=rn.SEAM_THRESHOLD, n=1)
    try:
        out = []
        for corner, surf in ((p.corner, p.surf), (other_c, other_s)):
            pose, info, u = _solve(h, p, corner, surf)
            out.append((pose.tobytes(), bytes(info), u.tobytes(), h.rejection(1)[0].tobytes() if on else b""))
            assert info.status == 0 and info.lm_successful[0] >= 1 and not _is_zero(u)
            if on:
                r = h.rejection(1)[0]
                assert r["valid"][0] == 1 and 0 < r["n_edge_rejected"][0] + r["n_plane_rejected"][0] < len(p.accepted)
    finally:
        if on:
            h.clear_outlier_rejection()
            h.clear_pose_prior()
    print("deskew width %d, %s: other cloud xyz, same bytes: %s" % (block, options, out[0] == out[1]))
    assert out[0] == out[1]


@pytest.mark.parametrize("block", lb.BLOCKS)
def test_points_equal_to_the_cloud_agree_with_the_plain_entry(handles, block):
    h = handles[block]
    p = lb.problem(lb.WIDTH_PAIR.k)                                          # 3 500 planes, 1 100 edges; records made from the f32 points
    points = np.concatenate([p.corner[:, :3], p.surf[:, :3]]).astype(np.float64)
    pose_a, info_a = h.solve_records(p.corner, p.surf, p.rec, p.guess)
    u_a = h.uncertainty(1)[0]
    pose_b, info_b = h.solve_records_deskew(p.corner, p.surf, p.rec, points, p.guess)
    u_b = h.uncertainty(1)[0]
    dt, dr = synth.pose_error(pose_a, pose_b)
    d_h = np.abs(u_a["information"] - u_b["information"]).max() / np.abs(u_a["information"]).max()
    print("width %d, plain entry vs deskew entry on the cloud's points: pose %.3e m %.3e rad  H rel %.3e  final cost rel %.3e  iterations %d/%d"
          % (block, dt, dr, d_h, _rel(info_b.final_cost[0], info_a.final_cost[0]), info_a.lm_iterations[0], info_b.lm_iterations[0]))
    assert info_a.status == 0 and info_b.status == 0
    assert (info_a.n_edge[0], info_a.n_plane[0]) == (info_b.n_edge[0], info_b.n_plane[0]) == (1100, 3500)
    assert (info_a.lm_iterations[0], info_a.lm_successful[0]) == (info_b.lm_iterations[0], info_b.lm_successful[0]) and info_b.lm_successful[0] >= 1
    assert u_a["n_residuals"] == u_b["n_residuals"]
    assert dt < 1e-9 and dr < 1e-9, (dt, dr)


# ---- the sibling kernels ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("block", ld.BLOCKS)
def test_prior_kernel_on_deskew_points(handles, block):
    h = handles[block]
    case = ld.SIBLINGS[block]
    p = ld.problem(case.k)
    prior = _prior_of(case.k)
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
    print("deskew width %d ns %d nc %d prior: H rel %.3e  initial cost rel %.3e  final cost rel %.3e  iterations %d/%d successful %d/%d  pose %.3e m %.3e rad"
          % (block, case.ns, case.nc, d_h, d_i, d_f, info.lm_iterations[0], tr.iterations, info.lm_successful[0], tr.successful_steps, dt, dr))
    kinds = p.corr["kind"]
    assert info.status == 0 and info.n_edge[0] == int((kinds == 1).sum()) and info.n_plane[0] == int((kinds == 2).sum())
    assert u["n_residuals"] == m + 6, (u["n_residuals"], m)                  # the prior's six rows count (docs/kernels/prior.md)
    assert info.lm_iterations[0] == tr.iterations and info.lm_successful[0] == tr.successful_steps and info.lm_successful[0] >= 1
    assert d_i <= 1e-9 and d_f <= 1e-9, (d_i, d_f)
    assert dt < 1e-6 and dr < 1e-6, (dt, dr)
    assert d_h <= 1e-9, d_h
    _check_eigen(u, ld.case_id(case))


@pytest.mark.parametrize("block", ld.BLOCKS)
def test_threshold_rejection_on_deskew_points(handles, block):
    """The bars of tests/test_gpu_rejection.py's fixed records: the solve with rejection on equals, bitwise, the solve with the
    feature off on the records with the model's mask zeroed; counts exact; cut_sq within 1e-12 relative."""
    h = handles[block]
    p = ld.problem(ld.SIBLINGS[block].k)
    what = "deskew sibling, %d threads" % block
    mask, want = rn.decide(p.corr, np.asarray(p.guess), rn.THRESHOLD, threshold=rn.SEAM_THRESHOLD)
    pose_ref, info_ref, _ = _solve(h, p, rec=rn.zeroed(p.rec, mask))
    h.set_outlier_rejection(threshold=rn.SEAM_THRESHOLD, n=1)
    try:
        pose_on, info_on, _ = _solve(h, p)
        r = h.rejection(1)[0]
    finally:
        h.clear_outlier_rejection()
    _check_record(r, 0, want, what)
    assert _slice_is_zero(r, 1), what                                        # one solve
    assert np.array_equal(pose_on, pose_ref) and bytes(info_on) == bytes(info_ref), what
    assert info_on.n_edge[0] == want["n_edge_in"] - want["n_edge_rejected"] and info_on.n_plane[0] == want["n_plane_in"] - want["n_plane_rejected"]
    assert info_on.lm_successful[0] >= 1
    pose_off, info_off, _ = _solve(h, p)
    assert mask.any() and not (np.array_equal(pose_on, pose_off) and bytes(info_on) == bytes(info_off)), what
    # the model's decision with the cloud's points in place of p' is another one: a rejection kernel reading the cloud would show
    mask_c, _ = rn.decide(ld.with_cloud_points(p), np.asarray(p.guess), rn.THRESHOLD, threshold=rn.SEAM_THRESHOLD)
    assert not np.array_equal(mask_c, mask)


@pytest.mark.parametrize("block", ld.BLOCKS)
def test_degeneracy_kernel_on_deskew_points(handles, block):
    h = handles[block]
    case = ld.SIBLINGS[block]
    p = ld.problem(case.k)
    what = "deskew sibling, %d threads" % block
    guess = np.asarray(p.guess)
    cost0, _, H0 = dn.entry_matrix(p.corr, guess)
    thr, n_below = dn.gap_threshold(np.linalg.eigvalsh(H0))
    h.set_degeneracy(thr, 1)
    try:
        pose_g, info, _ = _solve(h, p)
        d = h.degeneracy(1)[0]
    finally:
        h.clear_degeneracy()
    assert d["valid"][0] == 1 and d["valid"][1] == 0 and d["n_held"][1] == 0
    lam, V = d["eigenvalues"][0], d["eigenvectors"][0]
    lam_np = _check_decomposition(lam, V, H0, what)
    assert dn.margin(lam_np, thr) >= 2.0, (lam_np, thr)                      # a condition on the inputs
    assert d["n_held"][0] == dn.classify(lam_np, thr) == n_below and 0 < n_below < 6
    pose_n, tr = dn.solve(p.corr, guess, V, int(d["n_held"][0]))
    dt, dr = _compare_solve(pose_g, info, 0, pose_n, tr, what)
    assert dt <= TIGHT and dr <= TIGHT, (what, dt, dr)
    assert info.n_edge[0] == case.nc and info.n_plane[0] == case.ns
    pose_off, _, _ = _solve(h, p)
    assert not np.array_equal(pose_g, pose_off)
