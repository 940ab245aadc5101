"""GPU: the de-skew association (knn5_scan2map_kernel<true> + fit_scan2map_kernel<true>) record by record, through
msfl_associate_scan2map_deskew, against the model of tests/deskew_assoc_cases.py (the plain oracle's association of each feature
at its own composed pose, C' = C - shift, p' = dq p + dp in numpy f64).

Bars (none from what the kernels deliver):
  accept set      exactly the model's.  The issue that introduced this test allows up to 3 features per case within 1e-6 of a
                  threshold to differ; the seeds are chosen so that the model has no such feature
                  (tests/test_deskew_assoc_model.py: two compositions of the pose, zero flips), so none is allowed here
  {C', N}         within 1e-9, the bar of the plain records (tests/test_gpu_scan2map.py); line directions compared as stored
  p'              within 1e-12 m: about 30 f64 operations on magnitudes of at most 40 m, roughly 1.3e-13
  counting form   msfl_set_timing(h, 3) runs knn5_scan2map_kernel<true, true>: the same bytes as the timed form
  end to end      one outer iteration of msfl_match_scan2map_deskew equals msfl_associate_scan2map_deskew followed by
                  msfl_solve_records_deskew on its output, byte for byte in pose and info
"""
import numpy as np
import pytest

from tests import common
from tests import deskew_assoc_cases as da

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mapped(gpu):
    from msf_loam_amd import capi
    _, mc, ms = common.small_world()
    prm = capi.default_params()
    prm.outer_iterations = 1
    h = capi.Handle(0, prm)
    h.set_map(mc, ms)
    yield h
    h.close()


def _associate(h, x, pose):
    return h.associate_scan2map_deskew(x.corner, x.surf, x.corner_dq, x.corner_dp, x.surf_dq, x.surf_dp, x.V, da.G, pose)


@pytest.mark.parametrize("case", da.CASES, ids=da.case_id)
def test_deskew_association_matches_the_model_record_by_record(mapped, oracle, case):
    x = da.inputs(case)
    m = da.model(case, 0)
    nc = len(x.corner)
    rec, pts = _associate(mapped, x, x.truth)
    accepted = rec[:, 3:].any(axis=1)
    differ = np.flatnonzero(accepted != m.accepted)
    both = accepted & m.accepted
    d_c = np.abs(rec[both, :3] - m.rec[both, :3]).max()
    d_n = np.abs(rec[both, 3:] - m.rec[both, 3:]).max()
    d_p = np.abs(pts - m.points).max()
    print("deskew association %s: %d corner %d surf, accepted %d / %d (model %d / %d), decisions that differ %d, |C' - model| %.3e  |N - model| %.3e  |p' - model| %.3e"
          % (da.case_id(case), nc, len(x.surf), accepted[:nc].sum(), accepted[nc:].sum(), m.accepted[:nc].sum(), m.accepted[nc:].sum(),
             len(differ), d_c, d_n, d_p))
    assert rec.shape == m.rec.shape and pts.shape == m.points.shape
    assert len(differ) == 0, differ[:10]
    assert not rec[~accepted].any()                                          # a rejected feature is all zeros
    assert d_c <= 1e-9 and d_n <= 1e-9, (d_c, d_n)
    assert d_p <= 1e-12, d_p
    # the counting instantiation
    mapped.set_timing(3)
    try:
        rec_n, pts_n = _associate(mapped, x, x.truth)
        t = mapped.get_timing()
    finally:
        mapped.set_timing(0)
    assert t.knn_candidates > 0                                              # the counting form did run
    assert rec_n.tobytes() == rec.tobytes() and pts_n.tobytes() == pts.tobytes()


@pytest.mark.parametrize("case", da.CASES, ids=da.case_id)
def test_one_outer_iteration_equals_association_then_solve(mapped, oracle, case):
    x = da.inputs(case)
    h = mapped
    s, pose_m, info_m = h.match_scan2map_deskew(x.corner, x.surf, x.corner_dq, x.corner_dp, x.surf_dq, x.surf_dp, x.V, da.G, x.guess)
    rec, pts = _associate(h, x, x.guess)
    pose_s, info_s = h.solve_records_deskew(x.corner, x.surf, rec, pts, x.guess)
    n_edge = int(rec[:len(x.corner), 3:].any(axis=1).sum())
    print("deskew end to end %s: %d edges %d planes, iterations %d successful %d, same pose bytes %s, same info bytes %s"
          % (da.case_id(case), info_m.n_edge[0], info_m.n_plane[0], info_m.lm_iterations[0], info_m.lm_successful[0],
             pose_m.tobytes() == pose_s.tobytes(), bytes(info_m) == bytes(info_s)))
    assert s == 0 and info_m.status == 0 and info_m.lm_successful[0] >= 1
    assert info_m.n_edge[0] == n_edge > 1024                                 # past the solve's dense edge list
    assert pose_m.tobytes() == pose_s.tobytes()
    assert bytes(info_m) == bytes(info_s)
    assert not np.array_equal(pose_m, x.guess)
