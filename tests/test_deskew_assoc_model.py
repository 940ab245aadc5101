"""CPU: the conditions tests/test_gpu_deskew_assoc.py puts on its own inputs (tests/deskew_assoc_cases.py).

  * the inverse distortion works: the model alone accepts at least half of the features of every case, and more than 1 024 corner
    features (the solve's dense edge list);
  * no accept decision hangs on rounding: the model evaluated with the per-feature pose composed in two ways (quaternion product
    against rotation matrices; they differ in the last bits) accepts the same set, with records within 1e-9 of each other.  A seed
    with a flip is replaced;
  * the strong motion is what the issue asks for: rotations to 0.3 rad, dp to 0.2 m, |V| = 15 m/s.
"""
import numpy as np
import pytest

from tests import deskew_assoc_cases as da


@pytest.mark.parametrize("case", da.CASES, ids=da.case_id)
def test_model_accepts_most_features_and_no_decision_hangs_on_rounding(oracle, case):
    x = da.inputs(case)
    nc, ns = len(x.corner), len(x.surf)
    a, b = da.model(case, 0), da.model(case, 1)
    share_c, share_s = a.accepted[:nc].mean(), a.accepted[nc:].mean()
    flips = int((a.accepted != b.accepted).sum())
    d_rec = np.abs(a.rec - b.rec).max()
    print("%s: %d corner %d surf features, accepted %.3f / %.3f, flips between the two compositions %d, records differ by %.3e"
          % (da.case_id(case), nc, ns, share_c, share_s, flips, d_rec))
    assert int(a.accepted[:nc].sum()) > 1024 and ns > 0                       # the edge count passes the solve's dense edge list
    assert a.accepted.mean() >= 0.5
    at_guess = da.model(case, 0, at="guess")                                  # where the end-to-end test starts
    print("%s at the guess: accepted %d corner %d surf" % (da.case_id(case), at_guess.accepted[:nc].sum(), at_guess.accepted[nc:].sum()))
    assert int(at_guess.accepted[:nc].sum()) > 1024 and at_guess.accepted.mean() >= 0.5
    assert flips == 0
    assert d_rec <= 1e-9
    assert np.array_equal(a.points, b.points)
    assert np.all(np.isfinite(x.corner)) and np.all(np.isfinite(x.surf))
    ang = 2 * np.arccos(np.clip(np.concatenate([x.corner_dq, x.surf_dq])[:, 3], -1, 1))
    dp = np.linalg.norm(np.concatenate([x.corner_dp, x.surf_dp]), axis=1)
    if case.motion == "strong":
        assert 0.25 < ang.max() <= 0.3 + 1e-12 and 0.15 < dp.max() <= 0.2 + 1e-3 and abs(np.linalg.norm(x.V) - 15.0) < 1e-12
    else:
        assert ang.max() <= 0.0301 and dp.max() <= 0.0065
