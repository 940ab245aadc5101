"""CPU: the numpy specification of outlier rejection (tests/rejection_numpy.py) and its case table, checked against themselves:
the record mirror's size, the rejected count against the reference's loop written literally, the tie and non-finite rules, every
case's margin, and that the moved-object input is meaningful (rejection makes the solve land 10 x closer to the truth)."""
import ctypes as C

import numpy as np
import pytest

from msf_loam_amd import synth
from tests import ceres_numpy as cn
from tests import lm_boundary_cases as lb
from tests import rejection_numpy as rn


def test_record_mirror_is_56_bytes():
    from msf_loam_amd import capi
    assert capi.REJECTION_DTYPE.itemsize == C.sizeof(capi.RejectionRecord) == 56
    assert [capi.REJECTION_DTYPE.fields[f][1] for f in ("n_edge_in", "n_plane_in", "n_edge_rejected", "n_plane_rejected", "cut_sq", "valid")] == \
        [0, 8, 16, 24, 32, 48]
    assert "msfl_set_outlier_rejection" in capi.EXPORTED and "msfl_slam_get_rejection" in capi.EXPORTED


def _reference_loop(n, frac):
    """RefineByRejectOutliersWithFrac (scan_matcher.cc:66): `for (size_t i = 0; i < n * frac; i++)` removes one block per trip."""
    i = 0
    while i < n * frac:
        i += 1
    return i


def test_rejected_count_is_the_reference_loop():
    for frac in (0.0, 0.07, 0.15, 0.3, 0.5, 1.0):
        for n in range(4001):
            assert rn.reject_count(n, frac) == _reference_loop(n, frac), (n, frac)
    assert rn.reject_count(100, 0.07) == 8                        # 100 * 0.07 = 7.000000000000001: a known answer


def test_ties_go_by_the_higher_index_and_non_finite_ranks_on_top():
    c = rn.case_by_name("tie")
    valid, s = rn.residual_sq(c.corr, c.guess)
    mask, rec = rn.decide(c.corr, c.guess, c.mode, fraction=c.fraction)
    dup = np.flatnonzero(s == rec["cut_sq"])
    assert len(dup) == 4 and len({rn.key_of(v) for v in s[dup]}) == 1
    assert list(mask[dup]) == [False, False, True, True]          # ascending index: the last two go
    assert mask.sum() == 12 and np.all(s[mask] >= rec["cut_sq"]) and np.all(s[valid & ~mask] <= rec["cut_sq"])
    for name in ("non_finite_threshold", "non_finite_fraction"):
        c = rn.case_by_name(name)
        valid, s = rn.residual_sq(c.corr, c.guess)
        bad = np.flatnonzero(valid & ~np.isfinite(s))
        assert len(bad) == 2 and np.isnan(s[bad]).any() and np.isinf(s[bad]).any()
        mask, rec = rn.decide(c.corr, c.guess, c.mode, threshold=c.threshold, fraction=c.fraction)
        assert mask[bad].all() and np.isfinite(rec["cut_sq"])
        if c.mode == rn.FRACTION:
            assert mask.sum() == 3 and rec["cut_sq"] == np.max(s[valid & np.isfinite(s)])


def test_low_bits_case_makes_every_radix_pass_decide():
    c = rn.case_by_name("low_bits")
    valid, s = rn.residual_sq(c.corr, c.guess)
    mask, rec = rn.decide(c.corr, c.guess, c.mode, fraction=c.fraction)
    around = np.flatnonzero(valid & (np.abs(s - 0.49) < 1e-6))
    keys = [rn.key_of(v) for v in s[around]]
    assert len(around) == 40 and len(set(keys)) == 40
    assert len({k >> 24 for k in keys}) == 1                      # the upper 40 bits are shared ...
    assert len({k >> 8 for k in keys}) < 40                       # ... and some keys only differ in the last byte
    assert mask.sum() == 30 and mask[around].sum() == 20          # the cut runs through the middle of them
    assert sorted(keys)[20] == rn.key_of(rec["cut_sq"])


@pytest.mark.parametrize("c", rn.cases(), ids=lambda c: c.name)
def test_every_case_meets_its_margin(c):
    valid, s = rn.residual_sq(c.corr, c.guess)
    mask, rec = rn.decide(c.corr, c.guess, c.mode, threshold=c.threshold, fraction=c.fraction)
    m = rn.margin(c.corr, c.guess, c.mode, threshold=c.threshold, fraction=c.fraction)
    print(c.name, "rows", len(c.corr), "valid", int(valid.sum()), "rejected", int(mask.sum()), "margin %.3e" % m, rec)
    assert (c.corr["kind"] == 0).any() and np.all(c.rec[c.corr["kind"] == 0] == 0)       # refused records are interleaved
    assert rec["n_edge_in"] + rec["n_plane_in"] == int(valid.sum())
    assert rec["n_edge_rejected"] + rec["n_plane_rejected"] == int(mask.sum()) == c.n_rejected
    if c.mode == rn.FRACTION:
        assert int(mask.sum()) == rn.reject_count(int(valid.sum()), c.fraction)
    if not c.exact:
        assert m >= rn.MARGIN, (c.name, m)
    if c.name == "moved_object":
        fin = s[valid]
        thr2 = c.threshold ** 2
        assert np.all((fin <= thr2 / 4) | (fin >= 4 * thr2)) and mask.sum() == 21
        assert rec["n_edge_rejected"] == 6 and rec["n_plane_rejected"] == 15 and rec["n_edge_in"] == 46 and rec["n_plane_in"] == 135
    if c.name == "fraction_n100_f007":
        assert mask.sum() == 8
    if c.name == "fraction_zero":
        assert not mask.any() and rec["cut_sq"] == 0.0
    if c.name == "fraction_one":
        assert np.array_equal(mask, valid)


@pytest.mark.parametrize("c", rn.seam_cases(), ids=rn.seam_case_id)
def test_seam_cases_meet_their_margin(c):
    p = lb.problem(c.k)
    mask, rec = rn.decide(p.corr, p.guess, rn.THRESHOLD, threshold=rn.SEAM_THRESHOLD)
    m = rn.margin(p.corr, p.guess, rn.THRESHOLD, threshold=rn.SEAM_THRESHOLD)
    print(rn.seam_case_id(c), "rejected", int(mask.sum()), "of", len(p.corr), "margin %.3e" % m)
    assert m >= rn.MARGIN and 0 < mask.sum() < len(p.corr)


def test_seam_cases_cover_both_seams_at_both_widths():
    got = {(c.block, c.ns, c.nc) for c in rn.seam_cases()}
    for block in lb.BLOCKS:
        for d in (-1, 0, 1):
            assert (block, lb.CACHE[block] + d, 0) in got and (block, 300, lb.EDGE_LIST_MAX + d) in got


def test_moved_object_rejection_brings_the_solve_ten_times_closer():
    c = rn.case_by_name("moved_object")
    mask, _ = rn.decide(c.corr, c.guess, c.mode, threshold=c.threshold)
    kept = np.array(c.corr)
    kept["kind"][mask] = 0
    x_all, _ = cn.solve(np.array(c.corr), np.array(c.guess))
    x_kept, _ = cn.solve(kept, np.array(c.guess))
    e_all, e_kept = synth.pose_error(x_all, c.truth), synth.pose_error(x_kept, c.truth)
    print("moved object: error to the truth with all rows %.3e m %.3e rad, with the survivors %.3e m %.3e rad" % (e_all + e_kept))
    assert e_all[0] >= 10 * e_kept[0] and e_all[1] >= 10 * e_kept[1]
