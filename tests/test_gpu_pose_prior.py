"""GPU: the optional Gaussian pose prior (msfl_set_pose_prior / msfl_slam_set_next_prior) against the independent numpy
model (tests/prior_numpy.py + the trust-region loop of tests/ceres_numpy.py) and against itself across the call paths.

The reference has no prior on its lidar problems, so there is no reference output to compare with.

Bars (from the issue that introduced the feature; none comes from what the kernel happens to deliver):
  pose            <= 1e-7 m / rad against the numpy solve, lm_iterations / lm_successful exact, final_cost relative <= 1e-9: what
                  tests/test_gpu_scan2map.py holds the lidar-only solve to
  information     posterior minus Jp^T Jp against the numpy lidar H, max-norm <= 1e-9 * max|H| (tests/test_gpu_uncertainty.py)
  everything "equals" / "bit-identical"   byte comparison
"""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from msf_loam_amd import synth
from tests import ceres_numpy as cn
from tests import common
from tests import prior_numpy as pn
from tests import uncertainty_numpy as un

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIGHT = 1e-7
MIN_EIG = 150.0
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])
CORR_DTYPE = [("kind", np.int32), ("p", np.float64, 3), ("C", np.float64, 3), ("N", np.float64, 3)]
_cache = {}


def _rp():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import replay_synthetic as rp
    return rp


def _corr_from_records(corner, surf, rec):
    """The correspondences ceres_numpy wants from {C, N} records in feature order (corner first; all-zero = rejected)."""
    pts = np.concatenate([np.asarray(corner, np.float32).reshape(-1, 4), np.asarray(surf, np.float32).reshape(-1, 4)])
    corr = np.zeros(len(pts), CORR_DTYPE)
    ok = np.any(rec[:, 3:] != 0, axis=1)
    corr["kind"] = np.where(ok, np.where(np.arange(len(pts)) < len(corner), 1, 2), 0)
    corr["p"] = pts[:, :3].astype(np.float64)
    corr["C"] = rec[:, :3]
    corr["N"] = rec[:, 3:]
    return corr


def _fixed_sets(oracle):
    """The record sets of test_solver_matches_oracle_on_fixed_records (three room scans, oracle association at the guess), thinned
    to a few hundred accepted rows each so that the numpy loop stays quick: (corner, surf, records, corr, truth, guess)."""
    if "fixed" not in _cache:
        _, mc, ms = common.small_world()
        sets = []
        for pts, ring, truth, guess in common.scans(3):
            _, corner, surf = common.features_from_oracle(oracle, pts, ring)
            corr = oracle.associate_scan2map(mc, ms, corner, surf, guess, use_kdtree=True).copy()
            acc = np.flatnonzero(corr["kind"] != 0)
            drop = np.setdiff1d(acc, acc[::max(1, len(acc) // 300)])
            corr["kind"][drop] = 0
            rec = np.zeros((len(corr), 6))
            ok = corr["kind"] != 0
            rec[ok, :3] = corr["C"][ok]
            rec[ok, 3:] = corr["N"][ok]
            assert 250 <= ok.sum() <= 700 and (corr["kind"] == 1).sum() >= 10 and (corr["kind"] == 2).sum() >= 100
            sets.append((corner, surf, rec, corr, truth, guess))
        _cache["fixed"] = sets
    return _cache["fixed"]


def _priors_for(i, truth):
    """A full-rank random SPD prior and a rank-3 translation-only one, both with a mean a few centimetres off the truth."""
    rng = np.random.default_rng(500 + i)
    mean = synth.perturb_pose(truth, rng, max_t=0.05, max_deg=0.5)
    return [("spd", (mean, pn.random_spd_sqrt(rng))), ("translation", (mean, pn.translation_only_sqrt(0.05)))]


def _le_norm(pose, prior):
    return float(np.linalg.norm(pn.prior_rows(pose, prior)[1]))


def _batch64(oracle):
    if "batch64" not in _cache:
        cs, ss, guesses, truths = [], [], [], []
        for pts, ring, truth, guess in common.scans(64):
            _, corner, surf = common.features_from_oracle(oracle, pts, ring)
            cs.append(corner); ss.append(surf); guesses.append(guess); truths.append(truth)
        co = np.cumsum([0] + [len(c) for c in cs]).astype(np.int32)
        so = np.cumsum([0] + [len(s) for s in ss]).astype(np.int32)
        _cache["batch64"] = (cs, ss, np.concatenate(cs), co, np.concatenate(ss), so, np.array(guesses), np.array(truths))
    return _cache["batch64"]


def _real_priors(truths, seed=900):
    rng = np.random.default_rng(seed)
    means = np.array([synth.perturb_pose(t, rng, max_t=0.05, max_deg=0.5) for t in truths])
    Ls = np.array([pn.random_spd_sqrt(rng) if b % 4 else pn.translation_only_sqrt(0.05) for b in range(len(truths))])
    return means, Ls


# ---- 1. fixed records ------------------------------------------------------------------------------------------------

def test_fixed_records_solve_matches_the_numpy_solve(gpu, oracle):
    from msf_loam_amd import capi
    h = capi.Handle(0)
    for i, (corner, surf, rec, corr, truth, guess) in enumerate(_fixed_sets(oracle)):
        h.clear_pose_prior()
        pose_plain, info_plain = h.solve_records(corner, surf, rec, guess)
        for name, prior in _priors_for(i, truth):
            h.set_pose_prior([prior[0]], [prior[1]])
            pose_g, info = h.solve_records(corner, surf, rec, guess)
            pose_n, tr = pn.solve(corr, guess, prior)
            dt, dr = synth.pose_error(pose_g, pose_n)
            rel_i = abs(info.initial_cost[0] - tr.initial_cost) / tr.initial_cost
            rel_f = abs(info.final_cost[0] - tr.final_cost) / tr.final_cost
            print("fixed %d %s: dt %.3e dr %.3e  iterations %d/%d successful %d/%d  cost rel %.3e / %.3e  moved %.3e m" %
                  (i, name, dt, dr, info.lm_iterations[0], tr.iterations, info.lm_successful[0], tr.successful_steps, rel_i, rel_f,
                   np.linalg.norm(pose_g[:3] - pose_plain[:3])))
            assert dt <= TIGHT and dr <= TIGHT, (i, name, dt, dr)
            assert info.lm_iterations[0] == tr.iterations and info.lm_successful[0] == tr.successful_steps, (i, name)
            assert rel_i <= 1e-9 and rel_f <= 1e-9, (i, name, rel_i, rel_f)
            assert info.n_edge[0] == info_plain.n_edge[0] and info.n_plane[0] == info_plain.n_plane[0]   # the prior is no correspondence
            assert not np.array_equal(pose_g, pose_plain)
    h.close()


# ---- 2. whole registration on the three worlds -------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["room", "outdoor", "corridor"])
def test_whole_registration_matches_the_python_outer_loop(gpu, oracle, kind):
    from msf_loam_amd import capi
    _, mc, ms = common.other_world(kind)
    pts, ring, truth, guess = common.other_scans(kind, 1)[0]
    _, corner, surf = common.features_from_oracle(oracle, pts, ring)
    corner, surf = corner[::2], surf[::3]                       # thinned: the numpy loop walks every record in Python
    rng = np.random.default_rng(77)
    prior = (synth.perturb_pose(truth, rng, max_t=0.05, max_deg=0.5), pn.random_spd_sqrt(rng))
    h = capi.Handle(0)
    h.set_map(mc, ms)
    h.set_pose_prior([prior[0]], [prior[1]])
    s, pose_g, info = h.match_scan2map(corner, surf, guess)
    assert s == 0
    pose = np.array(guess, dtype=np.float64)
    for it in range(2):
        h.clear_pose_prior()
        rec = h.associate_scan2map(corner, surf, pose)
        corr = _corr_from_records(corner, surf, rec)
        pose, tr = pn.solve(corr, pose, prior)
        assert info.n_edge[it] == int((corr["kind"] == 1).sum()) and info.n_plane[it] == int((corr["kind"] == 2).sum()), (kind, it)
        assert info.lm_iterations[it] == tr.iterations and info.lm_successful[it] == tr.successful_steps, (kind, it)
        assert abs(info.final_cost[it] - tr.final_cost) <= 1e-9 * tr.final_cost, (kind, it)
    dt, dr = synth.pose_error(pose_g, pose)
    print(kind, "dt %.3e dr %.3e" % (dt, dr), list(info.n_edge), list(info.n_plane), list(info.lm_iterations))
    assert dt <= TIGHT and dr <= TIGHT, (kind, dt, dr)
    h.close()


# ---- 3. the corridor does what the prior is for ------------------------------------------------------------------------

def test_corridor_prior_pins_the_unobservable_direction(gpu, oracle):
    from msf_loam_amd import capi
    _, mc, ms = common.other_world("corridor")
    pts, ring, truth, _ = common.other_scans("corridor", 1)[0]
    _, corner, surf = common.features_from_oracle(oracle, pts, ring)
    h = capi.Handle(0)
    h.set_map(mc, ms)
    h.set_uncertainty(1, MIN_EIG)
    s, _, _ = h.match_scan2map(corner, surf, truth)
    u0 = h.uncertainty(1)[0]
    assert s == 0 and u0["n_degenerate"] >= 1
    ut = u0["eigenvectors"][0][:3]                              # translation part of the weakest eigenvector
    guess = np.array(truth, dtype=np.float64)
    guess[:3] += 0.2 * ut / np.linalg.norm(ut)
    prior = (np.array(truth, dtype=np.float64), pn.translation_only_sqrt(0.05))
    s, pose_f, _ = h.match_scan2map(corner, surf, guess)
    u_f = h.uncertainty(1)[0]
    h.set_pose_prior([prior[0]], [prior[1]])
    s2, pose_fp, _ = h.match_scan2map(corner, surf, guess)
    u_fp = h.uncertainty(1)[0]
    le_f, le_fp = _le_norm(pose_f, prior), _le_norm(pose_fp, prior)
    print("corridor: |L e| without the prior %.6f, with it %.6f; lambda_0 %.1f -> %.1f; n_degenerate %d -> %d" %
          (le_f, le_fp, u_f["eigenvalues"][0], u_fp["eigenvalues"][0], u_f["n_degenerate"], u_fp["n_degenerate"]))
    assert s == 0 and s2 == 0
    assert u_f["n_degenerate"] >= 1
    assert le_fp < le_f
    assert u_fp["n_degenerate"] == 0
    h.close()


# ---- 4. off means off ------------------------------------------------------------------------------------------------

def test_off_means_off(gpu, oracle):
    from msf_loam_amd import capi
    _, mc, ms = common.small_world()
    cs, ss, c, co, s, so, guesses, truths = _batch64(oracle)
    means, Ls = _real_priors(truths)
    fresh = capi.Handle(0)
    fresh.set_map(mc, ms)
    poses_a, st_a, info_a = fresh.match_scan2map_batch(c, co, s, so, guesses, want_info=True)           # (a) never set
    fresh.close()
    h = capi.Handle(0)
    h.set_map(mc, ms)
    h.set_pose_prior(means, Ls)
    poses_on, st_on, _ = h.match_scan2map_batch(c, co, s, so, guesses, want_info=True)
    assert not np.array_equal(poses_on, poses_a)
    h.clear_pose_prior()
    poses_b, st_b, info_b = h.match_scan2map_batch(c, co, s, so, guesses, want_info=True)               # (b) set then cleared
    h.set_pose_prior(means, np.zeros((64, 6, 6)))
    poses_c, st_c, info_c = h.match_scan2map_batch(c, co, s, so, guesses, want_info=True)               # (c) all-zero sqrt_information
    for poses, st, info in ((poses_b, st_b, info_b), (poses_c, st_c, info_c)):
        assert np.array_equal(poses, poses_a) and np.array_equal(st, st_a) and bytes(info) == bytes(info_a)
    # mixed batch: odd scans a zero prior, even scans a real one
    mixed = Ls.copy(); mixed[1::2] = 0.0
    h.set_pose_prior(means, mixed)
    poses_m, st_m, info_m = h.match_scan2map_batch(c, co, s, so, guesses, want_info=True)
    for b in range(1, 64, 2):
        assert np.array_equal(poses_m[b], poses_a[b]) and st_m[b] == st_a[b] and bytes(info_m[b]) == bytes(info_a[b]), b
    for b in range(0, 64, 2):
        h.set_pose_prior([means[b]], [Ls[b]])
        s1, pose1, info1 = h.match_scan2map(cs[b], ss[b], guesses[b])
        assert s1 == st_m[b] and np.array_equal(pose1, poses_m[b]) and bytes(info1) == bytes(info_m[b]), b
        assert np.array_equal(poses_m[b], poses_on[b])
    h.close()


# ---- 5. the call paths agree bitwise ---------------------------------------------------------------------------------

def test_device_pointer_priors_equal_host_priors(gpu, oracle):
    import torch
    from msf_loam_amd import capi
    _, mc, ms = common.small_world()
    cs, ss, c, co, s, so, guesses, truths = _batch64(oracle)
    B = 8
    co, so = co[:B + 1], so[:B + 1]
    means, Ls = _real_priors(truths[:B])
    h = capi.Handle(0)
    h.set_map(mc, ms)
    h.set_pose_prior(means, Ls)
    poses_h, st_h, info_h = h.match_scan2map_batch(c[:co[B]], co, s[:so[B]], so, guesses[:B], want_info=True)
    rec = capi.pose_priors(means, Ls)
    d_prior = torch.from_numpy(np.frombuffer(rec.tobytes(), np.uint8).copy()).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    h.set_pose_prior_device(d_prior, B)
    poses_d, st_d, info_d = h.match_scan2map_batch(c[:co[B]], co, s[:so[B]], so, guesses[:B], want_info=True)
    assert np.array_equal(poses_d, poses_h) and np.array_equal(st_d, st_h) and bytes(info_d) == bytes(info_h)
    # a non-finite DEVICE record: that registration gets MSFL_BAD_ARG and keeps its pose, the others do not notice
    bad = rec.copy(); bad["sqrt_information"][3, 2, 2] = np.nan
    d_bad = torch.from_numpy(np.frombuffer(bad.tobytes(), np.uint8).copy()).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    h.set_pose_prior_device(d_bad, B)
    poses_n, st_n, _ = h.match_scan2map_batch(c[:co[B]], co, s[:so[B]], so, guesses[:B])
    assert st_n[3] == capi.BAD_ARG and np.array_equal(poses_n[3], guesses[3])
    keep = np.arange(B) != 3
    assert np.array_equal(poses_n[keep], poses_h[keep]) and np.array_equal(st_n[keep], st_h[keep])
    h.clear_pose_prior()
    h.close()


def test_pairs_batch_with_priors_equals_looped_single_calls(gpu, oracle):
    from msf_loam_amd import capi
    from tests.test_gpu_pairs import _pairs, _cat
    rng = np.random.default_rng(11)
    mcs, mss, cs, ss, guesses, truths = _pairs(oracle, 8, rng)
    mc, mco = _cat(mcs, lead=7); ms, mso = _cat(mss)
    c, co = _cat(cs, lead=3); s, so = _cat(ss)
    means, Ls = _real_priors(truths, seed=901)
    h = capi.Handle(0)
    poses0, status0, _ = h.match_pairs_batch(mc, mco, ms, mso, c, co, s, so, guesses)
    h.set_pose_prior(means, Ls)
    poses, status, info = h.match_pairs_batch(mc, mco, ms, mso, c, co, s, so, guesses, want_info=True)
    single = capi.Handle(0)
    for p in range(8):
        single.set_map(mcs[p], mss[p])
        single.set_pose_prior([means[p]], [Ls[p]])
        st, pose1, info1 = single.match_scan2map(cs[p], ss[p], guesses[p])
        assert st == status[p] == 0 and np.array_equal(pose1, poses[p]) and bytes(info1) == bytes(info[p]), p
        assert not np.array_equal(poses[p], poses0[p])
    single.close(); h.close()


def test_deskew_batch_with_priors_equals_deskew_single_calls(gpu, oracle):
    from msf_loam_amd import capi
    _, mc, ms = common.small_world()
    rng = np.random.default_rng(33)
    G = np.array([0.0, 0.0, 9.81])
    items, truths = [], []
    for i, (pts, ring, truth, guess) in enumerate(common.scans(3)):
        _, corner, surf = common.features_from_oracle(oracle, pts, ring)
        V = np.array([0.8, -0.3, 0.05]) * (i + 1) / 2
        def dqdp(cloud, k=i):
            t = cloud[:, 3].astype(np.float64)
            dq = np.stack([synth.quat_from_rotvec(r) for r in np.outer(t, [0.02, -0.01, 0.1 * (k + 1)])])
            return dq, np.outer(t, [0.05, 0.02, -0.01]) + rng.normal(0, 1e-4, (len(t), 3))
        items.append((corner, surf, *dqdp(corner), *dqdp(surf), V, guess))
        truths.append(truth)
    co = np.cumsum([0] + [len(it[0]) for it in items]).astype(np.int32)
    so = np.cumsum([0] + [len(it[1]) for it in items]).astype(np.int32)
    cat = lambda k: np.concatenate([it[k] for it in items])
    guesses = np.stack([it[7] for it in items]); vel = np.stack([it[6] for it in items])
    means, Ls = _real_priors(truths, seed=902)
    h = capi.Handle(0)
    h.set_map(mc, ms)
    poses0, _ = h.match_scan2map_deskew_batch(cat(0), co, cat(1), so, cat(2), cat(3), cat(4), cat(5), vel, G, guesses)
    h.set_pose_prior(means, Ls)
    poses, status = h.match_scan2map_deskew_batch(cat(0), co, cat(1), so, cat(2), cat(3), cat(4), cat(5), vel, G, guesses)
    assert np.all(status == 0)
    for b, it in enumerate(items):
        h.set_pose_prior([means[b]], [Ls[b]])
        s1, p, _ = h.match_scan2map_deskew(it[0], it[1], it[2], it[3], it[4], it[5], it[6], G, it[7])
        assert s1 == 0 and np.array_equal(p, poses[b]), b
        assert not np.array_equal(poses[b], poses0[b])
    h.close()


def _scan2scan_inputs(gpu):
    pts, ring, truth, guess = common.scans(1)[0]
    f = gpu.extract_features(pts, ring, extrinsic=IDENT)
    return (f["full"][f["less_sharp"]], f["ring"][f["less_sharp"]], f["full"][f["less_flat"]], f["ring"][f["less_flat"]],
            f["full"][f["sharp"]], f["full"][f["flat"]])


def test_scan2scan_with_a_prior_batch_equals_single_and_gating_holds(gpu):
    """The scan-to-scan tests expose no record dump, so the scan-to-scan solve site is compared batch against single, bitwise
    (docs/kernels/prior.md says so), plus: the prior moves the result, and a pair below min_correspondences keeps its
    MSFL_TOO_FEW_CORRESPONDENCES status and its pose although it has a prior."""
    from msf_loam_amd import capi
    ls, ls_ring, lf, lf_ring, sharp, flat = _scan2scan_inputs(gpu)
    guess = np.array([0.05, -0.03, 0.01, 0, 0, 0.005, 0.9999875])
    prior = (np.array([0.02, 0.01, 0.0, 0, 0, 0, 1.0]), pn.random_spd_sqrt(np.random.default_rng(5)))
    h = capi.Handle(0)
    s0, pose0, info0 = h.match_scan2scan(ls, ls_ring, lf, lf_ring, sharp, flat, guess)
    h.set_pose_prior([prior[0], prior[0]], [prior[1], prior[1]])
    s1, pose1, info1 = h.match_scan2scan(ls, ls_ring, lf, lf_ring, sharp, flat, guess)
    assert s0 == s1 == 0 and not np.array_equal(pose0, pose1)
    assert info1.n_edge[0] == info0.n_edge[0] and info1.n_plane[0] == info0.n_plane[0]          # same first association
    few_s, few_f = sharp[:3], flat[:3]
    clouds = [(np.concatenate([ls, ls]), np.concatenate([ls_ring, ls_ring]), [0, len(ls), 2 * len(ls)]),
              (np.concatenate([lf, lf]), np.concatenate([lf_ring, lf_ring]), [0, len(lf), 2 * len(lf)]),
              (np.concatenate([sharp, few_s]), None, [0, len(sharp), len(sharp) + 3]),
              (np.concatenate([flat, few_f]), None, [0, len(flat), len(flat) + 3])]
    poses, status, info = h.match_scan2scan_batch(clouds, np.array([guess, guess]), want_info=True)
    assert list(status) == [0, capi.TOO_FEW_CORRESPONDENCES]
    assert np.array_equal(poses[0], pose1) and bytes(info[0]) == bytes(info1)
    assert np.array_equal(poses[1], guess)
    h.close()


# ---- 6. posterior information ------------------------------------------------------------------------------------------

def test_posterior_information_is_lidar_plus_prior(gpu, oracle):
    from msf_loam_amd import capi
    h = capi.Handle(0)
    h.set_uncertainty(1)
    for i, (corner, surf, rec, corr, truth, guess) in enumerate(_fixed_sets(oracle)):
        h.clear_pose_prior()
        pose_plain, info_plain = h.solve_records(corner, surf, rec, guess)
        u_plain = h.uncertainty(1)[0]
        for name, prior in _priors_for(i, truth):
            h.set_pose_prior([prior[0]], [prior[1]])
            pose_g, info = h.solve_records(corner, surf, rec, guess)
            u = h.uncertainty(1)[0]
            Jp = pn.prior_rows(pose_g, prior)[2]
            H, _, m = un.information(corr, pose_g)
            d = np.abs(u["information"] - Jp.T @ Jp - H).max() / np.abs(H).max()
            print("posterior %d %s: (information - Jp^T Jp) vs lidar H rel %.3e" % (i, name, d))
            assert u["valid"] == 1 and d <= 1e-9, (i, name, d)
            assert u["n_residuals"] == 3 * info.n_edge[0] + info.n_plane[0] + 6 == m + 6
            assert u["sigma2"] == 2.0 * info.final_cost[0] / (u["n_residuals"] - 6)
        # an all-zero record adds nothing to either
        h.set_pose_prior([truth], [np.zeros((6, 6))])
        pose_z, info_z = h.solve_records(corner, surf, rec, guess)
        assert np.array_equal(pose_z, pose_plain) and bytes(info_z) == bytes(info_plain)
        assert h.uncertainty(1)[0].tobytes() == u_plain.tobytes()
    h.close()


# ---- 7. gating -------------------------------------------------------------------------------------------------------

def test_gating_capacity_and_non_finite_records(gpu, oracle):
    from msf_loam_amd import capi
    _, mc, ms = common.small_world()
    pts, ring, truth, guess = common.scans(1)[0]
    _, corner, surf = common.features_from_oracle(oracle, pts, ring)
    h = capi.Handle(0)
    h.set_map(mc, ms)
    h.set_pose_prior([truth], [pn.translation_only_sqrt(0.05)])
    # one record, two registrations: MSFL_CAPACITY before anything is staged or launched; poses and statuses stay what they were
    c2 = np.concatenate([corner, corner]); s2 = np.concatenate([surf, surf])
    co = np.array([0, len(corner), 2 * len(corner)], np.int32); so = np.array([0, len(surf), 2 * len(surf)], np.int32)
    poses = np.array([guess, guess], np.float64)
    status = np.full(2, -7, np.int32)
    rc = h.lib.msfl_match_scan2map_batch(h.h, C.c_int(2), C.c_void_p(c2.ctypes.data), C.c_void_p(co.ctypes.data), C.c_void_p(s2.ctypes.data),
                                         C.c_void_p(so.ctypes.data), C.c_void_p(poses.ctypes.data), C.c_void_p(status.ctypes.data), None, C.c_int(capi.MEM_HOST))
    assert rc == capi.CAPACITY
    assert np.array_equal(poses, np.array([guess, guess])) and list(status) == [-7, -7]
    # a scan without features: no correspondence, the pose passes through although a prior is set (docs/kernels/prior.md)
    empty = np.zeros((0, 4), np.float32)
    s, pose_e, info_e = h.match_scan2map(empty, empty, guess)
    assert s == 0 and np.array_equal(pose_e, guess) and list(info_e.lm_iterations) == [0, 0]
    # a NaN in a host record: refused with a message, the pose untouched
    L = pn.translation_only_sqrt(0.05); L[4, 1] = np.nan
    h.set_pose_prior([truth], [L])
    with pytest.raises(capi.MsflError) as e:
        h.match_scan2map(corner, surf, guess)
    assert e.value.status == capi.BAD_ARG
    msg = h.lib.msfl_last_error(h.h).decode()
    print("last_error:", msg)
    assert "non-finite" in msg and "sqrt_information[25]" in msg
    mean = np.array(truth, dtype=np.float64); mean[1] = np.inf
    h.set_pose_prior([mean], [pn.translation_only_sqrt(0.05)])
    with pytest.raises(capi.MsflError) as e:
        h.solve_records(corner, surf, np.zeros((len(corner) + len(surf), 6)), guess)
    assert e.value.status == capi.BAD_ARG and "pose[1]" in h.lib.msfl_last_error(h.h).decode()
    # cleared: the plain result
    h.clear_pose_prior()
    s, pose, _ = h.match_scan2map(corner, surf, guess)
    ref = capi.Handle(0); ref.set_map(mc, ms)
    assert s == 0 and np.array_equal(pose, ref.match_scan2map(corner, surf, guess)[1])
    ref.close(); h.close()


# ---- 8. the SLAM step ------------------------------------------------------------------------------------------------

def _slam_case():
    if "slam" not in _cache:
        rp = _rp()
        world = synth.World(ground_half=45.0)
        truth = rp.trajectory(300)[:30]
        scans = [synth.make_scan(world, truth[k], synth.SEED + 5000 + k) for k in range(30)]
        rng = np.random.default_rng(41)
        L_map = [pn.translation_only_sqrt(0.05) if k % 2 else pn.random_spd_sqrt(rng) for k in range(30)]
        real = [(None, (truth[k], L_map[k])) for k in range(30)]
        zero = [((IDENT, np.zeros((6, 6))), (truth[k], np.zeros((6, 6)))) for k in range(30)]
        # both priors before the EVEN scans only: the odd ones must not inherit them
        rel = [IDENT] + [rp.compose(rp.inverse(truth[k - 1]), truth[k]) for k in range(1, 30)]
        even = [((rel[k], pn.translation_only_sqrt(0.05)), (truth[k], L_map[k])) if k % 2 == 0 else None for k in range(30)]
        _cache["slam"] = (rp, world, truth, scans, real, zero, even)
    return _cache["slam"]


def _slam_run(key, pipelined, priors, uncertainty=None):
    """One 30-scan replay, cached by (key, pipelined): (poses, records, uncertainty records)."""
    k = ("slam_run", key, pipelined)
    if k not in _cache:
        rp, world, truth, scans, _, _, _ = _slam_case()
        unc = []
        est, recs, _ = rp.run_slam(world, truth, pipelined=pipelined, scans=scans, priors=priors, uncertainty=uncertainty,
                                   unc_out=unc if uncertainty is not None else None)
        _cache[k] = (est, recs, unc)
    return _cache[k]


def _rec_core(r):
    """What a pipelined and a synchronous replay share bit for bit: the four poses, both msfl_match_info, the statuses and counts, and
    points / cells of the map stores (the stores' pool_top and later report words depend on when the host harvested its bounds:
    tests/test_gpu_slam.py compares grid_surf[:2] for the same reason)."""
    return (bytes(r.pose_odom) + bytes(r.pose_map) + bytes(r.pose_curr2last) + bytes(r.pose_odom2map) + bytes(r.odometry) + bytes(r.mapping) +
            struct.pack("<14i", r.scan_index, r.status_extract, r.status_mapping, r.n_full, r.n_sharp, r.n_less_sharp, r.n_flat, r.n_less_flat,
                        r.n_corner_ds, r.n_surf_ds, r.n_map_corner, r.n_map_surf, r.status_imu, r.status_insert) +
            struct.pack("<4i", *list(r.grid_corner)[:2], *list(r.grid_surf)[:2]))


@pytest.mark.parametrize("pipelined", [False, True])
def test_slam_step_priors(gpu, pipelined):
    rp, world, truth, scans, real, zero, even = _slam_case()
    est0, recs0, _ = _slam_run("none", pipelined, None)
    est_z, recs_z, _ = _slam_run("zero", pipelined, zero)
    assert est_z.tobytes() == est0.tobytes()
    for k in range(30):
        assert bytes(recs_z[k]) == bytes(recs0[k]), k
    est_r, recs_r, unc_r = _slam_run("real", pipelined, real, MIN_EIG)
    est_s, recs_s, unc_s = _slam_run("real", False, real, MIN_EIG)                # the synchronous run (cached)
    assert est_r.tobytes() == est_s.tobytes()
    for k in range(30):
        assert _rec_core(recs_r[k]) == _rec_core(recs_s[k]), k
        assert unc_r[k].tobytes() == unc_s[k].tobytes(), k
    assert not np.array_equal(est_r, est0)
    n_valid = 0
    for k in range(1, 30):
        m, info = unc_r[k][1], recs_r[k].mapping
        if recs_r[k].status_mapping != 0 or info.status != 0:
            assert m["valid"] == 0
            continue
        n_valid += 1
        assert m["valid"] == 1 and m["n_residuals"] == 3 * info.n_edge[1] + info.n_plane[1] + 6, k
        assert m["sigma2"] == 2.0 * info.final_cost[1] / (m["n_residuals"] - 6), k
        o, oinfo = unc_r[k][0], recs_r[k].odometry
        if oinfo.status == 0:
            assert o["n_residuals"] == 3 * oinfo.n_edge[1] + oinfo.n_plane[1], k                 # no odometry prior in this run
    assert n_valid >= 20
    # priors before the even scans only: scan k + 1 does not inherit scan k's
    est_e, recs_e, unc_e = _slam_run("even", pipelined, even, MIN_EIG)
    n_with = n_without = 0
    for k in range(1, 30):
        extra = 6 if k % 2 == 0 else 0
        for which, info in ((0, recs_e[k].odometry), (1, recs_e[k].mapping)):
            u = unc_e[k][which]
            if info.status != 0 or (which == 1 and recs_e[k].status_mapping != 0):
                assert u["valid"] == 0
                continue
            assert u["n_residuals"] == 3 * info.n_edge[1] + info.n_plane[1] + extra, (k, which)
            n_with += extra == 6
            n_without += extra == 0
    assert n_with >= 15 and n_without >= 15


# ---- 9. the C++ mirror -------------------------------------------------------------------------------------------------

def test_cpp_adapter_reproduces_the_ctypes_pose(gpu, oracle, tmp_path):
    from msf_loam_amd import capi
    exe = str(tmp_path / "prior_check")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "prior_check.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "msf_loam_amd"), "-lmsfl_hip", "-Wl,-rpath," + os.path.join(ROOT, "msf_loam_amd")])
    _, mc, ms = common.other_world("corridor")
    pts, ring, truth, guess = common.other_scans("corridor", 1)[0]
    _, corner, surf = common.features_from_oracle(oracle, pts, ring)
    rng = np.random.default_rng(19)
    mean = synth.perturb_pose(truth, rng, max_t=0.05, max_deg=0.5)
    L = pn.random_spd_sqrt(rng)
    A = rng.normal(size=(6, 6))
    cov = np.diag([0.05] * 3 + [0.01] * 3) @ (A @ A.T / 6.0 + np.eye(6)) @ np.diag([0.05] * 3 + [0.01] * 3)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        for cloud in (mc, ms, corner, surf):
            a = np.ascontiguousarray(cloud, "<f4").reshape(-1, 4)
            f.write(struct.pack("<i", len(a))); f.write(a.tobytes())
        for a in (guess, mean, L, cov):
            f.write(np.ascontiguousarray(a, "<f8").tobytes())
    subprocess.check_call([exe, str(fin), str(fout)])
    raw = open(fout, "rb").read()
    assert len(raw) == 56 + 56 + 288
    h = capi.Handle(0)
    h.set_map(mc, ms)
    h.set_pose_prior([mean], [L])
    s, pose_p, _ = h.match_scan2map(corner, surf, guess)
    h.clear_pose_prior()
    s0, pose_0, _ = h.match_scan2map(corner, surf, guess)
    h.close()
    assert s == 0 and s0 == 0 and not np.array_equal(pose_p, pose_0)
    assert raw[:56] == pose_p.tobytes()
    assert raw[56:112] == pose_0.tobytes()
    # SqrtInformationFromCovariance: L^T L cov = I.  cond(cov) <= 1e3 here (asserted), a Cholesky factor and a triangular inverse
    # are backward stable, so the product is off by a modest multiple of cond * eps: 1e-10 leaves three orders
    Lc = np.frombuffer(raw[112:], "<f8").reshape(6, 6)
    assert np.linalg.cond(cov) <= 1e3
    d = np.abs(Lc.T @ Lc @ cov - np.eye(6)).max()
    print("SqrtInformationFromCovariance: |L^T L cov - I| %.3e" % d)
    assert d <= 1e-10
