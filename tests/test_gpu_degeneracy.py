"""GPU: the degeneracy-aware solve (msfl_set_degeneracy / msfl_slam_set_degeneracy; docs/kernels/degeneracy.md) against the
independent numpy model (tests/degeneracy_numpy.py over the trust-region loop of tests/ceres_numpy.py) and against itself
across the call paths.

The reference has no solution remapping, so there is no reference output to compare with.

Bars (from the issue that introduced the feature; none comes from what the kernel happens to deliver):
  eigenvectors    orthonormal to 1e-12; |H0 v - lambda v| <= 1e-9 lambda_max and eigenvalues within 1e-9 lambda_max of eigvalsh,
                  against the numpy H0 at the solve's entry pose
  n_held          equal to the model's classification
  pose            <= 1e-7 m / rad against degeneracy_numpy.solve run WITH THE RECORD'S OWN V (just verified): close eigenvalue
                  pairs make the basis inside their span ill-conditioned and the Jacobi scaling is basis-dependent
  counts, costs   lm_iterations / lm_successful exact, costs relative <= 1e-9 (the bars of tests/test_gpu_pose_prior.py)
  axis case       |x_out - x_guess| <= 1e-12 m with the feature on, > 1e-3 m with it off
  everything "equals" / "identical"   byte comparison
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from msf_loam_amd import synth
from tests import ceres_numpy as cn
from tests import common
from tests import degeneracy_numpy as dn
from tests import lm_boundary_cases as lb
from tests import prior_numpy as pn
from tests.test_gpu_pose_prior import _batch64, _corr_from_records, _rec_core, _rp, _scan2scan_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIGHT = 1e-7
MIN_EIG = 150.0           # between the corridor's weak eigenvalue (~50) and the next (>= 370): docs/kernels/uncertainty.md
_cache = {}


@pytest.fixture(scope="module")
def handles(gpu):
    """One fresh handle per solve workgroup of msfl_solve_records (the knob is read when the handle is created)."""
    from msf_loam_amd import capi
    hs = {}
    for block in lb.BLOCKS:
        with pytest.MonkeyPatch.context() as monkeypatch:
            monkeypatch.setenv("MSFL_SOLVE_RECORDS_BLOCK", str(block))
            hs[block] = capi.Handle(0)
    yield hs
    for h in hs.values():
        h.close()


def _check_decomposition(lam, V, H0, what):
    """The record's eigenpairs against the numpy H0; returns lambda_max."""
    lam_np = np.linalg.eigvalsh(H0)
    lmax = lam_np[-1]
    orth = np.abs(V @ V.T - np.eye(6)).max()
    resid = max(np.abs(H0 @ V[k] - lam[k] * V[k]).max() for k in range(6))
    dlam = np.abs(lam - lam_np).max()
    print("%s: orthonormality %.2e  |H0 v - lambda v| / lambda_max %.2e  |lambda - eigvalsh| / lambda_max %.2e" %
          (what, orth, resid / lmax, dlam / lmax))
    assert orth <= 1e-12, (what, orth)
    assert resid <= 1e-9 * lmax, (what, resid, lmax)
    assert dlam <= 1e-9 * lmax, (what, dlam, lmax)
    assert np.all(np.diff(lam) >= 0)
    for k in range(6):                                          # the sign convention of msfl_match_uncertainty.eigenvectors
        assert V[k, int(np.argmax(np.abs(V[k])))] > 0, (what, k)
    return lam_np


def _compare_solve(pose_g, info, it, pose_n, tr, what):
    dt, dr = synth.pose_error(pose_g, pose_n)
    rel_i = abs(info.initial_cost[it] - tr.initial_cost) / tr.initial_cost
    rel_f = abs(info.final_cost[it] - tr.final_cost) / tr.final_cost
    print("%s: dt %.3e dr %.3e  iterations %d/%d successful %d/%d  cost rel %.3e / %.3e" %
          (what, dt, dr, info.lm_iterations[it], tr.iterations, info.lm_successful[it], tr.successful_steps, rel_i, rel_f))
    assert info.lm_iterations[it] == tr.iterations and info.lm_successful[it] == tr.successful_steps, what
    assert rel_i <= 1e-9 and rel_f <= 1e-9, (what, rel_i, rel_f)
    return dt, dr


# ---- 1. fixed records, both widths -------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", dn.cases(), ids=dn.case_id)
def test_fixed_records_match_the_numpy_model(handles, c):
    h = handles[c.block]
    h.set_degeneracy(c.min_eig, 1)
    pose_g, info = h.solve_records(c.corner, c.surf, c.rec, c.guess)
    d = h.degeneracy(1)[0]
    h.clear_degeneracy()
    assert d["valid"][0] == 1
    assert d["valid"][1] == 0 and d["n_held"][1] == 0 and not d["eigenvalues"][1].any() and not d["eigenvectors"][1].any()   # one solve only
    lam, V = d["eigenvalues"][0], d["eigenvectors"][0]
    cost0, _, H0 = dn.entry_matrix(c.corr, c.guess)
    lam_np = _check_decomposition(lam, V, H0, dn.case_id(c))
    assert d["n_held"][0] == dn.classify(lam_np, c.min_eig) == c.n_held
    if c.n_held == 6:
        assert np.array_equal(pose_g, c.guess)
        assert info.lm_iterations[0] == 0 and info.lm_successful[0] == 0 and info.status == 0
        assert info.initial_cost[0] == info.final_cost[0] and abs(info.initial_cost[0] - cost0) <= 1e-9 * cost0
        return
    pose_n, tr = dn.solve(c.corr, c.guess, V, c.n_held)
    dt, dr = _compare_solve(pose_g, info, 0, pose_n, tr, dn.case_id(c))
    assert dt <= TIGHT and dr <= TIGHT, (dn.case_id(c), dt, dr)
    pose_off, info_off = h.solve_records(c.corner, c.surf, c.rec, c.guess)
    if c.n_held == 0:
        assert np.array_equal(pose_g, pose_off) and bytes(info) == bytes(info_off)
    else:
        assert not np.array_equal(pose_g, pose_off)


# ---- 2. the axis case ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("block", lb.BLOCKS)
def test_axis_case_holds_x_at_the_guess(handles, block):
    c = next(c for c in dn.cases() if c.name == "axis" and c.block == block)
    h = handles[block]
    pose_off, _ = h.solve_records(c.corner, c.surf, c.rec, c.guess)
    h.set_degeneracy(c.min_eig, 1)
    pose_on, _ = h.solve_records(c.corner, c.surf, c.rec, c.guess)
    d = h.degeneracy(1)[0]
    h.clear_degeneracy()
    print("axis case, %d threads: x moved %.3e m with the feature on, %.6f m with it off; lambda_0 %.6f, v_0 %s" %
          (block, abs(pose_on[0] - c.guess[0]), abs(pose_off[0] - c.guess[0]), d["eigenvalues"][0][0], d["eigenvectors"][0][0]))
    assert d["n_held"][0] == 1
    assert abs(pose_on[0] - c.guess[0]) <= 1e-12
    assert abs(pose_off[0] - c.guess[0]) > 1e-3
    assert np.linalg.norm(pose_on[1:3] - c.guess[1:3]) > 1e-3                  # the observable directions did move


# ---- 3. whole registrations against the Python outer loop --------------------------------------------------------------

def _world_case(oracle, kind):
    if ("world", kind) not in _cache:
        _, mc, ms = common.other_world(kind)
        pts, ring, truth, guess = common.other_scans(kind, 1)[0]
        _, corner, surf = common.features_from_oracle(oracle, pts, ring)
        _cache[("world", kind)] = (mc, ms, corner[::2], surf[::3], truth, guess)      # thinned: the numpy loop walks every record in Python
    return _cache[("world", kind)]


@pytest.mark.parametrize("kind", ["room", "outdoor", "corridor"])
def test_whole_registration_matches_the_python_outer_loop(gpu, oracle, kind):
    from msf_loam_amd import capi
    mc, ms, corner, surf, truth, guess = _world_case(oracle, kind)
    h = capi.Handle(0)
    h.set_map(mc, ms)
    h.set_degeneracy(0.0, 1)                                    # a first look at the spectrum, nothing held
    s, pose_0, _ = h.match_scan2map(corner, surf, guess)
    lam0 = h.degeneracy(1)[0]["eigenvalues"][0]
    # corridor: between the weak eigenvalue and the next; the other worlds: in the widest gap of the entry spectrum
    thr = float(np.sqrt(lam0[0] * lam0[1])) if kind == "corridor" else dn.gap_threshold(lam0)[0]
    h.set_degeneracy(thr, 1)
    s, pose_g, info = h.match_scan2map(corner, surf, guess)
    d = h.degeneracy(1)[0]
    assert s == 0 and list(d["valid"]) == [1, 1]
    print(kind, "threshold %.2f" % thr, "eigenvalues", d["eigenvalues"][0], d["eigenvalues"][1], "n_held", list(d["n_held"]))
    if kind == "corridor":
        for it in range(2):
            assert d["eigenvalues"][it][0] < thr < d["eigenvalues"][it][1], (it, d["eigenvalues"][it][:2], thr)
    h.clear_degeneracy()
    pose = np.array(guess, dtype=np.float64)
    for it in range(2):
        rec = h.associate_scan2map(corner, surf, pose)
        corr = _corr_from_records(corner, surf, rec)
        lam_np = _check_decomposition(d["eigenvalues"][it], d["eigenvectors"][it], dn.entry_matrix(corr, pose)[2], "%s outer %d" % (kind, it))
        assert dn.margin(lam_np, thr) >= 1.2, (kind, it, lam_np, thr)           # a condition on the inputs: the held set does not hang on rounding
        assert d["n_held"][it] == dn.classify(lam_np, thr) and 0 < d["n_held"][it] < 6, (kind, it)
        pose, tr = dn.solve(corr, pose, d["eigenvectors"][it], int(d["n_held"][it]))
        assert info.n_edge[it] == int((corr["kind"] == 1).sum()) and info.n_plane[it] == int((corr["kind"] == 2).sum()), (kind, it)
        _compare_solve(pose if it == 1 else pose_g, info, it, pose_g, tr, "%s outer %d (counts and costs; the pose follows)" % (kind, it))
    dt, dr = synth.pose_error(pose_g, pose)
    print(kind, "dt %.3e dr %.3e" % (dt, dr))
    assert dt <= TIGHT and dr <= TIGHT, (kind, dt, dr)
    assert not np.array_equal(pose_g, pose_0)
    h.close()


# ---- 4. the corridor does what the feature is for ----------------------------------------------------------------------

def _tangent(a, b):
    """[dt, dtheta] with b = Plus(a, .): translation difference and the rotation vector of conj(q_a) q_b."""
    ax, ay, az, aw = a[3:7]
    bx, by, bz, bw = b[3:7]
    v = np.array([aw * bx - ax * bw - ay * bz + az * by, aw * by - ay * bw - az * bx + ax * bz, aw * bz - az * bw - ax * by + ay * bx])
    w = aw * bw + ax * bx + ay * by + az * bz
    n = np.linalg.norm(v)
    rot = np.zeros(3) if n == 0 else v / n * 2.0 * np.arctan2(n, w)
    return np.concatenate([b[:3] - a[:3], rot])


def test_corridor_weak_direction_stays_at_the_guess(gpu, oracle):
    from msf_loam_amd import capi
    _, mc, ms = common.other_world("corridor")
    pts, ring, truth, _ = common.other_scans("corridor", 1)[0]
    _, corner, surf = common.features_from_oracle(oracle, pts, ring)
    h = capi.Handle(0)
    h.set_map(mc, ms)
    h.set_degeneracy(MIN_EIG, 1)
    s, _, _ = h.match_scan2map(corner, surf, truth)
    v_t = h.degeneracy(1)[0]["eigenvectors"][0][0]
    # the guess: the truth displaced along an observable direction only (a translation orthogonal to the weak eigenvector's)
    e = np.cross(v_t[:3], [0.0, 0.0, 1.0]); e /= np.linalg.norm(e)
    guess = np.array(truth, dtype=np.float64); guess[:3] += 0.1 * e
    s_on, pose_on, _ = h.match_scan2map(corner, surf, guess)
    d = h.degeneracy(1)[0]
    v0 = d["eigenvectors"][0][0]
    h.clear_degeneracy()
    s_off, pose_off, _ = h.match_scan2map(corner, surf, guess)
    m_on, m_off = abs(v0 @ _tangent(guess, pose_on)), abs(v0 @ _tangent(guess, pose_off))
    print("corridor: |v0 . tangent(guess -> out)| with the feature %.6e, without %.6e; n_held %s, lambda_0 %.2f lambda_1 %.2f" %
          (m_on, m_off, list(d["n_held"]), d["eigenvalues"][0][0], d["eigenvalues"][0][1]))
    assert s_on == 0 and s_off == 0 and d["n_held"][0] >= 1
    assert m_on < m_off
    h.close()


# ---- 5. off means off; nothing held means nothing changed --------------------------------------------------------------

def test_off_means_off_and_nothing_held_changes_nothing(gpu, oracle):
    from msf_loam_amd import capi
    _, mc, ms = common.small_world()
    cs, ss, c, co, s, so, guesses, truths = _batch64(oracle)
    fresh = capi.Handle(0)
    fresh.set_map(mc, ms)
    poses_a, st_a, info_a = fresh.match_scan2map_batch(c, co, s, so, guesses, want_info=True)           # (a) never set
    fresh.close()
    h = capi.Handle(0)
    h.set_map(mc, ms)
    h.set_degeneracy(1e9, 64)
    poses_all, _, _ = h.match_scan2map_batch(c, co, s, so, guesses, want_info=True)
    assert np.array_equal(poses_all, guesses)                                                           # (the feature does act on this handle)
    h.clear_degeneracy()
    poses_b, st_b, info_b = h.match_scan2map_batch(c, co, s, so, guesses, want_info=True)               # (b) enabled = 0
    h.set_degeneracy(1e-3, 64)
    poses_c, st_c, info_c = h.match_scan2map_batch(c, co, s, so, guesses, want_info=True)               # (c) a threshold below every eigenvalue
    d = h.degeneracy(64)
    ok = st_a == 0
    assert ok.sum() >= 60
    assert not d["n_held"].any() and np.all(d["valid"][ok] == 1) and np.all(d["eigenvalues"][ok][:, :, 0] > 1e-3 * 2)
    for poses, st, info in ((poses_b, st_b, info_b), (poses_c, st_c, info_c)):
        assert np.array_equal(poses, poses_a) and np.array_equal(st, st_a) and bytes(info) == bytes(info_a)
    h.close()


def test_mixed_batch_changes_only_the_registrations_with_held_directions(gpu, oracle):
    """Room and corridor registrations in one msfl_match_pairs_batch call (every pair has its own map)."""
    from msf_loam_amd import capi
    from tests.test_gpu_pairs import _cat
    mcs, mss, cs, ss, guesses = [], [], [], [], []
    for kind, i in (("room", 0), ("corridor", 0), ("room", 1), ("corridor", 1)):
        _, mc, ms = common.other_world(kind)
        pts, ring, truth, guess = common.other_scans(kind, 2)[i]
        _, corner, surf = common.features_from_oracle(oracle, pts, ring)
        mcs.append(mc); mss.append(ms); cs.append(corner); ss.append(surf); guesses.append(guess)
    mc, mco = _cat(mcs); ms, mso = _cat(mss); c, co = _cat(cs); s, so = _cat(ss)
    guesses = np.array(guesses)
    h = capi.Handle(0)
    poses0, st0, info0 = h.match_pairs_batch(mc, mco, ms, mso, c, co, s, so, guesses, want_info=True)
    h.set_degeneracy(MIN_EIG, 4)
    poses1, st1, info1 = h.match_pairs_batch(mc, mco, ms, mso, c, co, s, so, guesses, want_info=True)
    d = h.degeneracy(4)
    print("mixed batch: n_held", d["n_held"].tolist(), "lambda_0", d["eigenvalues"][:, :, 0].tolist())
    held = d["n_held"].sum(1) > 0
    assert list(st0) == [0, 0, 0, 0] and np.array_equal(st0, st1)
    assert held.any() and not held.all()
    for b in range(4):
        same = np.array_equal(poses1[b], poses0[b]) and bytes(info1[b]) == bytes(info0[b])
        assert same == (not held[b]), (b, held[b])
    h.close()


# ---- 6. all held -------------------------------------------------------------------------------------------------------

def test_all_held_passes_the_pose_through(gpu, oracle):
    from msf_loam_amd import capi
    mc, ms, corner, surf, truth, guess = _world_case(oracle, "room")
    h = capi.Handle(0)
    h.set_map(mc, ms)
    h.set_degeneracy(1e12, 1)
    s, pose, info = h.match_scan2map(corner, surf, guess)
    d = h.degeneracy(1)[0]
    assert s == 0 and info.status == 0 and np.array_equal(pose, guess)
    assert list(d["n_held"]) == [6, 6] and list(d["valid"]) == [1, 1]
    assert list(info.lm_iterations) == [0, 0] and list(info.lm_successful) == [0, 0]
    assert info.initial_cost[0] == info.final_cost[0] > 0 and info.initial_cost[1] == info.final_cost[1] == info.initial_cost[0]
    assert info.n_plane[0] > 0 and info.n_plane[1] == info.n_plane[0]
    h.close()


# ---- 7. with a prior -----------------------------------------------------------------------------------------------------

def test_a_prior_can_make_the_weak_direction_observable(gpu, oracle):
    from msf_loam_amd import capi
    _, mc, ms = common.other_world("corridor")
    pts, ring, truth, guess = common.other_scans("corridor", 1)[0]
    _, corner, surf = common.features_from_oracle(oracle, pts, ring)
    h = capi.Handle(0)
    h.set_map(mc, ms)
    h.set_degeneracy(MIN_EIG, 1)
    s, pose_d, _ = h.match_scan2map(corner, surf, guess)
    d0 = h.degeneracy(1)[0]
    assert s == 0 and list(d0["n_held"]) == [1, 1]
    # a translation prior along the weak axis: information 1 / (0.05 m)^2 = 400 on that direction
    ut = d0["eigenvectors"][0][0][:3] / np.linalg.norm(d0["eigenvectors"][0][0][:3])
    L = np.zeros((6, 6)); L[0, :3] = ut / 0.05
    h.set_pose_prior([truth], [L])
    s, pose_dp, info_dp = h.match_scan2map(corner, surf, guess)
    d1 = h.degeneracy(1)[0]
    print("corridor: lambda_0 %.2f -> %.2f with the prior, n_held %s -> %s" % (d0["eigenvalues"][0][0], d1["eigenvalues"][0][0], list(d0["n_held"]), list(d1["n_held"])))
    assert s == 0 and list(d1["n_held"]) == [0, 0]
    h.clear_degeneracy()
    s, pose_p, info_p = h.match_scan2map(corner, surf, guess)
    assert s == 0 and np.array_equal(pose_dp, pose_p) and bytes(info_dp) == bytes(info_p)
    assert not np.array_equal(pose_dp, pose_d)
    h.close()


@pytest.mark.parametrize("block", lb.BLOCKS)
def test_held_with_a_prior_matches_the_model(handles, block):
    c = next(c for c in dn.cases() if c.name == "axis" and c.block == block)
    rng = np.random.default_rng(61)
    mean = synth.perturb_pose(c.guess, rng, max_t=0.05, max_deg=0.5)
    L = pn.random_spd_sqrt(rng, scale_t=1.0, scale_r=30.0)      # ~1 on the translation block: the weak eigenvalue stays far below the threshold
    prior = (mean, L)
    cost0, _, H0 = dn.entry_matrix(c.corr, c.guess, prior)
    thr = dn.gap_threshold(np.linalg.eigvalsh(H0)[:3])[0]
    h = handles[block]
    h.set_pose_prior([mean], [L])
    h.set_degeneracy(thr, 1)
    pose_g, info = h.solve_records(c.corner, c.surf, c.rec, c.guess)
    d = h.degeneracy(1)[0]
    h.clear_degeneracy()
    pose_p, _ = h.solve_records(c.corner, c.surf, c.rec, c.guess)
    h.clear_pose_prior()
    lam_np = _check_decomposition(d["eigenvalues"][0], d["eigenvectors"][0], H0, "axis + prior, %d" % block)
    assert dn.margin(lam_np, thr) >= 2.0
    assert d["n_held"][0] == dn.classify(lam_np, thr) and 0 < d["n_held"][0] < 6
    pose_n, tr = dn.solve(c.corr, c.guess, d["eigenvectors"][0], int(d["n_held"][0]), prior=prior)
    dt, dr = _compare_solve(pose_g, info, 0, pose_n, tr, "axis + prior, %d" % block)
    assert dt <= TIGHT and dr <= TIGHT
    assert not np.array_equal(pose_g, pose_p)


# ---- 8. the call paths agree bitwise -----------------------------------------------------------------------------------

def _room_threshold(h, corner, surf, guess):
    """A threshold in the widest gap of a room registration's entry spectrum: some directions are held, some kept."""
    h.set_degeneracy(0.0, 1)
    h.match_scan2map(corner, surf, guess)
    return dn.gap_threshold(h.degeneracy(1)[0]["eigenvalues"][0])[0]


def test_batch_equals_single_calls_and_device_sink_equals_host_sink(gpu, oracle):
    import torch
    from msf_loam_amd import capi
    _, mc, ms = common.small_world()
    cs, ss, c, co, s, so, guesses, truths = _batch64(oracle)
    B = 8
    co, so = co[:B + 1], so[:B + 1]
    h = capi.Handle(0)
    h.set_map(mc, ms)
    thr = _room_threshold(h, cs[0], ss[0], guesses[0])
    h.set_degeneracy(thr, B)
    poses, st, info = h.match_scan2map_batch(c[:co[B]], co, s[:so[B]], so, guesses[:B], want_info=True)
    d = h.degeneracy(B)
    assert d["n_held"].any() and np.all(d["n_held"] < 6)
    for b in range(B):
        h.set_degeneracy(thr, 1)
        s1, pose1, info1 = h.match_scan2map(cs[b], ss[b], guesses[b])
        assert s1 == st[b] and np.array_equal(pose1, poses[b]) and bytes(info1) == bytes(info[b]), b
        assert h.degeneracy(1)[0].tobytes() == d[b].tobytes(), b
    d_sink = torch.zeros(B * capi.DEGENERACY_DTYPE.itemsize, dtype=torch.uint8, device=torch.device("cuda", 0))
    d_sink.fill_(255)
    torch.cuda.synchronize()
    h.set_degeneracy_device(thr, d_sink, B)
    poses_d, st_d, info_d = h.match_scan2map_batch(c[:co[B]], co, s[:so[B]], so, guesses[:B], want_info=True)
    h.synchronize()
    assert np.array_equal(poses_d, poses) and np.array_equal(st_d, st) and bytes(info_d) == bytes(info)
    assert d_sink.cpu().numpy().tobytes() == d.tobytes()
    # no sink at all: the remapping still runs
    h.set_degeneracy(thr, 0)
    poses_n, st_n, info_n = h.match_scan2map_batch(c[:co[B]], co, s[:so[B]], so, guesses[:B], want_info=True)
    assert np.array_equal(poses_n, poses) and bytes(info_n) == bytes(info)
    h.close()


def test_pairs_batch_equals_looped_single_calls(gpu, oracle):
    from msf_loam_amd import capi
    from tests.test_gpu_pairs import _pairs, _cat
    rng = np.random.default_rng(11)
    mcs, mss, cs, ss, guesses, truths = _pairs(oracle, 8, rng)
    mc, mco = _cat(mcs, lead=7); ms, mso = _cat(mss)
    c, co = _cat(cs, lead=3); s, so = _cat(ss)
    single = capi.Handle(0)
    single.set_map(mcs[0], mss[0])
    thr = _room_threshold(single, cs[0], ss[0], guesses[0])
    h = capi.Handle(0)
    h.set_degeneracy(thr, 8)
    poses, status, info = h.match_pairs_batch(mc, mco, ms, mso, c, co, s, so, guesses, want_info=True)
    d = h.degeneracy(8)
    assert d["n_held"].any()
    for p in range(8):
        single.set_map(mcs[p], mss[p])
        single.set_degeneracy(thr, 1)
        st, pose1, info1 = single.match_scan2map(cs[p], ss[p], guesses[p])
        assert st == status[p] == 0 and np.array_equal(pose1, poses[p]) and bytes(info1) == bytes(info[p]), p
        assert single.degeneracy(1)[0].tobytes() == d[p].tobytes(), p
    single.close(); h.close()


def test_deskew_batch_equals_deskew_single_calls(gpu, oracle):
    from msf_loam_amd import capi
    _, mc, ms = common.small_world()
    rng = np.random.default_rng(33)
    G = np.array([0.0, 0.0, 9.81])
    items = []
    for i, (pts, ring, truth, guess) in enumerate(common.scans(3)):
        _, corner, surf = common.features_from_oracle(oracle, pts, ring)
        V = np.array([0.8, -0.3, 0.05]) * (i + 1) / 2

        def dqdp(cloud, k=i):
            t = cloud[:, 3].astype(np.float64)
            dq = np.stack([synth.quat_from_rotvec(r) for r in np.outer(t, [0.02, -0.01, 0.1 * (k + 1)])])
            return dq, np.outer(t, [0.05, 0.02, -0.01]) + rng.normal(0, 1e-4, (len(t), 3))
        items.append((corner, surf, *dqdp(corner), *dqdp(surf), V, guess))
    co = np.cumsum([0] + [len(it[0]) for it in items]).astype(np.int32)
    so = np.cumsum([0] + [len(it[1]) for it in items]).astype(np.int32)
    cat = lambda k: np.concatenate([it[k] for it in items])
    guesses = np.stack([it[7] for it in items]); vel = np.stack([it[6] for it in items])
    h = capi.Handle(0)
    h.set_map(mc, ms)
    thr = _room_threshold(h, items[0][0], items[0][1], items[0][7])
    h.clear_degeneracy()
    poses0, _ = h.match_scan2map_deskew_batch(cat(0), co, cat(1), so, cat(2), cat(3), cat(4), cat(5), vel, G, guesses)
    h.set_degeneracy(thr, 3)
    poses, status = h.match_scan2map_deskew_batch(cat(0), co, cat(1), so, cat(2), cat(3), cat(4), cat(5), vel, G, guesses)
    d = h.degeneracy(3)
    assert np.all(status == 0) and np.all(d["n_held"].sum(1) > 0)
    for b, it in enumerate(items):
        h.set_degeneracy(thr, 1)
        s1, p, _ = h.match_scan2map_deskew(it[0], it[1], it[2], it[3], it[4], it[5], it[6], G, it[7])
        assert s1 == 0 and np.array_equal(p, poses[b]), b
        assert h.degeneracy(1)[0].tobytes() == d[b].tobytes(), b
        assert not np.array_equal(poses[b], poses0[b])
    h.close()


def test_scan2scan_batch_equals_single_and_gating_holds(gpu):
    """No record dump exists for scan-to-scan, so that solve site is compared batch against single, bitwise, as the prior tests do;
    plus: a pair below min_correspondences keeps its status and pose and gets an all-zero record."""
    from msf_loam_amd import capi
    ls, ls_ring, lf, lf_ring, sharp, flat = _scan2scan_inputs(gpu)
    guess = np.array([0.05, -0.03, 0.01, 0, 0, 0.005, 0.9999875])
    h = capi.Handle(0)
    s0, pose0, info0 = h.match_scan2scan(ls, ls_ring, lf, lf_ring, sharp, flat, guess)
    h.set_degeneracy(0.0, 2)
    h.match_scan2scan(ls, ls_ring, lf, lf_ring, sharp, flat, guess)
    thr = dn.gap_threshold(h.degeneracy(1)[0]["eigenvalues"][0])[0]
    h.set_degeneracy(thr, 2)
    s1, pose1, info1 = h.match_scan2scan(ls, ls_ring, lf, lf_ring, sharp, flat, guess)
    d1 = h.degeneracy(1)[0]
    assert s0 == s1 == 0 and d1["n_held"][0] > 0 and not np.array_equal(pose0, pose1)
    few_s, few_f = sharp[:3], flat[:3]
    clouds = [(np.concatenate([ls, ls]), np.concatenate([ls_ring, ls_ring]), [0, len(ls), 2 * len(ls)]),
              (np.concatenate([lf, lf]), np.concatenate([lf_ring, lf_ring]), [0, len(lf), 2 * len(lf)]),
              (np.concatenate([sharp, few_s]), None, [0, len(sharp), len(sharp) + 3]),
              (np.concatenate([flat, few_f]), None, [0, len(flat), len(flat) + 3])]
    poses, status, info = h.match_scan2scan_batch(clouds, np.array([guess, guess]), want_info=True)
    d = h.degeneracy(2)
    assert list(status) == [0, capi.TOO_FEW_CORRESPONDENCES]
    assert np.array_equal(poses[0], pose1) and bytes(info[0]) == bytes(info1) and d[0].tobytes() == d1.tobytes()
    assert np.array_equal(poses[1], guess) and d[1].tobytes() == bytes(capi.DEGENERACY_DTYPE.itemsize)
    h.close()


# ---- 9. gating -----------------------------------------------------------------------------------------------------------

def test_gating_capacity_and_bad_thresholds(gpu, oracle):
    from msf_loam_amd import capi
    _, mc, ms = common.small_world()
    pts, ring, truth, guess = common.scans(1)[0]
    _, corner, surf = common.features_from_oracle(oracle, pts, ring)
    h = capi.Handle(0)
    h.set_map(mc, ms)
    for bad in (-1.0, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(capi.MsflError) as e:
            h.set_degeneracy(bad, 1)
        assert e.value.status == capi.BAD_ARG
    s, pose_ref, info_ref = h.match_scan2map(corner, surf, guess)           # the refused calls changed nothing
    h.set_degeneracy(1e12, 1)
    # a sink of one record, two registrations: MSFL_CAPACITY before anything is staged or launched
    c2 = np.concatenate([corner, corner]); s2 = np.concatenate([surf, surf])
    co = np.array([0, len(corner), 2 * len(corner)], np.int32); so = np.array([0, len(surf), 2 * len(surf)], np.int32)
    poses = np.array([guess, guess], np.float64)
    status = np.full(2, -7, np.int32)
    h._degen[:] = np.frombuffer(b"\x55" * 688, capi.DEGENERACY_DTYPE)
    rc = h.lib.msfl_match_scan2map_batch(h.h, C.c_int(2), C.c_void_p(c2.ctypes.data), C.c_void_p(co.ctypes.data), C.c_void_p(s2.ctypes.data),
                                         C.c_void_p(so.ctypes.data), C.c_void_p(poses.ctypes.data), C.c_void_p(status.ctypes.data), None, C.c_int(capi.MEM_HOST))
    assert rc == capi.CAPACITY
    assert np.array_equal(poses, np.array([guess, guess])) and list(status) == [-7, -7]
    assert h._degen.tobytes() == b"\x55" * 688                              # a failing call writes nothing
    # a scan without features: nothing to solve, nothing decomposed, the record all zero, the pose untouched
    empty = np.zeros((0, 4), np.float32)
    s, pose_e, info_e = h.match_scan2map(empty, empty, guess)
    assert s == 0 and np.array_equal(pose_e, guess) and h.degeneracy(1)[0].tobytes() == bytes(688)
    h.clear_degeneracy()
    s, pose, info = h.match_scan2map(corner, surf, guess)
    assert np.array_equal(pose, pose_ref) and bytes(info) == bytes(info_ref)
    h.close()


# ---- 10. the SLAM step ---------------------------------------------------------------------------------------------------

N_SLAM = 12


def _slam_scans(kind):
    if ("slam_scans", kind) not in _cache:
        rp = _rp()
        if kind == "room":
            world = synth.World(ground_half=45.0)
            truth = rp.trajectory(300)[:N_SLAM]
        else:
            world = synth.World(kind=kind)
            truth = rp.world_drive(world, kind, N_SLAM)
        scans = [synth.make_scan(world, truth[k], synth.SEED + 5000 + k) for k in range(N_SLAM)]
        _cache[("slam_scans", kind)] = (rp, world, truth, scans)
    return _cache[("slam_scans", kind)]


def _slam_run(kind, pipelined, degeneracy):
    key = ("slam_run", kind, pipelined, degeneracy)
    if key not in _cache:
        rp, world, truth, scans = _slam_scans(kind)
        out = []
        est, recs, _ = rp.run_slam(world, truth, pipelined=pipelined, scans=scans, degeneracy=degeneracy, degen_out=out)
        _cache[key] = (est, recs, out)
    return _cache[key]


@pytest.mark.parametrize("pipelined", [False, True])
def test_slam_step_room_nothing_held_is_bit_identical(gpu, pipelined):
    est0, recs0, _ = _slam_run("room", pipelined, None)
    est1, recs1, degen = _slam_run("room", pipelined, (1e-3, 1e-3))
    assert len(degen) == N_SLAM
    n_valid = 0
    for k in range(N_SLAM):
        o, m = degen[k]
        assert not o["n_held"].any() and not m["n_held"].any(), k
        n_valid += int(m["valid"].sum())
        if k == 0:
            assert o.tobytes() == bytes(688)                                # scan 0 has no scan-to-scan match
        assert bytes(recs1[k]) == bytes(recs0[k]), k
    assert n_valid >= N_SLAM and est1.tobytes() == est0.tobytes()


@pytest.mark.parametrize("pipelined", [False, True])
def test_slam_step_corridor_holds_and_pipelined_equals_synchronous(gpu, pipelined):
    from msf_loam_amd import capi
    est, recs, degen = _slam_run("corridor", pipelined, (None, MIN_EIG))
    est_s, recs_s, degen_s = _slam_run("corridor", False, (None, MIN_EIG))
    est0, _, _ = _slam_run("corridor", False, None)
    held = [int(m["n_held"].max()) for _, m in degen]
    print("corridor SLAM step, mapping n_held per scan:", held)
    assert max(held) >= 1
    assert est.tobytes() == est_s.tobytes() and not np.array_equal(est, est0)
    for k in range(N_SLAM):
        assert _rec_core(recs[k]) == _rec_core(recs_s[k]), k
        assert degen[k][0].tobytes() == degen_s[k][0].tobytes() and degen[k][1].tobytes() == degen_s[k][1].tobytes(), k
        assert degen[k][0].tobytes() == bytes(688)                          # the odometry matcher was left off


def test_slam_get_degeneracy_refuses_what_it_cannot_deliver(gpu):
    from msf_loam_amd import capi
    rp, world, truth, scans = _slam_scans("room")
    slam = capi.Slam(0, max_scan_points=max(len(p) for p, _ in scans), max_rings=16, pose_odom2map=truth[0])
    for bad in ((-1.0, 1.0), (1.0, float("nan")), (float("inf"), None)):
        with pytest.raises(capi.MsflError) as e:
            slam.set_degeneracy(odometry=bad[0], mapping=bad[1])
        assert e.value.status == capi.BAD_ARG
    slam.add_scan(*scans[0])                                                  # fed with the feature off
    with pytest.raises(capi.MsflError) as e:
        slam.get_degeneracy(0)
    assert e.value.status == capi.BAD_ARG
    slam.set_degeneracy(odometry=1e-3, mapping=1e-3)
    slam.add_scan(*scans[1])
    o, m = slam.get_degeneracy(1)
    assert o["valid"].any() or m["valid"].any()
    for k in (2, 7, -1):                                                      # not fed yet / out of range
        with pytest.raises(capi.MsflError) as e:
            slam.get_degeneracy(k)
        assert e.value.status == capi.BAD_ARG, k
    slam.close()


# ---- 11. the C++ mirror ----------------------------------------------------------------------------------------------------

def test_cpp_adapter_reproduces_the_ctypes_pose(gpu, oracle, tmp_path):
    from msf_loam_amd import capi
    exe = str(tmp_path / "degeneracy_check")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "degeneracy_check.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "msf_loam_amd"), "-lmsfl_hip", "-Wl,-rpath," + os.path.join(ROOT, "msf_loam_amd")])
    _, mc, ms = common.other_world("corridor")
    pts, ring, truth, guess = common.other_scans("corridor", 1)[0]
    _, corner, surf = common.features_from_oracle(oracle, pts, ring)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        for cloud in (mc, ms, corner, surf):
            a = np.ascontiguousarray(cloud, "<f4").reshape(-1, 4)
            f.write(struct.pack("<i", len(a))); f.write(a.tobytes())
        f.write(np.ascontiguousarray(guess, "<f8").tobytes())
        f.write(struct.pack("<d", MIN_EIG))
    subprocess.check_call([exe, str(fin), str(fout)])
    raw = open(fout, "rb").read()
    assert len(raw) == 56 + 56 + 16
    h = capi.Handle(0)
    h.set_map(mc, ms)
    h.set_degeneracy(MIN_EIG, 1)
    s, pose_d, _ = h.match_scan2map(corner, surf, guess)
    d = h.degeneracy(1)[0]
    h.clear_degeneracy()
    s0, pose_0, _ = h.match_scan2map(corner, surf, guess)
    h.close()
    assert s == 0 and s0 == 0 and not np.array_equal(pose_d, pose_0) and d["n_held"][0] >= 1
    assert raw[:56] == pose_d.tobytes()
    assert raw[56:112] == pose_0.tobytes()
    assert list(np.frombuffer(raw[112:], "<f8")) == [float(d["n_held"][0]), float(d["n_held"][1])]
