"""GPU: msfl_match_uncertainty (msfl_set_uncertainty / msfl_slam_set_uncertainty) against the independent numpy model
(tests/uncertainty_numpy.py) and against itself across the call paths.

The reference computes no covariance, so there is no reference output to compare with: the yardstick is the numpy
restatement of what ceres::Covariance would be handed (tests/ceres_numpy.evaluate -> J^T J) at the GPU's returned pose.

Bars (from the issue that introduced the feature; none comes from what the kernel happens to deliver):
  information   max-norm difference <= 1e-9 * max|H|: the bar tests/test_gpu_scan2map.py holds the cost to; cost and H leave the
                same accumulators
  eigenvalues   within 1e-12 * lambda_max of numpy.linalg.eigvalsh(information): backward stability of a symmetric solver is
                O(eps * |H|), three orders of margin
  eigenvectors  |V V^T - I|_max <= 1e-12
  covariance    vs numpy.linalg.inv(information), max-norm relative <= 1e-10: cond(H) <= 1e4 (asserted on the CPU in
                tests/test_uncertainty_model.py) times eps, ~50x margin
  sigma2, n_residuals   exact from `info`
"""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from msf_loam_amd import synth
from tests import common
from tests import uncertainty_numpy as un

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_EIG = 150.0
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])


def _oracle_records(orc, mc, ms, corner, surf, pose):
    corr = orc.associate_scan2map(mc, ms, corner, surf, pose, use_kdtree=True)
    rec = np.zeros((len(corr), 6))
    ok = corr["kind"] != 0
    rec[ok, :3] = corr["C"][ok]
    rec[ok, 3:] = corr["N"][ok]
    return rec, corr


def _check_eigen(u, what="", min_eig=0.0):
    """The record's decomposition against LAPACK on its OWN information matrix."""
    assert u["valid"] == 1, what
    H = u["information"]
    assert np.array_equal(H, H.T), what
    w, V = u["eigenvalues"], u["eigenvectors"]
    assert np.all(np.diff(w) >= 0), (what, w)
    ref = np.linalg.eigvalsh(H)
    d_eig = np.abs(w - ref).max() / ref[-1]
    d_orth = np.abs(V @ V.T - np.eye(6)).max()
    print(what, "eig rel %.3e  orth %.3e" % (d_eig, d_orth), end="")
    assert d_eig <= 1e-12, (what, d_eig)
    assert d_orth <= 1e-12, (what, d_orth)
    for k in range(6):
        assert V[k, int(np.argmax(np.abs(V[k])))] > 0, (what, k)            # sign convention
    thr = max(min_eig, 1e-14 * w[-1])
    assert u["n_degenerate"] == int((w < thr).sum()), what
    if u["n_degenerate"] == 0:
        inv = np.linalg.inv(H)
        d_cov = np.abs(u["covariance"] - inv).max() / np.abs(inv).max()
        print("  cov rel %.3e" % d_cov)
        assert d_cov <= 1e-10, (what, d_cov)
    else:
        cov = u["covariance"]
        d_p = np.abs(H @ cov @ H - sum(w[k] * np.outer(V[k], V[k]) for k in range(u["n_degenerate"], 6))).max() / np.abs(H).max()
        print("  pinv rel %.3e" % d_p)
        assert d_p <= 1e-10, (what, d_p)                                     # the pseudo-inverse over the kept pairs


def _rp():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import replay_synthetic as rp
    return rp


def _check_model(u, corr, pose, info, it, what=""):
    """information against the numpy H of the problem `corr` at the GPU's returned pose; sigma2 / n_residuals from info."""
    H, cost, m = un.information(corr, pose)
    d = np.abs(u["information"] - H).max() / np.abs(H).max()
    print(what, "information rel %.3e (cond %.0f)" % (d, u["eigenvalues"][5] / max(u["eigenvalues"][0], 1e-300)))
    assert d <= 1e-9, (what, d)
    assert u["n_residuals"] == 3 * info.n_edge[it] + info.n_plane[it] == m, what
    assert u["sigma2"] == 2.0 * info.final_cost[it] / (u["n_residuals"] - 6), what
    assert u["reserved_"] == 0


def _is_zero(u):
    return u.tobytes() == bytes(u.dtype.itemsize)


# ---- 1. fixed records -----------------------------------------------------------------------------------------------

def test_fixed_records_information_matches_the_numpy_model(gpu, oracle):
    from msf_loam_amd import capi
    _, mc, ms = common.small_world()
    h = capi.Handle(0)
    h.set_map(mc, ms)
    h.set_uncertainty(1)
    for i, (pts, ring, truth, guess) in enumerate(common.scans(3)):
        _, corner, surf = common.features_from_oracle(oracle, pts, ring)
        rec_o, corr = _oracle_records(oracle, mc, ms, corner, surf, guess)
        pose_g, info = h.solve_records(corner, surf, rec_o, guess)
        u = h.uncertainty(1)[0]
        _check_model(u, corr, pose_g, info, 0, "fixed %d" % i)
        _check_eigen(u, "fixed %d" % i)
    h.close()


# ---- 2. full match on the three worlds -----------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,expect_degenerate", [("room", 0), ("outdoor", 0), ("corridor", 1)])
def test_full_match_information_on_the_three_worlds(gpu, oracle, kind, expect_degenerate):
    from msf_loam_amd import capi
    _, mc, ms = common.other_world(kind)
    h2 = capi.Handle(0)
    p1 = capi.default_params(); p1.outer_iterations = 1
    h1 = capi.Handle(0, p1)
    for h in (h1, h2):
        h.set_map(mc, ms)
    for i, (pts, ring, truth, guess) in enumerate(common.other_scans(kind, 2)):
        _, corner, surf = common.features_from_oracle(oracle, pts, ring)
        s1, pose_mid, info1 = h1.match_scan2map(corner, surf, guess)
        h2.set_uncertainty(1, 0.0)                                            # nothing dropped: covariance is the inverse
        s2, pose, info = h2.match_scan2map(corner, surf, guess)
        u_full = h2.uncertainty(1)[0]
        h2.set_uncertainty(1, MIN_EIG)
        s3, pose3, info3 = h2.match_scan2map(corner, surf, guess)
        assert s1 == 0 and s2 == 0 and s3 == 0 and np.array_equal(pose, pose3) and bytes(info) == bytes(info3)
        # the one-iteration handle returns the two-iteration run's intermediate pose: its first half, bit for bit
        for f in ("n_edge", "n_plane", "lm_iterations", "lm_successful", "initial_cost", "final_cost"):
            assert getattr(info1, f)[0] == getattr(info, f)[0], f
        corr = oracle.associate_scan2map(mc, ms, corner, surf, pose_mid)      # the second solve's records
        assert int((corr["kind"] == 1).sum()) == info.n_edge[1] and int((corr["kind"] == 2).sum()) == info.n_plane[1]
        u = h2.uncertainty(1)[0]
        _check_model(u_full, corr, pose, info, 1, "%s %d" % (kind, i))
        _check_eigen(u_full, "%s %d" % (kind, i))
        assert u_full["n_degenerate"] == 0
        _check_eigen(u, "%s %d at %.0f" % (kind, i, MIN_EIG), MIN_EIG)
        for f in ("information", "eigenvalues", "eigenvectors", "sigma2", "n_residuals"):
            assert np.array_equal(u[f], u_full[f]), f                          # the threshold only moves n_degenerate and the covariance
        print(kind, i, "eigenvalues", u["eigenvalues"], "v0", u["eigenvectors"][0])
        assert u["n_degenerate"] == expect_degenerate == un.record(corr, pose, MIN_EIG)["n_degenerate"]
        if kind == "corridor":
            assert int(np.argmax(np.abs(u["eigenvectors"][0]))) == 0
    h1.close(); h2.close()


# ---- 3. the feature perturbs nothing ------------------------------------------------------------------------------------

def _batch64(oracle):
    cs, ss, guesses = [], [], []
    for pts, ring, truth, guess in common.scans(64):
        _, corner, surf = common.features_from_oracle(oracle, pts, ring)
        cs.append(corner); ss.append(surf); guesses.append(guess)
    co = np.cumsum([0] + [len(c) for c in cs]).astype(np.int32)
    so = np.cumsum([0] + [len(s) for s in ss]).astype(np.int32)
    return cs, ss, np.concatenate(cs), co, np.concatenate(ss), so, np.array(guesses)


def test_batch_results_are_bit_identical_with_the_feature_on_and_off(gpu, oracle):
    from msf_loam_amd import capi
    _, mc, ms = common.small_world()
    cs, ss, c, co, s, so, guesses = _batch64(oracle)
    h = capi.Handle(0)
    h.set_map(mc, ms)
    poses0, st0, info0 = h.match_scan2map_batch(c, co, s, so, guesses, want_info=True)
    h.set_uncertainty(64)
    poses1, st1, info1 = h.match_scan2map_batch(c, co, s, so, guesses, want_info=True)
    poses2, st2, _ = h.match_scan2map_batch(c, co, s, so, guesses, want_info=False)      # the record borrows the info scratch: no info asked for
    u_b = h.uncertainty(64)
    h.set_uncertainty(0)
    poses3, st3, info3 = h.match_scan2map_batch(c, co, s, so, guesses, want_info=True)
    for poses, st in ((poses1, st1), (poses2, st2), (poses3, st3)):
        assert poses.tobytes() == poses0.tobytes() and st.tobytes() == st0.tobytes()
    assert bytes(info1) == bytes(info0) == bytes(info3)
    assert all(u["valid"] == 1 for u in u_b)
    # 4a. scan b's record in the batch equals the single call's bytes
    h.set_uncertainty(1)
    for b in (0, 17, 63):
        s1, pose1, _ = h.match_scan2map(cs[b], ss[b], guesses[b])
        assert np.array_equal(pose1, poses0[b])
        assert h.uncertainty(1)[0].tobytes() == u_b[b].tobytes(), b
    for b in (0, 63):
        _check_eigen(u_b[b], "batch %d" % b)
        assert u_b[b]["sigma2"] == 2.0 * info0[b].final_cost[1] / (u_b[b]["n_residuals"] - 6)
    h.close()


def _slam_scans(n):
    rp = _rp()
    world = synth.World(ground_half=45.0)
    truth = rp.trajectory(300)[:n]
    return rp, world, truth, [synth.make_scan(world, truth[k], synth.SEED + 5000 + k) for k in range(n)]


@pytest.mark.parametrize("pipelined", [False, True])
def test_slam_replay_is_bit_identical_and_its_records_hold(gpu, pipelined):
    rp, world, truth, scans = _slam_scans(30)
    est0, recs0, _ = rp.run_slam(world, truth, pipelined=pipelined, scans=scans)
    unc = []
    est1, recs1, _ = rp.run_slam(world, truth, pipelined=pipelined, scans=scans, uncertainty=MIN_EIG, unc_out=unc)
    assert est0.tobytes() == est1.tobytes()
    for k in range(30):
        assert bytes(recs0[k]) == bytes(recs1[k]), k
    assert len(unc) == 30
    # scan 0: no MatchScan2Scan (laser_odometry.cc:72-73) and the gate is closed on an empty map (laser_mapping.cc:284-285)
    assert _is_zero(unc[0][0]) and _is_zero(unc[0][1]) and recs1[0].status_mapping != 0
    n_valid = 0
    for k in range(1, 30):
        for which, info in ((0, recs1[k].odometry), (1, recs1[k].mapping)):
            u = unc[k][which]
            solved = info.status == 0 and (which == 0 or recs1[k].status_mapping == 0)
            assert u["valid"] == (1 if solved else 0), (k, which)
            if not solved:
                assert _is_zero(u)
                continue
            n_valid += 1
            _check_eigen(u, "slam %d/%d" % (k, which), MIN_EIG)
            assert u["n_residuals"] == 3 * info.n_edge[1] + info.n_plane[1]
            assert u["sigma2"] == 2.0 * info.final_cost[1] / (u["n_residuals"] - 6), (k, which)
    assert n_valid >= 50


# ---- 4. the call paths agree ---------------------------------------------------------------------------------------------

def test_pairs_batch_records_equal_looped_single_calls(gpu, oracle):
    from msf_loam_amd import capi
    from tests.test_gpu_pairs import _pairs, _cat
    rng = np.random.default_rng(11)
    mcs, mss, cs, ss, guesses, truths = _pairs(oracle, 4, rng)
    mcs[2] = mcs[2][:3]                                   # MSFL_MAP_TOO_SMALL pair
    mc, mco = _cat(mcs, lead=7); ms, mso = _cat(mss)
    c, co = _cat(cs, lead=3); s, so = _cat(ss)
    h = capi.Handle(0)
    h.set_uncertainty(4, MIN_EIG)
    poses, status, info = h.match_pairs_batch(mc, mco, ms, mso, c, co, s, so, guesses, want_info=True)
    u_p = h.uncertainty(4)
    single = capi.Handle(0)
    single.set_uncertainty(1, MIN_EIG)
    for p in range(4):
        if p == 2:
            assert status[p] == capi.MAP_TOO_SMALL and _is_zero(u_p[p]) and np.array_equal(poses[p], guesses[p])
            continue
        single.set_map(mcs[p], mss[p])
        st, pose1, info1 = single.match_scan2map(cs[p], ss[p], guesses[p])
        assert st == 0 and np.array_equal(pose1, poses[p])
        assert single.uncertainty(1)[0].tobytes() == u_p[p].tobytes(), p
        _check_eigen(u_p[p], "pair %d" % p, MIN_EIG)
    single.close(); h.close()


def test_device_pointer_path_equals_the_host_path(gpu, oracle):
    import torch
    from msf_loam_amd import capi
    _, mc, ms = common.small_world()
    cs, ss, c, co, s, so, guesses = _batch64(oracle)
    B = 8
    co, so = co[:B + 1], so[:B + 1]
    h = capi.Handle(0)
    h.set_map(mc, ms)
    h.set_uncertainty(B, MIN_EIG)
    poses_h, st_h, _ = h.match_scan2map_batch(c[:co[B]], co, s[:so[B]], so, guesses[:B])
    u_h = h.uncertainty(B)
    dev = torch.device("cuda", 0)
    d_c, d_s = torch.from_numpy(c[:co[B]].copy()).to(dev), torch.from_numpy(s[:so[B]].copy()).to(dev)
    d_poses = torch.from_numpy(guesses[:B].copy()).to(dev)
    d_status = torch.zeros(B, dtype=torch.int32, device=dev)
    d_unc = torch.full((B * capi.UNCERTAINTY_DTYPE.itemsize,), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    h.set_uncertainty_device(d_unc, B, MIN_EIG)
    h.match_scan2map_batch_device(B, d_c, co, d_s, so, d_poses, d_status)
    h.synchronize()
    u_d = np.frombuffer(d_unc.cpu().numpy().tobytes(), capi.UNCERTAINTY_DTYPE)
    assert d_poses.cpu().numpy().tobytes() == poses_h.tobytes()
    assert u_d.tobytes() == u_h.tobytes()
    # capacity: a call with more registrations than the sink holds is refused before anything is launched
    h.set_uncertainty_device(d_unc, B - 1, MIN_EIG)
    d_poses2 = torch.from_numpy(guesses[:B].copy()).to(dev)
    torch.cuda.synchronize()
    with pytest.raises(capi.MsflError) as e:
        h.match_scan2map_batch_device(B, d_c, co, d_s, so, d_poses2, d_status)
    assert e.value.status == capi.CAPACITY
    h.synchronize()
    assert d_poses2.cpu().numpy().tobytes() == guesses[:B].tobytes()
    h.set_uncertainty(0)
    h.close()


def _scan2scan_inputs(gpu):
    pts, ring, truth, guess = common.scans(1)[0]
    f = gpu.extract_features(pts, ring, extrinsic=IDENT)
    return (f["full"][f["less_sharp"]], f["ring"][f["less_sharp"]], f["full"][f["less_flat"]], f["ring"][f["less_flat"]],
            f["full"][f["sharp"]], f["full"][f["flat"]])


def test_scan2scan_record(gpu):
    from msf_loam_amd import capi
    ls, ls_ring, lf, lf_ring, sharp, flat = _scan2scan_inputs(gpu)
    guess = np.array([0.05, -0.03, 0.01, 0, 0, 0.005, 0.9999875])
    h = capi.Handle(0)
    s0, pose0, info0 = h.match_scan2scan(ls, ls_ring, lf, lf_ring, sharp, flat, guess)
    h.set_uncertainty(2)
    s1, pose1, info1 = h.match_scan2scan(ls, ls_ring, lf, lf_ring, sharp, flat, guess)
    assert s0 == s1 == 0 and np.array_equal(pose0, pose1) and bytes(info0) == bytes(info1)
    u = h.uncertainty(1)[0]
    assert u["valid"] == 1 and u["n_residuals"] == 3 * info1.n_edge[1] + info1.n_plane[1]
    assert u["sigma2"] == 2.0 * info1.final_cost[1] / (u["n_residuals"] - 6)
    _check_eigen(u, "scan2scan")
    # the batch form: pair 0 as above, pair 1 with too few features (MSFL_TOO_FEW_CORRESPONDENCES)
    few_s, few_f = sharp[:3], flat[:3]
    clouds = [(np.concatenate([ls, ls]), np.concatenate([ls_ring, ls_ring]), [0, len(ls), 2 * len(ls)]),
              (np.concatenate([lf, lf]), np.concatenate([lf_ring, lf_ring]), [0, len(lf), 2 * len(lf)]),
              (np.concatenate([sharp, few_s]), None, [0, len(sharp), len(sharp) + 3]),
              (np.concatenate([flat, few_f]), None, [0, len(flat), len(flat) + 3])]
    poses, status, info = h.match_scan2scan_batch(clouds, np.array([guess, guess]), want_info=True)
    ub = h.uncertainty(2)
    assert list(status) == [0, capi.TOO_FEW_CORRESPONDENCES]
    assert ub[0].tobytes() == u.tobytes() and np.array_equal(poses[0], pose1)
    assert _is_zero(ub[1])
    h.close()


# ---- 5. gating -----------------------------------------------------------------------------------------------------------

def test_gating_and_capacity(gpu, oracle):
    from msf_loam_amd import capi
    _, mc, ms = common.small_world()
    pts, ring, truth, guess = common.scans(1)[0]
    _, corner, surf = common.features_from_oracle(oracle, pts, ring)
    h = capi.Handle(0)
    h.set_map(mc, ms)
    h.set_uncertainty(1)
    s, pose, info = h.match_scan2map(corner, surf, guess)
    assert s == 0 and h.uncertainty(1)[0]["valid"] == 1
    empty = np.zeros((0, 4), np.float32)
    s, pose_e, info_e = h.match_scan2map(empty, empty, guess)                 # a scan with no features: Ceres solves an empty problem
    assert s == 0 and np.array_equal(pose_e, guess) and _is_zero(h.uncertainty(1)[0])
    # capacity 1, two registrations: MSFL_CAPACITY before anything is staged or launched; the poses stay what they were
    c2 = np.concatenate([corner, corner]); s2 = np.concatenate([surf, surf])
    co = np.array([0, len(corner), 2 * len(corner)], np.int32); so = np.array([0, len(surf), 2 * len(surf)], np.int32)
    poses = np.array([guess, guess], np.float64)
    status = np.full(2, -7, np.int32)
    before = h.uncertainty(1).tobytes()
    rc = h.lib.msfl_match_scan2map_batch(h.h, C.c_int(2), C.c_void_p(c2.ctypes.data), C.c_void_p(co.ctypes.data), C.c_void_p(s2.ctypes.data),
                                         C.c_void_p(so.ctypes.data), C.c_void_p(poses.ctypes.data), C.c_void_p(status.ctypes.data), None, C.c_int(capi.MEM_HOST))
    assert rc == capi.CAPACITY
    assert np.array_equal(poses, np.array([guess, guess])) and list(status) == [-7, -7] and h.uncertainty(1).tobytes() == before
    # off again: nothing is written any more
    h.set_uncertainty(0)
    s, pose3, _ = h.match_scan2map(corner, surf, guess)
    assert np.array_equal(pose3, pose)
    with pytest.raises(RuntimeError):
        h.uncertainty(1)
    h.close()


# ---- 6. the corridor drive through the SLAM step ---------------------------------------------------------------------------

def test_corridor_drive_reports_a_degenerate_direction(gpu, oracle):
    rp_mod = _rp()
    world, mc, ms = common.other_world("corridor")
    truth = common.world_drive("corridor", 12)
    scans = [synth.make_scan(world, truth[k], synth.SEED + 5000 + k) for k in range(12)]
    # first the CPU model on a few of the drive's scans (against the world's full map): the x direction is below the threshold there
    for k in (3, 7, 11):
        _, corner, surf = common.features_from_oracle(oracle, *scans[k])
        corr, pose, _ = un.oracle_last_problem(oracle, mc, ms, corner, surf, truth[k])
        rec = un.record(corr, pose, MIN_EIG)
        print("cpu model, drive scan", k, rec["eigenvalues"])
        assert rec["n_degenerate"] >= 1
    unc = []
    est, recs, _ = rp_mod.run_slam(world, truth, scans=scans, uncertainty=MIN_EIG, unc_out=unc)
    n = 0
    for k in range(1, 12):
        m = unc[k][1]
        if recs[k].status_mapping != 0:
            assert _is_zero(m)
            continue
        n += 1
        print("slam, drive scan", k, m["eigenvalues"], m["n_degenerate"])
        _check_eigen(m, "corridor %d" % k, MIN_EIG)
        assert m["n_degenerate"] >= 1, (k, m["eigenvalues"])
        assert m["sigma2"] == 2.0 * recs[k].mapping.final_cost[1] / (m["n_residuals"] - 6)
    assert n >= 8


# ---- 7. the C++ mirror -----------------------------------------------------------------------------------------------------

def test_cpp_adapter_reproduces_the_ctypes_record(gpu, oracle, tmp_path):
    from msf_loam_amd import capi
    exe = str(tmp_path / "uncertainty_check")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "uncertainty_check.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "msf_loam_amd"), "-lmsfl_hip", "-Wl,-rpath," + os.path.join(ROOT, "msf_loam_amd")])
    _, mc, ms = common.other_world("corridor")
    pts, ring, truth, guess = common.other_scans("corridor", 1)[0]
    _, corner, surf = common.features_from_oracle(oracle, pts, ring)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        for cloud in (mc, ms, corner, surf):
            a = np.ascontiguousarray(cloud, "<f4").reshape(-1, 4)
            f.write(struct.pack("<i", len(a))); f.write(a.tobytes())
        f.write(np.asarray(guess, "<f8").tobytes()); f.write(struct.pack("<d", MIN_EIG))
    subprocess.check_call([exe, str(fin), str(fout)])
    raw = open(fout, "rb").read()
    assert len(raw) == 56 + 936 + 288
    h = capi.Handle(0)
    h.set_map(mc, ms)
    h.set_uncertainty(1, MIN_EIG)
    s, pose, info = h.match_scan2map(corner, surf, guess)
    u = h.uncertainty(1)[0]
    h.close()
    assert s == 0 and raw[:56] == pose.tobytes()
    assert raw[56:56 + 936] == u.tobytes()
    assert u["n_degenerate"] == 1
    parent = np.frombuffer(raw[56 + 936:], "<f8").reshape(6, 6)
    want = un.covariance_in_parent_frame(pose, u["covariance"], u["sigma2"])
    d = np.abs(parent - want).max() / np.abs(want).max()
    print("CovarianceInParentFrame rel %.3e" % d)
    assert d <= 1e-15
