"""GPU: outlier rejection in front of the solve (msfl_set_outlier_rejection / msfl_slam_set_outlier_rejection;
docs/kernels/rejection.md) against the independent numpy model (tests/rejection_numpy.py) and against itself across the call paths.

The reference's hook is commented out, so there is no reference output to compare with.

Bars (from the issue that introduced the feature; none comes from what the kernels happen to deliver):
  fixed records        solve_records with rejection on == solve_records on the records with the model's mask zeroed, feature off:
                       pose and msfl_match_info bitwise; the record's counts exact; cut_sq within 1e-12 relative
  moved object         the GPU pose within 1e-7 m / rad of ceres_numpy.solve on the model's survivors
  whole registration   counts exact, pose within TIGHT = 1e-7 of solve_records on the zeroed records of associate_scan2map at the
                       solve's entry pose; every s at least 1e-6 relative from thr2 (asserted, never skipped)
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
from tests import lm_boundary_cases as lb
from tests import rejection_numpy as rn
from tests.test_gpu_degeneracy import _world_case
from tests.test_gpu_pose_prior import _batch64, _corr_from_records, _rec_core, _rp, _scan2scan_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIGHT = 1e-7
THR = rn.REFERENCE_THRESHOLD
FIELDS = ("n_edge_in", "n_plane_in", "n_edge_rejected", "n_plane_rejected")
ZERO = bytes(56)
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


def _check_record(r, it, want, what):
    """Slice `it` of a record against the model's: counts exact, cut_sq within 1e-12 relative."""
    got = {f: int(r[f][it]) for f in FIELDS}
    print(what, "outer", it, got, "cut_sq %.17g (model %.17g)" % (r["cut_sq"][it], want["cut_sq"]))
    assert r["valid"][it] == 1, what
    assert got == {f: want[f] for f in FIELDS}, (what, got, want)
    assert abs(r["cut_sq"][it] - want["cut_sq"]) <= 1e-12 * want["cut_sq"], (what, r["cut_sq"][it], want["cut_sq"])


def _slice_is_zero(r, it):
    return all(r[f][it] == 0 for f in FIELDS) and r["cut_sq"][it] == 0.0 and r["valid"][it] == 0


def _run_fixed(h, corner, surf, rec, corr, guess, mode, threshold, fraction, what, off_run=True):
    mask, want = rn.decide(corr, guess, mode, threshold=threshold, fraction=fraction)
    pose_ref, info_ref = h.solve_records(corner, surf, rn.zeroed(rec, mask), guess)
    h.set_outlier_rejection(threshold=threshold, fraction=fraction, n=1)
    try:
        pose_on, info_on = h.solve_records(corner, surf, rec, guess)
        r = h.rejection(1)[0]
    finally:
        h.clear_outlier_rejection()
    _check_record(r, 0, want, what)
    assert _slice_is_zero(r, 1), what                               # msfl_solve_records has one solve
    assert np.array_equal(pose_on, pose_ref) and bytes(info_on) == bytes(info_ref), what
    assert info_on.n_edge[0] == want["n_edge_in"] - want["n_edge_rejected"] and info_on.n_plane[0] == want["n_plane_in"] - want["n_plane_rejected"]
    if off_run:
        pose_off, info_off = h.solve_records(corner, surf, rec, guess)
        same = np.array_equal(pose_on, pose_off) and bytes(info_on) == bytes(info_off)
        assert same == (not mask.any()), (what, int(mask.sum()))
    return pose_on, info_on, mask


# ---- 1. fixed records, both widths -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("block", lb.BLOCKS)
@pytest.mark.parametrize("c", rn.cases(), ids=lambda c: c.name)
def test_fixed_records_equal_the_solve_on_the_models_survivors(handles, c, block):
    # (the records with a non-finite entry are only ever solved with those rows rejected)
    pose, info, mask = _run_fixed(handles[block], c.corner, c.surf, c.rec, c.corr, c.guess, c.mode, c.threshold, c.fraction,
                                  "%s, %d threads" % (c.name, block), off_run=not c.name.startswith("non_finite"))
    assert int(mask.sum()) == c.n_rejected
    if c.name == "fraction_one":                                    # nothing left: the empty-problem rule, the pose passes through
        assert np.array_equal(pose, c.guess) and info.status == 0 and info.n_edge[0] == 0 and info.n_plane[0] == 0
    if c.name == "fraction_zero":
        assert not mask.any()                                       # (_run_fixed compared bitwise with the feature-off result)
    if c.name == "moved_object":
        kept = np.array(c.corr)
        kept["kind"][mask] = 0
        pose_n, _ = cn.solve(kept, np.array(c.guess))
        dt, dr = synth.pose_error(pose, pose_n)
        print("moved object, %d threads: dt %.3e dr %.3e against the model; %.3e m from the truth" % (block, dt, dr, synth.pose_error(pose, c.truth)[0]))
        assert dt <= TIGHT and dr <= TIGHT


@pytest.mark.parametrize("block", lb.BLOCKS)
@pytest.mark.parametrize("c", rn.seam_cases(), ids=rn.seam_case_id)
def test_seam_cases_with_threshold_rejection(handles, c, block):
    p = lb.problem(c.k)
    _run_fixed(handles[block], p.corner, p.surf, p.rec, p.corr, p.guess, rn.THRESHOLD, rn.SEAM_THRESHOLD, None,
               "%s, %d threads" % (rn.seam_case_id(c), block))


# ---- 2. whole registrations ----------------------------------------------------------------------------------------------------

def _expected_solve(h, corner, surf, pose, threshold, what):
    """Association at `pose`, the model's mask (with its margin asserted), the solve on the zeroed records: (pose, info, record)."""
    rec = h.associate_scan2map(corner, surf, pose)
    corr = _corr_from_records(corner, surf, rec)
    if threshold is None:
        pose_e, info_e = h.solve_records(corner, surf, rec, pose)
        return pose_e, info_e, None
    m = rn.margin(corr, pose, rn.THRESHOLD, threshold=threshold)
    mask, want = rn.decide(corr, pose, rn.THRESHOLD, threshold=threshold)
    print(what, "margin %.3e" % m, want)
    assert m >= rn.MARGIN, (what, m)
    pose_e, info_e = h.solve_records(corner, surf, rn.zeroed(rec, mask), pose)
    return pose_e, info_e, want


def _same_solve(info, it, info_e, pose, pose_e, what):
    dt, dr = synth.pose_error(pose, pose_e)
    print(what, "dt %.3e dr %.3e  n_edge %d/%d n_plane %d/%d" % (dt, dr, info.n_edge[it], info_e.n_edge[0], info.n_plane[it], info_e.n_plane[0]))
    assert info.n_edge[it] == info_e.n_edge[0] and info.n_plane[it] == info_e.n_plane[0], what
    assert dt <= TIGHT and dr <= TIGHT, (what, dt, dr)


@pytest.mark.parametrize("kind", ["room", "outdoor", "corridor"])
def test_whole_registration_matches_the_construction_from_its_parts(gpu, oracle, kind):
    from msf_loam_amd import capi
    mc, ms, corner, surf, truth, guess = _world_case(oracle, kind)
    prm = capi.default_params()
    prm.outer_iterations = 1
    h1 = capi.Handle(0, prm)
    h1.set_map(mc, ms)
    s, entry, _ = h1.match_scan2map(corner, surf, guess)            # the entry pose of the last solve
    h1.close()
    assert s == 0
    h = capi.Handle(0)
    h.set_map(mc, ms)
    # control: the same comparison with the feature off
    pose_e, info_e, _ = _expected_solve(h, corner, surf, entry, None, kind + " control")
    s, pose_0, info_0 = h.match_scan2map(corner, surf, guess)
    assert s == 0
    _same_solve(info_0, 1, info_e, pose_0, pose_e, kind + " control")
    # LAST_OUTER
    pose_e, info_e, want = _expected_solve(h, corner, surf, entry, THR, kind + " last outer")
    assert want["n_edge_rejected"] + want["n_plane_rejected"] > 0
    h.set_outlier_rejection(threshold=THR, n=1)
    s, pose_g, info_g = h.match_scan2map(corner, surf, guess)
    r = h.rejection(1)[0]
    h.clear_outlier_rejection()
    assert s == 0 and _slice_is_zero(r, 0)
    _check_record(r, 1, want, kind + " last outer")
    _same_solve(info_g, 1, info_e, pose_g, pose_e, kind + " last outer")
    assert info_g.n_edge[0] == info_0.n_edge[0] and info_g.n_plane[0] == info_0.n_plane[0] and not np.array_equal(pose_g, pose_0)
    # EVERY_OUTER against the chained construction
    pose, wants, infos = np.array(guess, np.float64), [], []
    for it in range(2):
        pose, info_e, want = _expected_solve(h, corner, surf, pose, THR, "%s every outer %d" % (kind, it))
        wants.append(want); infos.append(info_e)
    h.set_outlier_rejection(threshold=THR, which=capi.REJECT_EVERY_OUTER, n=1)
    s, pose_g, info_g = h.match_scan2map(corner, surf, guess)
    r = h.rejection(1)[0]
    assert s == 0
    for it in range(2):
        _check_record(r, it, wants[it], "%s every outer %d" % (kind, it))
        assert info_g.n_edge[it] == infos[it].n_edge[0] and info_g.n_plane[it] == infos[it].n_plane[0]
    _same_solve(info_g, 1, infos[1], pose_g, pose, kind + " every outer")
    h.close()


# ---- 3. the call paths agree bitwise -----------------------------------------------------------------------------------------

MODES = {"threshold": dict(threshold=THR), "fraction": dict(fraction=0.15)}


def _rejected(d):
    return d["n_edge_rejected"].sum(-1) + d["n_plane_rejected"].sum(-1)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_batch_equals_single_calls_and_device_sink_equals_host_sink(gpu, oracle, mode):
    import torch
    from msf_loam_amd import capi
    kw = dict(MODES[mode], which=capi.REJECT_EVERY_OUTER)
    _, mc, ms = common.small_world()
    cs, ss, c, co, s, so, guesses, truths = _batch64(oracle)
    B = 8
    co, so = co[:B + 1], so[:B + 1]
    h = capi.Handle(0)
    h.set_map(mc, ms)
    poses0, st0, info0 = h.match_scan2map_batch(c[:co[B]], co, s[:so[B]], so, guesses[:B], want_info=True)
    h.set_outlier_rejection(n=B, **kw)
    poses, st, info = h.match_scan2map_batch(c[:co[B]], co, s[:so[B]], so, guesses[:B], want_info=True)
    d = h.rejection(B)
    print(mode, "rejected per scan", _rejected(d).tolist())
    assert np.all(_rejected(d) > 0) and np.all(d["valid"] == 1) and not np.array_equal(poses, poses0)
    if mode == "fraction":
        for b in range(B):
            for it in range(2):
                assert d["n_edge_rejected"][b, it] + d["n_plane_rejected"][b, it] == rn.reject_count(d["n_edge_in"][b, it] + d["n_plane_in"][b, it], 0.15)
                assert info[b].n_edge[it] + info[b].n_plane[it] == d["n_edge_in"][b, it] + d["n_plane_in"][b, it] - d["n_edge_rejected"][b, it] - d["n_plane_rejected"][b, it]
    for b in range(B):
        h.set_outlier_rejection(n=1, **kw)
        s1, pose1, info1 = h.match_scan2map(cs[b], ss[b], guesses[b])
        assert s1 == st[b] and np.array_equal(pose1, poses[b]) and bytes(info1) == bytes(info[b]), b
        assert h.rejection(1)[0].tobytes() == d[b].tobytes(), b
    d_sink = torch.zeros(B * capi.REJECTION_DTYPE.itemsize, dtype=torch.uint8, device=torch.device("cuda", 0))
    d_sink.fill_(255)
    torch.cuda.synchronize()
    h.set_outlier_rejection_device(d_sink, B, **kw)
    poses_d, st_d, info_d = h.match_scan2map_batch(c[:co[B]], co, s[:so[B]], so, guesses[:B], want_info=True)
    h.synchronize()
    assert np.array_equal(poses_d, poses) and np.array_equal(st_d, st) and bytes(info_d) == bytes(info)
    assert d_sink.cpu().numpy().tobytes() == d.tobytes()
    h.set_outlier_rejection(n=0, **kw)                               # no sink at all: rejection still runs
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
    h = capi.Handle(0)
    h.set_outlier_rejection(fraction=0.15, n=8)
    poses, status, info = h.match_pairs_batch(mc, mco, ms, mso, c, co, s, so, guesses, want_info=True)
    d = h.rejection(8)
    assert np.all(_rejected(d) > 0)
    for p in range(8):
        single.set_map(mcs[p], mss[p])
        single.set_outlier_rejection(fraction=0.15, n=1)
        st, pose1, info1 = single.match_scan2map(cs[p], ss[p], guesses[p])
        assert st == status[p] == 0 and np.array_equal(pose1, poses[p]) and bytes(info1) == bytes(info[p]), p
        assert single.rejection(1)[0].tobytes() == d[p].tobytes(), p
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
    poses0, _ = h.match_scan2map_deskew_batch(cat(0), co, cat(1), so, cat(2), cat(3), cat(4), cat(5), vel, G, guesses)
    h.set_outlier_rejection(fraction=0.15, n=3)
    poses, status = h.match_scan2map_deskew_batch(cat(0), co, cat(1), so, cat(2), cat(3), cat(4), cat(5), vel, G, guesses)
    d = h.rejection(3)
    assert np.all(status == 0) and np.all(_rejected(d) > 0) and np.all(d["valid"] == [0, 1])
    for b, it in enumerate(items):
        h.set_outlier_rejection(fraction=0.15, n=1)
        s1, p, _ = h.match_scan2map_deskew(it[0], it[1], it[2], it[3], it[4], it[5], it[6], G, it[7])
        assert s1 == 0 and np.array_equal(p, poses[b]), b
        assert h.rejection(1)[0].tobytes() == d[b].tobytes(), b
        assert not np.array_equal(poses[b], poses0[b])
    h.close()


def test_scan2scan_batch_equals_single_and_gating_holds(gpu):
    """A scan-to-scan batch equals the single call bitwise, with something rejected; a pair whose status is not 0 when the last solve's
    rejection runs keeps an all-zero record; survivors under odom_min_correspondences give MSFL_TOO_FEW_CORRESPONDENCES."""
    from msf_loam_amd import capi
    ls, ls_ring, lf, lf_ring, sharp, flat = _scan2scan_inputs(gpu)
    guess = np.array([0.05, -0.03, 0.01, 0, 0, 0.005, 0.9999875])
    h = capi.Handle(0)
    s0, pose0, info0 = h.match_scan2scan(ls, ls_ring, lf, lf_ring, sharp, flat, guess)
    h.set_outlier_rejection(fraction=0.15, n=2)
    s1, pose1, info1 = h.match_scan2scan(ls, ls_ring, lf, lf_ring, sharp, flat, guess)
    d1 = h.rejection(1)[0]
    n_in = int(d1["n_edge_in"][1] + d1["n_plane_in"][1])
    assert s0 == s1 == 0 and not np.array_equal(pose0, pose1) and _slice_is_zero(d1, 0) and d1["valid"][1] == 1
    assert d1["n_edge_rejected"][1] + d1["n_plane_rejected"][1] == rn.reject_count(n_in, 0.15) > 0
    assert info1.n_edge[1] + info1.n_plane[1] == n_in - rn.reject_count(n_in, 0.15)
    few_s, few_f = sharp[:3], flat[:3]
    clouds = [(np.concatenate([ls, ls]), np.concatenate([ls_ring, ls_ring]), [0, len(ls), 2 * len(ls)]),
              (np.concatenate([lf, lf]), np.concatenate([lf_ring, lf_ring]), [0, len(lf), 2 * len(lf)]),
              (np.concatenate([sharp, few_s]), None, [0, len(sharp), len(sharp) + 3]),
              (np.concatenate([flat, few_f]), None, [0, len(flat), len(flat) + 3])]
    poses, status, info = h.match_scan2scan_batch(clouds, np.array([guess, guess]), want_info=True)
    d = h.rejection(2)
    assert list(status) == [0, capi.TOO_FEW_CORRESPONDENCES]
    assert np.array_equal(poses[0], pose1) and bytes(info[0]) == bytes(info1) and d[0].tobytes() == d1.tobytes()
    assert np.array_equal(poses[1], guess) and d[1].tobytes() == ZERO            # failed in the first solve: skipped in front of the last
    # everything rejected: the survivors decide, not the count before the call
    h.set_outlier_rejection(fraction=1.0, which=capi.REJECT_EVERY_OUTER, n=1)
    s2, pose2, info2 = h.match_scan2scan(ls, ls_ring, lf, lf_ring, sharp, flat, guess)
    d2 = h.rejection(1)[0]
    assert s2 == capi.TOO_FEW_CORRESPONDENCES and info2.status == capi.TOO_FEW_CORRESPONDENCES and np.array_equal(pose2, guess)
    assert d2["n_edge_in"][0] + d2["n_plane_in"][0] >= 10 and info2.n_edge[0] == 0 and info2.n_plane[0] == 0 and _slice_is_zero(d2, 1)
    h.close()


def test_mixed_batch_changes_only_the_registrations_with_rejections(gpu, oracle):
    """One batch, a threshold near the largest residual norms (association admits neighbours up to 1 m): some registrations lose
    rows, some none.  The threshold is searched on a fixed grid until the batch is mixed."""
    from msf_loam_amd import capi
    _, mc, ms = common.small_world()
    cs, ss, c, co, s, so, guesses, truths = _batch64(oracle)
    B = 8
    co, so = co[:B + 1], so[:B + 1]
    h = capi.Handle(0)
    h.set_map(mc, ms)
    poses0, st0, info0 = h.match_scan2map_batch(c[:co[B]], co, s[:so[B]], so, guesses[:B], want_info=True)
    found = None
    for thr in np.arange(0.60, 1.0, 0.02):
        h.set_outlier_rejection(threshold=float(thr), n=B)
        poses1, st1, info1 = h.match_scan2map_batch(c[:co[B]], co, s[:so[B]], so, guesses[:B], want_info=True)
        hit = _rejected(h.rejection(B)) > 0
        if hit.any() and not hit.all():
            found = (float(thr), hit, poses1, st1, info1)
            break
    assert found is not None
    thr, hit, poses1, st1, info1 = found
    print("mixed batch at threshold %.2f: registrations with rejections" % thr, hit.tolist())
    assert np.array_equal(st0, st1)
    for b in range(B):
        same = np.array_equal(poses1[b], poses0[b]) and bytes(info1[b]) == bytes(info0[b])
        assert same == (not hit[b]), (b, hit[b])
    h.close()


# ---- 4. off means off ----------------------------------------------------------------------------------------------------------

N_SLAM = 20


def _slam_scans():
    if "slam_scans" not in _cache:
        rp = _rp()
        world = synth.World(ground_half=45.0)
        truth = rp.trajectory(300)[:N_SLAM]
        scans = [synth.make_scan(world, truth[k], synth.SEED + 5000 + k) for k in range(N_SLAM)]
        _cache["slam_scans"] = (rp, world, truth, scans)
    return _cache["slam_scans"]


def _slam_run(tag, pipelined, reject=None, hook=None):
    key = ("slam_run", tag, pipelined)
    if key not in _cache:
        rp, world, truth, scans = _slam_scans()
        out = []
        est, recs, _ = rp.run_slam(world, truth, pipelined=pipelined, scans=scans, reject=reject, reject_out=out, slam_hook=hook)
        _cache[key] = (est, recs, out)
    return _cache[key]


def test_set_and_cleared_equals_a_fresh_handle(gpu, oracle):
    from msf_loam_amd import capi
    mc, ms, corner, surf, truth, guess = _world_case(oracle, "room")
    out = []
    for touched in (False, True):
        h = capi.Handle(0)
        h.set_map(mc, ms)
        if touched:
            h.set_outlier_rejection(fraction=0.5, which=capi.REJECT_EVERY_OUTER, n=1)
            h.match_scan2map(corner, surf, guess)
            h.clear_outlier_rejection()
        s, pose, info = h.match_scan2map(corner, surf, guess)
        scores = h.score_poses(corner, surf, np.array([guess, truth, pose]), 0.5)
        out.append((s, pose.tobytes(), bytes(info), scores.tobytes()))
        h.close()
    assert out[0] == out[1]


def test_slam_set_and_cleared_equals_a_fresh_session(gpu):
    from msf_loam_amd import capi
    cfg = capi.outlier_rejection(fraction=0.5)

    def hook(slam, k):
        if k == 0:
            slam.set_outlier_rejection(cfg, cfg)
            slam.set_outlier_rejection(None, None)
    est0, recs0, _ = _slam_run("off", False)
    est1, recs1, _ = _slam_run("cleared", False, hook=hook)
    assert est0.tobytes() == est1.tobytes()
    for k in range(N_SLAM):
        assert bytes(recs0[k]) == bytes(recs1[k]), k


# ---- 5. gating -------------------------------------------------------------------------------------------------------------------

def test_gating_bad_arguments_and_capacity(gpu, oracle):
    from msf_loam_amd import capi
    _, mc, ms = common.small_world()
    pts, ring, truth, guess = common.scans(1)[0]
    _, corner, surf = common.features_from_oracle(oracle, pts, ring)
    h = capi.Handle(0)
    h.set_map(mc, ms)
    s, pose_ref, info_ref = h.match_scan2map(corner, surf, guess)
    for kw in (dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(fraction=-0.1), dict(fraction=1.5),
               dict(fraction=float("nan")), dict(threshold=0.2, which=7)):
        with pytest.raises(capi.MsflError) as e:
            h.set_outlier_rejection(n=1, **kw)
        assert e.value.status == capi.BAD_ARG, kw
    bad_mode = capi.OutlierRejection(9, 0.2, 0.1, 0)
    assert h.lib.msfl_set_outlier_rejection(h.h, C.byref(bad_mode), None, C.c_int(0), C.c_int(capi.MEM_HOST)) == capi.BAD_ARG
    s, pose, info = h.match_scan2map(corner, surf, guess)                   # the refused calls changed nothing
    assert np.array_equal(pose, pose_ref) and bytes(info) == bytes(info_ref)
    h.set_outlier_rejection(fraction=1.0, n=1)
    # a sink of one record, two registrations: MSFL_CAPACITY before anything is staged or launched
    c2 = np.concatenate([corner, corner]); s2 = np.concatenate([surf, surf])
    co = np.array([0, len(corner), 2 * len(corner)], np.int32); so = np.array([0, len(surf), 2 * len(surf)], np.int32)
    poses = np.array([guess, guess], np.float64)
    status = np.full(2, -7, np.int32)
    h._reject[:] = np.frombuffer(b"\x55" * 56, capi.REJECTION_DTYPE)
    rc = h.lib.msfl_match_scan2map_batch(h.h, C.c_int(2), C.c_void_p(c2.ctypes.data), C.c_void_p(co.ctypes.data), C.c_void_p(s2.ctypes.data),
                                         C.c_void_p(so.ctypes.data), C.c_void_p(poses.ctypes.data), C.c_void_p(status.ctypes.data), None, C.c_int(capi.MEM_HOST))
    assert rc == capi.CAPACITY
    assert np.array_equal(poses, np.array([guess, guess])) and list(status) == [-7, -7]
    assert h._reject.tobytes() == b"\x55" * 56                              # a failing call writes nothing
    # a scan without features: rejection runs on an empty problem, the pose is untouched
    empty = np.zeros((0, 4), np.float32)
    s, pose_e, info_e = h.match_scan2map(empty, empty, guess)
    r = h.rejection(1)[0]
    assert s == 0 and np.array_equal(pose_e, guess) and _slice_is_zero(r, 0) and r["valid"][1] == 1 and r["n_plane_in"][1] == 0
    h.clear_outlier_rejection()
    s, pose, info = h.match_scan2map(corner, surf, guess)
    assert np.array_equal(pose, pose_ref) and bytes(info) == bytes(info_ref)
    h.close()


# ---- 6. the SLAM step ------------------------------------------------------------------------------------------------------------

def test_slam_pipelined_equals_synchronous_and_delivers_both_records(gpu):
    from msf_loam_amd import capi
    cfg = capi.outlier_rejection(fraction=0.15)
    est_s, recs_s, rej_s = _slam_run("fraction", False, reject=(cfg, cfg))
    est_p, recs_p, rej_p = _slam_run("fraction", True, reject=(cfg, cfg))
    est_0, _, _ = _slam_run("off", False)
    assert len(rej_s) == len(rej_p) == N_SLAM
    assert est_p.tobytes() == est_s.tobytes() and not np.array_equal(est_s, est_0)
    n_map = 0
    for k in range(N_SLAM):
        assert _rec_core(recs_p[k]) == _rec_core(recs_s[k]), k
        o, m = rej_s[k]
        assert o.tobytes() == rej_p[k][0].tobytes() and m.tobytes() == rej_p[k][1].tobytes(), k
        if k == 0:
            assert o.tobytes() == ZERO                                       # scan 0 has no scan-to-scan match
        for r, info in ((o, recs_s[k].odometry), (m, recs_s[k].mapping)):
            assert _slice_is_zero(r, 0)                                      # LAST_OUTER
            if r["valid"][1]:
                n_in = int(r["n_edge_in"][1] + r["n_plane_in"][1])
                assert r["n_edge_rejected"][1] + r["n_plane_rejected"][1] == rn.reject_count(n_in, 0.15)
                assert info.n_edge[1] + info.n_plane[1] == n_in - rn.reject_count(n_in, 0.15)
        assert k == 0 or o["valid"][1] == 1, k
        n_map += int(m["valid"][1])
    assert n_map >= N_SLAM // 2


def test_slam_get_rejection_refuses_what_it_cannot_deliver(gpu):
    from msf_loam_amd import capi
    rp, world, truth, scans = _slam_scans()
    slam = capi.Slam(0, max_scan_points=max(len(p) for p, _ in scans), max_rings=16, pose_odom2map=truth[0])
    for bad in (capi.outlier_rejection(threshold=-1.0), capi.outlier_rejection(fraction=2.0), capi.OutlierRejection(5, 0.0, 0.0, 0)):
        with pytest.raises(capi.MsflError) as e:
            slam.set_outlier_rejection(odometry=bad)
        assert e.value.status == capi.BAD_ARG
    slam.add_scan(*scans[0])                                                  # fed with the feature off
    with pytest.raises(capi.MsflError) as e:
        slam.get_rejection(0)
    assert e.value.status == capi.BAD_ARG
    slam.set_outlier_rejection(odometry=capi.outlier_rejection(threshold=THR), mapping=capi.outlier_rejection(fraction=0.1))
    slam.add_scan(*scans[1])
    o, m = slam.get_rejection(1)
    assert o["valid"][1] == 1 or m["valid"][1] == 1
    for k in (2, 7, -1):                                                      # not fed yet / out of range
        with pytest.raises(capi.MsflError) as e:
            slam.get_rejection(k)
        assert e.value.status == capi.BAD_ARG, k
    slam.close()


# ---- 7. the C++ mirror -------------------------------------------------------------------------------------------------------------

def test_cpp_adapter_reproduces_the_ctypes_pose(gpu, oracle, tmp_path):
    from msf_loam_amd import capi
    exe = str(tmp_path / "rejection_check")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "rejection_check.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "msf_loam_amd"), "-lmsfl_hip", "-Wl,-rpath," + os.path.join(ROOT, "msf_loam_amd")])
    mc, ms, corner, surf, truth, guess = _world_case(oracle, "room")
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        for cloud in (mc, ms, corner, surf):
            a = np.ascontiguousarray(cloud, "<f4").reshape(-1, 4)
            f.write(struct.pack("<i", len(a))); f.write(a.tobytes())
        f.write(np.ascontiguousarray(guess, "<f8").tobytes())
        f.write(struct.pack("<d", THR))
    subprocess.check_call([exe, str(fin), str(fout)])
    raw = open(fout, "rb").read()
    assert len(raw) == 56 + 56 + 56
    h = capi.Handle(0)
    h.set_map(mc, ms)
    h.set_outlier_rejection(threshold=THR, n=1)
    s, pose_r, _ = h.match_scan2map(corner, surf, guess)
    r = h.rejection(1)[0]
    h.clear_outlier_rejection()
    s0, pose_0, _ = h.match_scan2map(corner, surf, guess)
    h.close()
    assert s == 0 and s0 == 0 and not np.array_equal(pose_r, pose_0) and _rejected(r) > 0
    assert raw[:56] == pose_r.tobytes()
    assert raw[56:112] == pose_0.tobytes()
    assert raw[112:] == r.tobytes()
