"""GPU: msfl_score_poses / msfl_score_poses_batch against the numpy model (tests/score_numpy.py).  The model is the specification:
every comparison is array_equal on the four record fields (and on d2_out / nn_out where they are asked for), no tolerance.

  room            four scans of the room world at sixteen poses each (truth, perturbed, far off, outside the map, a NaN pose),
                  max_dist 1.0 and 0.05, with the per-feature outputs
  lattice         the lattice map of tests/knn_grid_cases.py (equal f32 distances, duplicated points) plus queries AT the
                  threshold (inlier) and one f32 step beyond it (miss)
  edges           0 / 1 / 255 / 256 / 257 features per kind, a scan without hypotheses in the middle of a batch, and 65 537
                  hypotheses in one call (two launches)
  grown cells     a handle whose cell table is capped so that the index takes at least two growth steps
  forms           batch = loop of single calls; device memory on a side stream = host memory; a call right after an asynchronous
                  device msfl_set_map sees the new map
  refusals, non-interference with the matcher, ranking of a position x yaw lattice, the C++ mirror
"""
import functools
import os
import subprocess

import numpy as np
import pytest

from msf_loam_amd import synth
from tests import common
from tests import knn_grid_cases as kc
from tests import knn_grid_model as gm
from tests import score_numpy as sn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FIELDS = ("inliers", "sum_sq_q32", "status", "reserved_")
IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1.0])


def _same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f, np.flatnonzero((got[f] != want[f]).reshape(len(got), -1).any(1))[:8])


def _yawed(pose, deg, dxyz=(0.0, 0.0, 0.0)):
    """`pose` moved by dxyz and turned by `deg` about the world's z axis."""
    out = np.array(pose, np.float64)
    out[:3] += dxyz
    a = np.deg2rad(deg) / 2.0
    q = synth.quat_mul(np.array([0.0, 0.0, np.sin(a), np.cos(a)]), out[3:])
    out[3:] = q / np.linalg.norm(q)
    return out


@functools.lru_cache(maxsize=None)
def _world_scans(kind, n=4):
    """(corner, surf, truth) of n scans of the world: features straight from the ray-cast hit kinds, voxel down-sampled."""
    w, _, _ = common.other_world(kind)
    out = []
    for i, (_, _, truth, _) in enumerate(common.other_scans(kind, n)):
        pts, _, hit = synth.make_scan(w, truth, synth.SEED + 12 + i, with_kind=True)
        corner, surf = synth.direct_features(pts, hit)
        out.append((corner, surf, truth))
    return out


@functools.lru_cache(maxsize=None)
def _model(kind):
    _, mc, ms = common.other_world(kind)
    return sn.Model(mc, ms)


def _sixteen(truth, rng):
    poses = [truth] + [synth.perturb_pose(truth, rng) for _ in range(6)] + [synth.perturb_pose(truth, rng, max_t=1.0, max_deg=10.0) for _ in range(5)]
    poses.append(_yawed(truth, 90.0, (2.0, 0.0, 0.0)))
    poses.append(_yawed(truth, 0.0, (500.0, 0.0, 0.0)))              # outside the map's box
    bad = np.array(truth); bad[4] = np.nan
    poses.append(bad)                                                 # its neighbours must not notice
    poses.append(synth.perturb_pose(truth, rng))
    return np.array(poses)


@functools.lru_cache(maxsize=None)
def _room_case(max_dist):
    rng = np.random.default_rng(23)
    out = []
    for corner, surf, truth in _world_scans("room"):
        poses = _sixteen(truth, rng)
        out.append((corner, surf, poses, _model("room").score(corner, surf, poses, max_dist, want_nn=True)))
    return out


@pytest.fixture(scope="module")
def room(gpu):
    from msf_loam_amd import capi
    _, mc, ms = common.small_world()
    h = capi.Handle(0)
    h.set_map(mc, ms)
    yield h
    h.close()


@pytest.mark.parametrize("max_dist", [1.0, 0.05])
def test_room_world_sixteen_poses_per_scan(room, max_dist):
    from msf_loam_amd import capi
    for i, (corner, surf, poses, (rec_m, d2_m, nn_m)) in enumerate(_room_case(max_dist)):
        rec, d2, nn = room.score_poses(corner, surf, poses, max_dist, want_nn=True)
        nf = len(corner) + len(surf)
        print("scan %d: %d + %d features, max_dist %.2f: fitness truth %.4f, 2 m / 90 deg off %.4f, outside %.4f; rmse truth %.4f m"
              % (i, len(corner), len(surf), max_dist, capi.fitness(rec, len(corner), len(surf))[0], capi.fitness(rec, len(corner), len(surf))[12],
                 capi.fitness(rec, len(corner), len(surf))[13], capi.rmse(rec)[0]))
        _same(rec, rec_m, "scan %d" % i)
        assert np.array_equal(nn, nn_m) and np.array_equal(d2, d2_m)
        assert rec["status"][14] == capi.BAD_ARG and rec["inliers"][14].sum() == 0 and rec["sum_sq_q32"][14].sum() == 0
        assert (nn[14] == -1).all() and np.isposinf(d2[14]).all()
        assert rec["inliers"][13].sum() == 0 and (rec["status"][[13, 15]] == 0).all()
        assert np.array_equal(capi.fitness(rec, len(corner), len(surf)), sn.fitness(rec_m, nf))
        if max_dist == 1.0:
            assert capi.fitness(rec, len(corner), len(surf))[0] >= 0.95 and rec["inliers"][15].sum() > 0
        # without the per-feature outputs: the same records
        _same(room.score_poses(corner, surf, poses, max_dist), rec_m, "scan %d, no outputs" % i)


def test_ties_duplicates_and_the_gate(gpu):
    from msf_loam_amd import capi
    c = kc.case("lattice")
    # Identity pose (the transform is exact).  (0, 0, -0.5) is exactly 1 m above the lattice node (0, 0, -1.5): d2 == thr, an inlier.
    # Moved aside by 2^-11.5 m, fl(dx * dx) is 2^-23 to a rounding and 1 + that rounds to the f32 after 1: a miss.  The same
    # 0.5 m in front of the pole's (0, 0, 0) for the corner kind and max_dist 0.5 (thr = 0.25, whose next f32 is 0.25 + 2^-25).
    at, dx1, dx05 = F(-0.5), F(2.0 ** -11.5), F(2.0 ** -12.5)
    node, foot = np.array([0, 0, -1.5], F), np.zeros(3, F)
    extra_s = np.array([[0, 0, at], [dx1, 0, at], [0.25, 0, at]], F)
    extra_c = np.array([[at, 0, 0], [at, dx05, 0], [np.nextafter(at, F(0.0)), 0, 0]], F)
    assert gm.l2_simple(node, extra_s).tolist() == [F(1.0), np.nextafter(F(1.0), F(2.0)), F(1.0625)]
    assert gm.l2_simple(foot, extra_c[:2]).tolist() == [F(0.25), np.nextafter(F(0.25), F(1.0))] and gm.l2_simple(foot, extra_c[2]) < F(0.25)
    surf, corner = np.concatenate([c.surf, kc.pts4(extra_s)]), np.concatenate([c.corner, kc.pts4(extra_c)])
    poses = np.array(list(c.poses) + [IDENTITY])
    model = sn.Model(c.mc, c.ms)
    h = capi.Handle(0)
    try:
        h.set_map(c.mc, c.ms)
        for max_dist in (1.0, 0.5, 0.25):
            rec, d2, nn = h.score_poses(corner, surf, poses, max_dist, want_nn=True)
            rec_m, d2_m, nn_m = model.score(corner, surf, poses, max_dist, want_nn=True)
            _same(rec, rec_m, max_dist)
            assert np.array_equal(nn, nn_m) and np.array_equal(d2, d2_m)
        # the gate itself, spelled out (identity pose = last row)
        rec, d2, nn = h.score_poses(corner, surf, poses, 1.0, want_nn=True)
        s0 = len(corner) + len(c.surf)
        assert d2[-1, s0] == F(1.0) and nn[-1, s0] >= 0 and np.array_equal(c.ms[nn[-1, s0], :3], node)
        assert np.isposinf(d2[-1, s0 + 1:s0 + 3]).all() and (nn[-1, s0 + 1:s0 + 3] == -1).all()
        rec, d2, nn = h.score_poses(corner, surf, poses, 0.5, want_nn=True)
        c0 = len(c.corner)
        assert d2[-1, c0] == F(0.25) and nn[-1, c0] == 0 and np.isposinf(d2[-1, c0 + 1]) and nn[-1, c0 + 1] == -1
        assert nn[-1, c0 + 2] == 0 and d2[-1, c0 + 2] < F(0.25)              # towards the pole: nearer; (0, 0, 0) is there twice, index 0 wins
        assert np.array_equal(c.mc[0, :3], foot) and (c.mc[1:, :3] == foot).all(1).any()
        assert (nn_m[-1] >= 0).sum() > 100
    finally:
        h.close()


def _edge_batch():
    corner0, surf0, truth = _world_scans("room")[0]
    cpool = np.concatenate([corner0, corner0 + F(0.03)])              # a scan has fewer than 255 corner features
    rng = np.random.default_rng(5)
    counts = [(0, 0), (1, 0), (0, 1), (255, 257), (256, 256), (257, 255), (1, 1), (300, 0), (0, 300)]
    n_poses = [2, 3, 1, 3, 0, 3, 2, 1, 2]                              # scan 4 (256 + 256 features) has no hypothesis
    cs, ss, ps = [], [], []
    for (nc, ns), npose in zip(counts, n_poses):
        cs.append(cpool[rng.permutation(len(cpool))[:nc]]); ss.append(surf0[rng.permutation(len(surf0))[:ns]])
        ps.append(np.array([synth.perturb_pose(truth, rng) for _ in range(npose)]).reshape(-1, 7))
    return cs, ss, ps


def _offsets(parts):
    return np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)


def test_workgroup_edges_and_a_scan_without_hypotheses(room):
    cs, ss, ps = _edge_batch()
    assert min(len(c) for c in cs) == 0 and sorted({len(c) for c in cs} & {255, 256, 257}) == [255, 256, 257]
    want = np.concatenate([_model("room").score(c, s, p, 1.0) for c, s, p in zip(cs, ss, ps)])
    got = room.score_poses_batch(np.concatenate(cs), _offsets(cs), np.concatenate(ss), _offsets(ss), np.concatenate(ps), _offsets(ps), 1.0)
    _same(got, want)
    assert got["inliers"].sum() > 500
    # the scan without hypotheses now gets three: its records are its own, the others' do not move
    ps2 = list(ps); ps2[4] = ps[3]
    got2 = room.score_poses_batch(np.concatenate(cs), _offsets(cs), np.concatenate(ss), _offsets(ss), np.concatenate(ps2), _offsets(ps2), 1.0)
    o = _offsets(ps2)
    _same(np.concatenate([got2[:o[4]], got2[o[5]:]]), want)
    _same(got2[o[4]:o[5]], _model("room").score(cs[4], ss[4], ps2[4], 1.0))
    # no scan, no pose: nothing to do
    z = np.zeros((0, 4), F)
    assert len(room.score_poses(cs[3], ss[3], np.zeros((0, 7)), 1.0)) == 0
    assert len(room.score_poses_batch(z, [0], z, [0], np.zeros((0, 7)), [0], 1.0)) == 0


def test_more_hypotheses_than_one_launch_holds(room):
    corner0, surf0, truth = _world_scans("room")[0]
    rng = np.random.default_rng(6)
    corner, surf = corner0[rng.permutation(len(corner0))[:40]], surf0[rng.permutation(len(surf0))[:88]]
    base = np.array([synth.perturb_pose(truth, rng, max_t=0.6, max_deg=5.0) for _ in range(16)])
    n = 65537
    poses = base[np.arange(n) % 16]
    rec, d2, nn = room.score_poses(corner, surf, poses, 1.0, want_nn=True)
    rec16, d216, nn16 = _model("room").score(corner, surf, base, 1.0, want_nn=True)
    _same(rec, rec16[np.arange(n) % 16])
    assert np.array_equal(nn, nn16[np.arange(n) % 16]) and np.array_equal(d2, d216[np.arange(n) % 16])
    assert len({tuple(r["inliers"]) + tuple(r["sum_sq_q32"]) for r in rec16}) > 8          # the sixteen are not all alike
    for row in (65534, 65535, 65536):                                                       # the last row of the first launch, the second launch
        one, d2_1, nn_1 = room.score_poses(corner, surf, poses[row:row + 1], 1.0, want_nn=True)
        _same(rec[row:row + 1], one, row)
        assert np.array_equal(d2[row], d2_1[0]) and np.array_equal(nn[row], nn_1[0])


def test_grown_cells_give_the_same_records(room, monkeypatch):
    from msf_loam_amd import capi
    _, mc, ms = common.small_world()
    cap = 512
    steps = (gm.desc_of(mc, cap).steps, gm.desc_of(ms, cap).steps)
    assert min(steps) >= 2, steps
    assert gm.desc_of(ms, gm.DEFAULT_CAP).steps == 0
    monkeypatch.setenv("MSFL_GRID_CAP_CELLS", str(cap))
    h = capi.Handle(0)
    monkeypatch.delenv("MSFL_GRID_CAP_CELLS")
    try:
        h.set_map(mc, ms)
        for max_dist in (1.0, 0.05):
            for corner, surf, poses, (rec_m, d2_m, nn_m) in _room_case(max_dist)[:2]:
                rec, d2, nn = h.score_poses(corner, surf, poses, max_dist, want_nn=True)
                rec_d, d2_d, nn_d = room.score_poses(corner, surf, poses, max_dist, want_nn=True)
                _same(rec, rec_d); _same(rec, rec_m)
                assert np.array_equal(nn, nn_d) and np.array_equal(d2, d2_d)
    finally:
        h.close()


def test_batch_equals_single_calls_and_device_equals_host(room):
    import torch
    from msf_loam_amd import capi
    case = _room_case(1.0)
    cs, ss, ps = [c[0] for c in case], [c[1] for c in case], [c[2][:5 + i] for i, c in enumerate(case)]
    loop = np.concatenate([room.score_poses(c, s, p, 1.0) for c, s, p in zip(cs, ss, ps)])
    _same(loop, np.concatenate([c[3][0][:5 + i] for i, c in enumerate(case)]))
    C, S, P = np.concatenate(cs), np.concatenate(ss), np.concatenate(ps)
    co, so, po = _offsets(cs), _offsets(ss), _offsets(ps)
    _same(room.score_poses_batch(C, co, S, so, P, po, 1.0), loop, "batch")
    # offsets that do not start at zero: scans 1 and 2 of the arrays, records at their poses' places
    part = room.score_poses_batch(C, co[1:4], S, so[1:4], P, po[1:4], 1.0)
    _same(part[po[1]:po[3]], loop[po[1]:po[3]], "inner scans")
    assert not part[:po[1]]["inliers"].any() and not part[po[3]:]["inliers"].any()
    dev = torch.device("cuda", 0)
    _, mc, ms = common.small_world()
    h = capi.Handle(0)
    try:
        side = torch.cuda.Stream(dev)
        h.set_stream(side.cuda_stream)
        with torch.cuda.stream(side):
            d_c, d_s, d_p = torch.from_numpy(C).to(dev), torch.from_numpy(S).to(dev), torch.from_numpy(P).to(dev)
            d_mc, d_ms = torch.from_numpy(mc).to(dev), torch.from_numpy(ms).to(dev)
            # a shifted copy of the map: what the handle holds first
            d_mc2, d_ms2 = d_mc.clone(), d_ms.clone()
            d_mc2[:, 0] += 0.25; d_ms2[:, 0] += 0.25
            side.synchronize()
            h.set_map(d_mc2, d_ms2, len(mc), len(ms), capi.MEM_DEVICE)
            shifted = h.score_poses_batch(d_c, co, d_s, so, d_p, po, 1.0)
            # asynchronous device set_map, scored at once: the new map
            h.set_map(d_mc, d_ms, len(mc), len(ms), capi.MEM_DEVICE)
            got = h.score_poses_batch(d_c, co, d_s, so, d_p, po, 1.0)
            _same(got, loop, "device batch on a side stream")
            assert not np.array_equal(shifted["sum_sq_q32"], loop["sum_sq_q32"])
            mc2, ms2 = mc.copy(), ms.copy(); mc2[:, 0] += F(0.25); ms2[:, 0] += F(0.25)
            room2 = sn.Model(mc2, ms2).score(cs[0], ss[0], ps[0], 1.0)
            _same(shifted[:po[1]], room2, "the shifted map")
            rec, d2, nn = h.score_poses(d_c[co[1]:co[2]], d_s[so[1]:so[2]], d_p[po[1]:po[2]], 1.0, want_nn=True)
            _same(rec, loop[po[1]:po[2]], "device single")
            assert np.array_equal(nn, case[1][3][2][:len(ps[1])]) and np.array_equal(d2, case[1][3][1][:len(ps[1])])
    finally:
        h.close()


def test_refusals(room):
    from msf_loam_amd import capi
    from tests.test_gpu_pairs import _cat
    corner, surf, truth = _world_scans("room")[0]
    _, mc, ms = common.small_world()

    def status(h, max_dist=1.0):
        try:
            h.score_poses(corner, surf, [truth], max_dist)
            return capi.OK
        except capi.MsflError as e:
            return e.status

    h = capi.Handle(0)
    try:
        assert status(h) == capi.NO_MAP
        h.set_map(mc, ms)
        assert status(h) == capi.OK
        # the pairs call replaces the resident single map
        C, co = _cat([corner]); S, so = _cat([surf]); MC, mco = _cat([mc]); MS, mso = _cat([ms])
        h.match_pairs_batch(MC, mco, MS, mso, C, co, S, so, [truth])
        assert status(h) == capi.NO_MAP
        h.set_map(mc, ms)
        for bad in (0.0, -1.0, float("nan"), float(np.nextafter(1.0, 2.0)), 8.5, float("inf")):
            assert status(h, bad) == capi.BAD_ARG, bad
        assert status(h, 1.0) == capi.OK and status(h, 1e-3) == capi.OK
        # a map side without points: zero inliers of that kind, not an error
        h.set_map(mc[:0], ms)
        rec = h.score_poses(corner, surf, [truth], 1.0)
        assert rec["inliers"][0, 0] == 0 and rec["sum_sq_q32"][0, 0] == 0
        _same(rec, sn.Model(mc[:0], ms).score(corner, surf, [truth], 1.0))
        assert rec["inliers"][0, 1] == _room_case(1.0)[0][3][0]["inliers"][0, 1]
    finally:
        h.close()
    # a wider index admits a wider threshold, up to 8 m
    p = capi.default_params(); p.map_knn_max_sq_dist = 100.0
    h = capi.Handle(0, p)
    try:
        h.set_map(mc, ms)
        assert status(h, 8.0) == capi.OK and status(h, 8.01) == capi.BAD_ARG
        _same(h.score_poses(corner, surf, [truth], 1.0), _room_case(1.0)[0][3][0][:1], "cells of 10 m")
    finally:
        h.close()


def test_scoring_leaves_the_matcher_alone(gpu):
    from msf_loam_amd import capi
    _, mc, ms = common.small_world()
    corner, surf, poses, _ = _room_case(1.0)[0]
    corner2, surf2, poses2, _ = _room_case(1.0)[1]
    guess = poses[1]
    out = []
    for score_first in (False, True):
        h = capi.Handle(0)
        try:
            h.set_map(mc, ms)
            if score_first:
                h.score_poses(corner2, surf2, poses2, 1.0, want_nn=True)
                h.score_poses_batch(corner2, [0, len(corner2)], surf2, [0, len(surf2)], poses2, [0, len(poses2)], 0.05)
            s, pose, info = h.match_scan2map(corner, surf, guess)
            out.append((s, pose.tobytes(), bytes(info)))
            if score_first:                                       # and between two matcher calls
                h.score_poses(corner, surf, poses, 1.0)
            s, pose, info = h.match_scan2map(corner2, surf2, poses2[2])
            out.append((s, pose.tobytes(), bytes(info)))
        finally:
            h.close()
    assert out[0] == out[2] and out[1] == out[3] and out[0][0] == 0 and out[1][0] == 0


def _lattice(truth):
    poses = [truth]
    for dx in (-3.0, -1.5, 0.0, 1.5, 3.0):
        for dy in (-3.0, -1.5, 0.0, 1.5, 3.0):
            for j in range(12):
                poses.append(_yawed(truth, 30.0 * j + 4.0, (0.4 + dx, -0.3 + dy, 0.0)))
    return np.array(poses)


@pytest.mark.parametrize("i", range(4))
@pytest.mark.parametrize("kind", ["room", "outdoor"])
def test_ranking_a_position_yaw_lattice(gpu, kind, i):
    from msf_loam_amd import capi
    _, mc, ms = common.other_world(kind)
    corner, surf, truth = _world_scans(kind)[i]
    poses = _lattice(truth)
    assert len(poses) == 301
    want = _model(kind).score(corner, surf, poses, 1.0)
    gpu.set_map(mc, ms)
    got = gpu.score_poses(corner, surf, poses, 1.0)
    fit = capi.fitness(got, len(corner), len(surf))
    order = np.lexsort((np.arange(301), -fit))
    print("%s scan %d: %d + %d features; fitness truth %.4f, best lattice pose %.4f (rmse %.3f m), median %.4f"
          % (kind, i, len(corner), len(surf), fit[0], fit[1:].max(), capi.rmse(got)[1 + int(np.argmax(fit[1:]))], np.median(fit[1:])))
    _same(got, want)
    fit_m = sn.fitness(want, len(corner) + len(surf))
    assert np.array_equal(order, np.lexsort((np.arange(301), -fit_m))) and order[0] == 0
    assert fit[0] >= 0.95 and fit[1:].max() <= 0.90


def test_cpp_mirror_scores_like_ctypes(room, tmp_path):
    from msf_loam_amd import capi
    exe = str(tmp_path / "score_check")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "score_check.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "msf_loam_amd"), "-lmsfl_hip", "-Wl,-rpath," + os.path.join(ROOT, "msf_loam_amd")])
    _, mc, ms = common.small_world()
    corner, surf, poses, (rec_m, _, _) = _room_case(1.0)[0]
    with open(tmp_path / "in.bin", "wb") as f:
        for cloud in (mc, ms, corner, surf):
            f.write(np.int32(len(cloud)).tobytes()); f.write(np.ascontiguousarray(cloud, F).tobytes())
        f.write(np.asarray(poses[1], np.float64).tobytes()); f.write(np.float64(1.0).tobytes())
        f.write(np.int32(len(poses)).tobytes()); f.write(np.ascontiguousarray(poses, np.float64).tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw = open(tmp_path / "out.bin", "rb").read()
    n = len(poses)
    assert len(raw) == n * 32 + n * 16
    rec = np.frombuffer(raw[:n * 32], capi.POSE_SCORE_DTYPE)
    here = room.score_poses(corner, surf, poses, 1.0)
    assert rec.tobytes() == here.tobytes()
    _same(rec, rec_m)
    fr = np.frombuffer(raw[n * 32:], np.float64).reshape(n, 2)
    assert np.array_equal(fr[:, 0], capi.fitness(here, len(corner), len(surf)))
    assert np.array_equal(fr[:, 1], capi.rmse(here), equal_nan=True)
