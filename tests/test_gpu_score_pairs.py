"""GPU: the resident pair maps, msfl_set_pair_maps / msfl_score_pairs / msfl_match_pairs_resident.  Every comparison is array_equal
(or bytes), no tolerance: against P x (msfl_set_map(pair p) + msfl_score_poses) on a second handle, against the numpy statement
(tests/score_pairs_numpy.py), and for the registrations against msfl_match_pairs_batch.

One fixture of P = 6 pairs cut from the room world serves all tests:
  maps         corner 4 / 0 / 257 / 1 024 / 2 000 / 5 000 points, surf 5 000 / 300 / 0 / 257 / 1 024 / 2 000: every size of
               0, 4, 257, 1 024, 2 000, 5 000 in the corner kind and all of them but 4 in the surf kind, whose sixth value is the
               300 of the pair with the empty corner map; pairs 0 - 2 are too small to register against, 3 - 5 are not
  scans        0 / 257 / 1 / 255 / 256 / 600 corner and 0 / 255 / 1 / 257 / 256 / 600 surf features: the workgroup edges
  hypotheses   0, 1, 3, 2, 1 and 4 per pair, one of pair 2's with a NaN entry
  offsets      every array starts behind a block of unused leading points / poses
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from msf_loam_amd import synth
from tests import common
from tests import knn_grid_model as gm
from tests import score_numpy as sn
from tests import score_pairs_numpy as spn
from tests.test_gpu_pairs import _cat
from tests.test_gpu_score import _same, _world_scans
from tests.test_score_pairs_model import lattice_pairs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
P = 6
MAP_SIZES = ((4, 5000), (0, 300), (257, 0), (1024, 257), (2000, 1024), (5000, 2000))
SCAN_SIZES = ((0, 0), (257, 255), (1, 1), (255, 257), (256, 256), (600, 600))
N_POSES = (0, 1, 3, 2, 1, 4)
LEAD_POSES = 2


def _cut(map_pts, feat, truth, n):
    """The n points of a map cloud that lie nearest to a feature of the scan at its true pose, in the map's order: a submap of that
    size which the scan still meets."""
    from scipy.spatial import cKDTree
    d, _ = cKDTree(sn.transform_point_f32(truth, feat[:, :3]).astype(np.float64)).query(map_pts[:, :3].astype(np.float64))
    return np.ascontiguousarray(map_pts[np.sort(np.argsort(d, kind="stable")[:n])])


class Pairs:
    """The fixture: per-pair lists, and the concatenated arrays with their offsets as the calls take them."""

    def __init__(self):
        _, mc, ms = common.small_world()
        rng = np.random.default_rng(31)
        mc_pool = np.concatenate([mc + F(0.03 * k) for k in range(4)])          # the room's corner map has 1 380 points
        scans = _world_scans("room")
        self.maps_c, self.maps_s, self.corners, self.surfs, self.poses, self.guesses = [], [], [], [], [], []
        for p in range(P):
            corner0, surf0, truth = scans[p % len(scans)]
            self.maps_c.append(_cut(mc_pool, corner0, truth, MAP_SIZES[p][0])); self.maps_s.append(_cut(ms, surf0, truth, MAP_SIZES[p][1]))
            cpool = np.concatenate([corner0 + F(0.03 * k) for k in range(4)])   # a scan has fewer than 255 corner features
            self.corners.append(cpool[rng.permutation(len(cpool))[:SCAN_SIZES[p][0]]])
            self.surfs.append(surf0[rng.permutation(len(surf0))[:SCAN_SIZES[p][1]]])
            self.poses.append(np.array(([truth] + [synth.perturb_pose(truth, rng) for _ in range(N_POSES[p])])[:N_POSES[p]]).reshape(-1, 7))
            self.guesses.append(synth.perturb_pose(truth, rng))
        self.poses[2][1, 5] = np.nan                                            # its neighbours must not notice
        assert [tuple(map(len, x)) for x in zip(self.maps_c, self.maps_s)] == list(MAP_SIZES)
        assert [tuple(map(len, x)) for x in zip(self.corners, self.surfs)] == list(SCAN_SIZES) and [len(x) for x in self.poses] == list(N_POSES)
        self.guesses = np.array(self.guesses)
        self.MC, self.mco = _cat(self.maps_c, lead=17); self.MS, self.mso = _cat(self.maps_s, lead=5)
        self.C, self.co = _cat(self.corners, lead=3); self.S, self.so = _cat(self.surfs, lead=9)
        self.H = np.concatenate([np.full((LEAD_POSES, 7), 0.5)] + self.poses)
        self.po = np.cumsum([LEAD_POSES] + list(N_POSES)).astype(np.int32)

    def score(self, h, max_dist, want_nn=True, arrays=None):
        """score_pairs over the fixture (arrays: its clouds and poses as device tensors): the records of the used poses (, d2, nn)."""
        corner, surf, poses = arrays or (self.C, self.S, self.H)
        out = h.score_pairs(corner, self.co, surf, self.so, poses, self.po, max_dist, want_nn=want_nn)
        rec = out[0] if want_nn else out
        assert not rec[:LEAD_POSES].tobytes().strip(b"\0")                       # records in front of pose_off[0] are not written
        return ((rec[LEAD_POSES:],) + tuple(out[1:])) if want_nn else rec[LEAD_POSES:]


@functools.lru_cache(maxsize=None)
def _pairs():
    return Pairs()


@functools.lru_cache(maxsize=None)
def _model_case(max_dist):
    x = _pairs()
    return spn.score_pairs(spn.models(x.maps_c, x.maps_s), x.corners, x.surfs, x.poses, max_dist)


@functools.lru_cache(maxsize=None)
def _loop_case(max_dist):
    """P x (set_map(pair p) + score_poses) on a handle of its own: the records and the flat per-feature outputs."""
    from msf_loam_amd import capi
    x = _pairs()
    h = capi.Handle(0)
    try:
        recs, d2s, nns = [np.zeros(0, capi.POSE_SCORE_DTYPE)], [np.zeros(0, F)], [np.zeros(0, np.int32)]
        for p in range(P):
            if N_POSES[p] == 0:
                continue
            h.set_map(x.maps_c[p], x.maps_s[p])
            rec, d2, nn = h.score_poses(x.corners[p], x.surfs[p], x.poses[p], max_dist, want_nn=True)
            recs.append(rec); d2s.append(d2.reshape(-1)); nns.append(nn.reshape(-1))
        return np.concatenate(recs), np.concatenate(d2s), np.concatenate(nns)
    finally:
        h.close()


def _equal(got, want, what):
    _same(got[0], want[0], what)
    assert got[1].shape == want[1].shape and got[2].shape == want[2].shape, what
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), what


@pytest.fixture(scope="module")
def resident(gpu):
    """A handle whose pair index was built by msfl_set_pair_maps over the fixture's maps."""
    from msf_loam_amd import capi
    x = _pairs()
    h = capi.Handle(0)
    h.set_pair_maps(x.MC, x.mco, x.MS, x.mso)
    yield h
    h.close()


@pytest.mark.parametrize("max_dist", [1.0, 0.05])
def test_records_equal_single_calls_and_the_model(resident, max_dist):
    from msf_loam_amd import capi
    x = _pairs()
    got = x.score(resident, max_dist)
    loop, model = _loop_case(max_dist), _model_case(max_dist)
    starts, total = spn.row_starts(x.corners, x.surfs, x.poses)
    assert len(got[0]) == sum(N_POSES) and len(got[1]) == total == len(loop[1]) == len(model[1])
    _equal(got, loop, "P x (set_map + score_poses)")
    _equal(got, model, "the numpy model")
    _same(x.score(resident, max_dist, want_nn=False), model[0], "no per-feature outputs")
    rec = got[0]
    print("max_dist %.2f: inliers per hypothesis %s" % (max_dist, rec["inliers"].tolist()))
    # pair 1: the empty corner map gives zero corner inliers, its 300 surf points some surf inliers at 1 m
    assert rec["inliers"][0, 0] == 0 and rec["sum_sq_q32"][0, 0] == 0 and (got[2][starts[0]:starts[0] + 257] == -1).all()
    # pair 2's NaN hypothesis: BAD_ARG, zero record, +inf / -1 rows; its neighbours are scored
    assert rec["status"].tolist() == [0, 0, capi.BAD_ARG] + [0] * 8 and not rec["inliers"][2].any()
    assert np.isposinf(got[1][starts[2]:starts[3]]).all() and (got[2][starts[2]:starts[3]] == -1).all()
    if max_dist == 1.0:
        assert rec["inliers"][0, 1] > 0 and rec["inliers"][7:, :].min() > 0
        # own-cloud indices: every hit of pair 5 lies inside its own clouds and AT the reported distance
        for kind, (m, feat, at) in enumerate(((x.maps_c[5], x.corners[5], 0), (x.maps_s[5], x.surfs[5], 600))):
            nn, d2 = got[2][starts[7] + at:starts[7] + at + 600], got[1][starts[7] + at:starts[7] + at + 600]
            hit = nn >= 0
            assert nn.max() < len(m) and hit.sum() == rec["inliers"][7, kind]
            q = sn.transform_point_f32(x.poses[5][0], feat[:, :3])
            assert np.array_equal(gm.l2_simple(m[nn[hit], :3], q[hit]), d2[hit])


def test_the_index_match_pairs_batch_left_serves_score_pairs(gpu):
    from msf_loam_amd import capi
    x = _pairs()
    h = capi.Handle(0)
    try:
        h.match_pairs_batch(x.MC, x.mco, x.MS, x.mso, x.C, x.co, x.S, x.so, x.guesses)
        for max_dist in (1.0, 0.05):
            _equal(x.score(h, max_dist), _model_case(max_dist), "after match_pairs_batch, max_dist %g" % max_dist)
    finally:
        h.close()


def _reg(out, unc=None):
    poses, status, info = out
    return (poses.tobytes(), np.asarray(status).tobytes(), bytes(info)) + (() if unc is None else (unc.tobytes(),))


@pytest.mark.parametrize("uncertainty", [False, True])
def test_match_pairs_resident_equals_match_pairs_batch(gpu, uncertainty):
    from msf_loam_amd import capi
    x = _pairs()
    a, b = capi.Handle(0), capi.Handle(0)
    try:
        if uncertainty:
            a.set_uncertainty(P); b.set_uncertainty(P)
        unc = lambda h: h.uncertainty() if uncertainty else None
        ref_out = a.match_pairs_batch(x.MC, x.mco, x.MS, x.mso, x.C, x.co, x.S, x.so, x.guesses, want_info=True)
        ref = _reg(ref_out, unc(a))
        poses, status, info = ref_out
        assert status.tolist() == [capi.MAP_TOO_SMALL] * 3 + [0] * 3 and np.array_equal(poses[:3], x.guesses[:3])
        print("edges / planes of the second outer iteration:", [(info[p].n_edge[1], info[p].n_plane[1]) for p in range(P)])
        assert not (poses[3:] == x.guesses[3:]).all(1).any() and info[5].n_plane[1] > 0
        b.set_pair_maps(x.MC, x.mco, x.MS, x.mso)
        run = lambda h: _reg(h.match_pairs_resident(x.C, x.co, x.S, x.so, x.guesses, want_info=True), unc(h))
        assert run(b) == ref, "first call"
        assert run(b) == ref, "second call in a row: the index is not consumed"
        _same(x.score(b, 1.0)[0], _model_case(1.0)[0], "scoring between registrations")
        assert run(b) == ref, "after a score_pairs call"
        # and on the index the batch call left on its own handle
        assert run(a) == ref, "on the index match_pairs_batch left"
    finally:
        a.close(); b.close()


def test_ties_and_duplicates_resolve_in_each_pairs_own_cloud(gpu):
    from msf_loam_amd import capi
    maps_c, maps_s, corners, surfs, poses = lattice_pairs()
    MC, mco = _cat(maps_c, lead=2); MS, mso = _cat(maps_s, lead=11)
    Cc, co = _cat(corners); S, so = _cat(surfs, lead=4)
    Hp, po = np.concatenate(poses), np.cumsum([0] + [len(p) for p in poses]).astype(np.int32)
    h = capi.Handle(0)
    try:
        h.set_pair_maps(MC, mco, MS, mso)
        for max_dist in (1.0, 0.5):
            got = h.score_pairs(Cc, co, S, so, Hp, po, max_dist, want_nn=True)
            want = spn.score_pairs(spn.models(maps_c, maps_s), corners, surfs, poses, max_dist)
            _equal(got, want, max_dist)
        assert (got[2] >= 0).sum() > 100
    finally:
        h.close()


def test_grown_cells_give_the_same_records(resident, monkeypatch):
    from msf_loam_amd import capi
    x = _pairs()
    cap = 512
    steps = lambda m, c: gm.desc_of(m, c).steps
    assert min(steps(x.maps_c[5], cap), steps(x.maps_s[5], cap)) >= 2
    assert steps(x.maps_s[5], cap) > steps(x.maps_s[5], max(4096, 2 * len(x.maps_s[5])))         # (the slice a pair gets by default)
    monkeypatch.setenv("MSFL_GRID_CAP_CELLS", str(cap))
    h = capi.Handle(0)
    monkeypatch.delenv("MSFL_GRID_CAP_CELLS")
    try:
        h.set_pair_maps(x.MC, x.mco, x.MS, x.mso)
        for max_dist in (1.0, 0.05):
            got = x.score(h, max_dist)
            _equal(got, x.score(resident, max_dist), "default cells")
            _equal(got, _model_case(max_dist), "the numpy model")
    finally:
        h.close()


def test_device_memory_equals_host_memory(resident):
    import torch
    from msf_loam_amd import capi
    x = _pairs()
    dev = torch.device("cuda", 0)
    h = capi.Handle(0)
    try:
        side = torch.cuda.Stream(dev)
        h.set_stream(side.cuda_stream)
        with torch.cuda.stream(side):
            d_mc, d_ms = torch.from_numpy(x.MC).to(dev), torch.from_numpy(x.MS).to(dev)
            d_c, d_s, d_p = torch.from_numpy(x.C).to(dev), torch.from_numpy(x.S).to(dev), torch.from_numpy(x.H).to(dev)
            side.synchronize()
            h.set_pair_maps_device(P, d_mc, x.mco, d_ms, x.mso)
            # the index holds its own sorted copy: once the stream has passed the call the caller's clouds may change
            d_mc.zero_(); d_ms.zero_()
            for max_dist in (1.0, 0.05):
                _equal(x.score(h, max_dist, arrays=(d_c, d_s, d_p)), x.score(resident, max_dist), "device = host, max_dist %g" % max_dist)
                _same(x.score(h, max_dist, want_nn=False, arrays=(d_c, d_s, d_p)), _model_case(max_dist)[0], "device memory, no outputs")
            # the registrations: device arrays in, the host call's bytes out
            ref, ref_status, _ = resident.match_pairs_resident(x.C, x.co, x.S, x.so, x.guesses)
            d_g = torch.from_numpy(x.guesses).to(dev)
            d_status = torch.full((P,), -1, dtype=torch.int32, device=dev)
            h.match_pairs_resident_device(P, d_c, x.co, d_s, x.so, d_g, d_status)
            h.synchronize()
            assert np.array_equal(d_g.cpu().numpy(), ref) and np.array_equal(d_status.cpu().numpy(), ref_status)
    finally:
        h.close()


def test_refusals(gpu):
    from msf_loam_amd import capi
    x = _pairs()
    _, mc, ms = common.small_world()

    def status(call):
        try:
            call()
            return capi.OK
        except capi.MsflError as e:
            return e.status

    score = lambda h, max_dist=1.0: status(lambda: x.score(h, max_dist, want_nn=False))
    match = lambda h: status(lambda: h.match_pairs_resident(x.C, x.co, x.S, x.so, x.guesses))
    h = capi.Handle(0)
    try:
        # no pair index yet; a single map is none
        assert score(h) == capi.NO_MAP and match(h) == capi.NO_MAP
        h.set_map(mc, ms)
        assert score(h) == capi.NO_MAP and match(h) == capi.NO_MAP
        h.set_pair_maps(x.MC, x.mco, x.MS, x.mso)
        assert score(h) == capi.OK and match(h) == capi.OK
        # ... and the pair index is no single map
        assert status(lambda: h.score_poses(x.corners[5], x.surfs[5], x.poses[5], 1.0)) == capi.NO_MAP
        assert status(lambda: h.score_poses_batch(x.C, x.co, x.S, x.so, x.H, x.po, 1.0)) == capi.NO_MAP
        assert status(lambda: h.match_scan2map(x.corners[5], x.surfs[5], x.guesses[5])) == capi.NO_MAP
        # msfl_set_map takes the arrays back
        h.set_map(mc, ms)
        assert score(h) == capi.NO_MAP and match(h) == capi.NO_MAP
        h.set_pair_maps(x.MC, x.mco, x.MS, x.mso)
        # P differs from the resident index
        assert status(lambda: h.score_pairs(x.C, x.co[:-1], x.S, x.so[:-1], x.H, x.po[:-1], 1.0)) == capi.BAD_ARG
        assert status(lambda: h.match_pairs_resident(x.C, x.co[:-1], x.S, x.so[:-1], x.guesses[:-1])) == capi.BAD_ARG
        # null and decreasing offsets
        lib, vp, mem = h.lib, capi._vp, C.c_int(capi.MEM_HOST)
        rec = np.zeros(len(x.H), capi.POSE_SCORE_DTYPE)
        for k in range(3):
            offs = [vp(x.co), vp(x.so), vp(x.po)]; offs[k] = None
            assert lib.msfl_score_pairs(h.h, C.c_int(P), vp(x.C), offs[0], vp(x.S), offs[1], vp(x.H), offs[2], C.c_double(1.0), vp(rec), None, None,
                                        mem) == capi.BAD_ARG
        st, g = np.zeros(P, np.int32), x.guesses.copy()
        assert lib.msfl_match_pairs_resident(h.h, C.c_int(P), vp(x.C), None, vp(x.S), vp(x.so), vp(g), vp(st), None, mem) == capi.BAD_ARG
        assert lib.msfl_match_pairs_resident(h.h, C.c_int(P), vp(x.C), vp(x.co), vp(x.S), vp(x.so), None, vp(st), None, mem) == capi.BAD_ARG
        down = x.co.copy(); down[3] = down[2] - 1
        assert status(lambda: h.score_pairs(x.C, down, x.S, x.so, x.H, x.po, 1.0)) == capi.BAD_ARG
        assert status(lambda: h.score_pairs(x.C, x.co, x.S, x.so, x.H, x.po[::-1].copy(), 1.0)) == capi.BAD_ARG
        assert status(lambda: h.match_pairs_resident(x.C, down, x.S, x.so, x.guesses)) == capi.BAD_ARG
        assert score(h) == capi.OK and match(h) == capi.OK                        # none of that touched the index
        # max_dist as in msfl_score_poses
        for bad in (0.0, -1.0, float("nan"), float(np.nextafter(1.0, 2.0)), 8.5, float("inf")):
            assert score(h, bad) == capi.BAD_ARG, bad
        assert score(h, 1e-3) == capi.OK
        # a failed msfl_set_pair_maps leaves no pair index behind
        assert lib.msfl_set_pair_maps(h.h, C.c_int(P), vp(x.MC), None, vp(x.MS), vp(x.mso), mem) == capi.BAD_ARG
        assert status(lambda: h.set_pair_maps(x.MC, x.mco[::-1].copy(), x.MS, x.mso)) == capi.BAD_ARG
        assert score(h) == capi.OK                                                # refused before anything was touched
        many = np.zeros(65537, np.int32)
        assert status(lambda: h.set_pair_maps(x.MC, many, x.MS, many)) == capi.CAPACITY and "65535" in h.lib.msfl_last_error(h.h).decode()
        assert score(h) == capi.OK
    finally:
        h.close()
    # a build that fails after the checks (the pairs' cell tables exceed 2^31 cells together: refused from the host offsets alone, in
    # front of any launch; device memory, so that nothing is staged either) leaves no pair index behind
    import torch
    h = capi.Handle(0)
    try:
        h.set_pair_maps(x.MC, x.mco, x.MS, x.mso)
        n = 65535
        d_pts = torch.zeros((8, 4), dtype=torch.float32, device="cuda:0")
        off = (np.arange(n + 1, dtype=np.int64) * (1 << 14)).astype(np.int32)
        assert status(lambda: h.set_pair_maps_device(n, d_pts, off, d_pts, np.zeros(n + 1, np.int32))) == capi.CAPACITY
        assert score(h) == capi.NO_MAP
    finally:
        h.close()


def test_cpp_mirror_gives_the_ctypes_bytes(resident, tmp_path):
    from msf_loam_amd import capi
    exe = str(tmp_path / "score_pairs_check")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "score_pairs_check.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "msf_loam_amd"), "-lmsfl_hip", "-Wl,-rpath," + os.path.join(ROOT, "msf_loam_amd")])
    x = _pairs()
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.int32(P).tobytes())
        for p in range(P):
            for cloud in (x.maps_c[p], x.maps_s[p], x.corners[p], x.surfs[p]):
                f.write(np.int32(len(cloud)).tobytes()); f.write(np.ascontiguousarray(cloud, F).tobytes())
            f.write(np.asarray(x.guesses[p], np.float64).tobytes())
            f.write(np.int32(N_POSES[p]).tobytes()); f.write(np.ascontiguousarray(x.poses[p], np.float64).tobytes())
        f.write(np.float64(1.0).tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw = open(tmp_path / "out.bin", "rb").read()
    n = sum(N_POSES)
    assert len(raw) == n * 32 + P * 4 + P * 56 + P * 32
    here = x.score(resident, 1.0, want_nn=False)
    assert raw[:n * 32] == here.tobytes()
    _same(np.frombuffer(raw[:n * 32], capi.POSE_SCORE_DTYPE), _model_case(1.0)[0])
    poses, status, _ = resident.match_pairs_resident(x.C, x.co, x.S, x.so, x.guesses)
    at = n * 32
    assert raw[at:at + P * 4] == status.astype(np.int32).tobytes() and raw[at + P * 4:at + P * 60] == poses.tobytes()
    after = resident.score_pairs(x.C, x.co, x.S, x.so, poses, np.arange(P + 1, dtype=np.int32), 1.0)
    assert raw[at + P * 60:] == after.tobytes()
