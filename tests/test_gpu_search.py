"""GPU: msfl_search_poses and msfl_relocalize against the numpy model (tests/search_numpy.py) and against the public calls they
are made of.  Every comparison is array_equal / tobytes(): hits over the WHOLE lattice, candidates, poses.  No tolerance anywhere.
The shapes are those of tests/search_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import search_cases as sc
from tests import search_numpy as sn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _config(cfg):
    from msf_loam_amd import capi
    return capi.SearchConfig(step=cfg.step, half=cfg.half, n_yaw=cfg.n_yaw, yaw_min=cfg.yaw_min, yaw_step=cfg.yaw_step, yaw_wraps=cfg.yaw_wraps,
                             dilate=cfg.dilate, range=cfg.range, nms_cells=cfg.nms_cells, nms_yaws=cfg.nms_yaws,
                             max_volume_bytes=cfg.max_volume_bytes)


def _same_candidates(got, want):
    assert got.dtype == want.dtype and len(got) == len(want), (len(got), len(want))
    for name in ("h", "a", "kx", "ky", "kz", "hits", "reserved_"):
        assert np.array_equal(got[name], want[name]), name
    assert got["pose"].tobytes() == want["pose"].tobytes()
    assert got.tobytes() == want.tobytes()


def _run(gpu, case, device=False):
    mc, ms, c, s, guess, cfg, K = case
    gpu.set_map(mc, ms)
    if device:
        import torch
        c, s = torch.from_numpy(c).to("cuda:0"), torch.from_numpy(s).to("cuda:0")
    return gpu.search_poses(c, s, guess, _config(cfg), capacity=K, want_hits=True)


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_hits_and_candidates_equal_the_model(gpu, name):
    case = sc.CASES[name]()
    mc, ms, c, s, guess, cfg, K = case
    want_cand, want_hits = sn.search(mc, ms, c, s, guess, cfg, K)
    cand, hits = _run(gpu, case)
    assert hits.shape == want_hits.shape and hits.dtype == np.int32
    assert np.array_equal(hits, want_hits)
    _same_candidates(cand, want_cand)


@pytest.mark.parametrize("name", ["random", "nonfinite", "half_x_64", "lattice_67240", "map_0"])
def test_device_memory_equals_the_model(gpu, name):
    case = sc.CASES[name]()
    mc, ms, c, s, guess, cfg, K = case
    want_cand, want_hits = sn.search(mc, ms, c, s, guess, cfg, K)
    cand, hits = _run(gpu, case, device=True)
    assert np.array_equal(hits, want_hits)
    _same_candidates(cand, want_cand)


def test_device_slots_past_n_out_are_zero(gpu):
    """Device memory gets all `capacity` slots: the found candidates, then zeros, never what an earlier search left in scratch."""
    import torch
    from msf_loam_amd import capi
    busy = sc.PEAK_CASES["busy_K1024"]()                                               # windows 0 / 0: all 75 hypotheses are peaks
    gpu.set_map(busy[0], busy[1])
    assert len(gpu.search_poses(busy[2], busy[3], busy[4], _config(busy[5]), capacity=64)) == 64    # scratch now holds 64 records
    mc, ms, c, s, guess, cfg, _ = sc.PEAK_CASES["cells2_yaws2_wrap1_K1"]()
    want = sn.search(mc, ms, c, s, guess, cfg, 64)[0]
    assert 0 < len(want) < 8
    gpu.set_map(mc, ms)
    size = capi.POSE_CANDIDATE_DTYPE.itemsize
    cand = torch.full((64 * size,), 0xff, dtype=torch.uint8, device="cuda:0")
    n_out = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
    gpu.search_poses_device(torch.from_numpy(c).to("cuda:0"), len(c), torch.from_numpy(s).to("cuda:0"), len(s), guess, _config(cfg), cand, 64, n_out)
    gpu.synchronize()
    raw = cand.cpu().numpy()
    assert int(n_out.item()) == len(want)
    _same_candidates(raw.view(capi.POSE_CANDIDATE_DTYPE)[:len(want)], want)
    assert not raw[len(want) * size:].any()


def _example(args, cwd):
    run = subprocess.run([sys.executable] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    return run


def test_relocalize_example_runs_with_places(tmp_path):
    """examples/relocalize.py is what this test is about: the lattice centred on the best capi.Places entry, through to an accepted pose."""
    out = _example([os.path.join(ROOT, "examples", "relocalize.py"), "--places", "--half", "4", "4", "0", "--candidates", "8", "--refine", "3"],
                   str(tmp_path)).stdout
    assert "best place: entry" in out and "refined (msfl_relocalize):" in out and "accepted pose:" in out


def test_replay_relocalizes_in_a_saved_map(tmp_path):
    """examples/replay_synthetic.py --load-map --relocalize is what this test is about: scan 0 is anchored where msfl_relocalize puts
    it in the map that a first run saved (mapio), and the run goes on from there."""
    import json
    replay = os.path.join(ROOT, "examples", "replay_synthetic.py")
    prefix = str(tmp_path / "map")
    _example([replay, "--scans", "4", "--save-map", prefix], str(tmp_path))
    run = _example([replay, "--scans", "4", "--load-map", prefix, "--relocalize"], str(tmp_path))
    assert "relocalised scan 0 from a guess 1.50 m / 34 deg off" in run.stderr
    res = json.loads(run.stdout.strip().splitlines()[-1])
    print(run.stderr.strip().splitlines()[-1], "| ate", res["ate_rmse_m"])
    # anchored by the search, not by the truth: still within the lattice pitch of it over the whole run
    assert res["load_map"] == prefix and res["ate_rmse_m"] < 0.5


@pytest.mark.parametrize("name", sorted(sc.PEAK_CASES))
def test_peaks_and_top_k_equal_the_model(gpu, name):
    case = sc.PEAK_CASES[name]()
    mc, ms, c, s, guess, cfg, K = case
    want_cand, want_hits = sn.search(mc, ms, c, s, guess, cfg, K)
    n_peaks = int(sn.peaks_window(want_hits, cfg).sum())
    assert len(want_cand) == min(K, n_peaks)
    cand, hits = _run(gpu, case)
    assert np.array_equal(hits, want_hits)
    _same_candidates(cand, want_cand)
    if name.startswith("all_zero"):
        assert not hits.any() and np.array_equal(cand["h"], np.sort(cand["h"]))          # the order is by index
    # without the hits the candidates are the same
    gpu.set_map(mc, ms)
    _same_candidates(gpu.search_poses(c, s, guess, _config(cfg), capacity=K), want_cand)


@pytest.fixture(scope="module", params=["room", "outdoor"])
def world(request, gpu):
    f = sc.fixture(request.param)
    gpu.set_map(f["mc"], f["ms"])
    return request.param, f


def test_room_fixture_search_equals_the_model(gpu):
    """One call on the room fixture: some 5 k features, 1 944 hypotheses."""
    f = sc.fixture("room")
    want_cand, want_hits = sn.search(f["mc"], f["ms"], f["corner"], f["surf"], f["guess"], f["cfg"], 16)
    gpu.set_map(f["mc"], f["ms"])
    cand, hits = gpu.search_poses(f["corner"], f["surf"], f["guess"], _config(f["cfg"]), capacity=16, want_hits=True)
    assert hits.shape == (2, 1944) and len(f["corner"]) + len(f["surf"]) > 5000
    assert np.array_equal(hits, want_hits)
    _same_candidates(cand, want_cand)


def _chain(gpu, f, K, max_dist, n_refine, min_fitness):
    """msfl_relocalize, chained by the caller from the four public calls."""
    from msf_loam_amd import capi
    corner, surf = f["corner"], f["surf"]
    cand = gpu.search_poses(corner, surf, f["guess"], _config(f["cfg"]), capacity=K)
    coarse = gpu.score_poses(corner, surf, cand["pose"], max_dist)
    key = lambda rec: np.lexsort((np.arange(len(rec)), rec["sum_sq_q32"].sum(1), -rec["inliers"].sum(1).astype(np.int64)))
    order = key(coarse)[:n_refine]
    n = len(order)
    co, so = np.arange(n + 1, dtype=np.int32) * len(corner), np.arange(n + 1, dtype=np.int32) * len(surf)
    refined, status, _ = gpu.match_scan2map_batch(np.tile(corner, (n, 1)), co, np.tile(surf, (n, 1)), so, cand["pose"][order])
    fine = gpu.score_poses(corner, surf, refined, max_dist)
    out = np.zeros(n, capi.RELOC_RESULT_DTYPE)
    for i, r in enumerate(key(fine)):
        out[i]["pose"], out[i]["candidate"], out[i]["coarse"], out[i]["refined"] = refined[r], cand[order[r]], coarse[order[r]], fine[r]
        out[i]["status"] = status[r]
        out[i]["accepted"] = int(fine[r]["inliers"].sum() / float(len(corner) + len(surf)) >= min_fitness)
    return out, cand, order, refined


def test_relocalize_equals_the_chain_of_public_calls(gpu, world):
    import torch
    from msf_loam_amd import synth
    kind, f = world
    gpu.set_map(f["mc"], f["ms"])
    want, cand, order, refined = _chain(gpu, f, 16, 1.0, 5, 0.5)
    got = gpu.relocalize(f["corner"], f["surf"], f["guess"], _config(f["cfg"]), n_candidates=16, max_dist=1.0, n_refine=5, min_fitness=0.5)
    assert len(got) == 5 and got.tobytes() == want.tobytes()
    dev = gpu.relocalize(torch.from_numpy(f["corner"]).to("cuda:0"), torch.from_numpy(f["surf"]).to("cuda:0"), f["guess"], _config(f["cfg"]),
                         n_candidates=16, max_dist=1.0, n_refine=5, min_fitness=0.5)
    assert dev.tobytes() == want.tobytes()
    # the accepted pose is the registration started from the winning candidate
    best = got[0]
    assert best["accepted"] == 1 and best["status"] == 0
    one, st, _ = gpu.match_scan2map_batch(f["corner"], [0, len(f["corner"])], f["surf"], [0, len(f["surf"])], [best["candidate"]["pose"]])
    assert st[0] == 0 and one[0].tobytes() == best["pose"].tobytes()
    dt, dr = synth.pose_error(best["pose"], f["truth"])
    print(kind, "accepted pose: |dt| %.4f m, |dr| %.4f deg, fitness %.4f" % (dt, np.rad2deg(dr), best["refined"]["inliers"].sum() / float(len(f["corner"]) + len(f["surf"]))))
    # a relocalisation has to beat the lattice it searched: closer to the truth than one cell and half a yaw step (how close the
    # matcher itself gets from a candidate is its own business, pinned by its own tests)
    assert dt < f["cfg"].step and dr < 0.5 * f["cfg"].yaw_step


def test_calls_after_a_search_are_unchanged(gpu, world):
    kind, f = world
    corner, surf = f["corner"], f["surf"]
    gpu.set_map(f["mc"], f["ms"])
    start = sn.pose(f["guess"], f["cfg"], 2, (-2, 2, 0))
    args = (corner, [0, len(corner)], surf, [0, len(surf)], [start])
    poses0, st0, _ = gpu.match_scan2map_batch(*args)
    rec0 = gpu.score_poses(corner, surf, [start, poses0[0]], 1.0)
    gpu.search_poses(corner, surf, f["guess"], _config(f["cfg"]), capacity=16, want_hits=True)
    poses1, st1, _ = gpu.match_scan2map_batch(*args)
    gpu.search_poses(corner, surf, f["guess"], _config(f["cfg"]), capacity=16)
    rec1 = gpu.score_poses(corner, surf, [start, poses0[0]], 1.0)
    assert poses0.tobytes() == poses1.tobytes() and np.array_equal(st0, st1) and rec0.tobytes() == rec1.tobytes()


def _mirror_case():
    case = sc.random_case(70, n_map=(300, 500), n_feat=(60, 90), half=(3, 3, 1), n_yaw=5, K=8)
    start = sn.pose(case[4], case[5], 0)
    return case, start


def test_cpp_mirror_searches_like_ctypes(gpu, tmp_path):
    from msf_loam_amd import capi
    exe = str(tmp_path / "search_check")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "search_check.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "msf_loam_amd"), "-lmsfl_hip", "-Wl,-rpath," + os.path.join(ROOT, "msf_loam_amd")])
    (mc, ms, c, s, guess, cfg, K), start = _mirror_case()
    with open(tmp_path / "in.bin", "wb") as f:
        for cloud in (mc, ms, c, s):
            f.write(np.int32(len(cloud)).tobytes()); f.write(np.ascontiguousarray(cloud, np.float32).tobytes())
        f.write(np.asarray(start, np.float64).tobytes()); f.write(np.asarray(guess, np.float64).tobytes())
        f.write(bytes(_config(cfg)))
        f.write(np.int32(K).tobytes()); f.write(np.int32(K).tobytes()); f.write(np.float64(1.0).tobytes())
        f.write(np.int32(3).tobytes()); f.write(np.float64(0.5).tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw = open(tmp_path / "out.bin", "rb").read()
    n = int(np.frombuffer(raw[:4], np.int32)[0])
    cand = np.frombuffer(raw[4:4 + 88 * n], capi.POSE_CANDIDATE_DTYPE)
    m = int(np.frombuffer(raw[4 + 88 * n:8 + 88 * n], np.int32)[0])
    res = np.frombuffer(raw[8 + 88 * n:], capi.RELOC_RESULT_DTYPE)
    assert len(res) == m
    gpu.set_map(mc, ms)
    here = gpu.search_poses(c, s, guess, _config(cfg), capacity=K)
    assert n == len(here) > 0 and cand.tobytes() == here.tobytes()
    _same_candidates(cand, sn.search(mc, ms, c, s, guess, cfg, K)[0])
    here_r = gpu.relocalize(c, s, guess, _config(cfg), n_candidates=K, max_dist=1.0, n_refine=3, min_fitness=0.5)
    assert m == len(here_r) > 0 and res.tobytes() == here_r.tobytes()


def test_c_mirror_searches_like_ctypes(gpu, tmp_path):
    import ctypes
    from msf_loam_amd import capi
    so = str(tmp_path / "libsearch_check_c.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "search_check_c.c"), "-o", so,
                           "-L" + os.path.join(ROOT, "msf_loam_amd"), "-lmsfl_hip", "-Wl,-rpath," + os.path.join(ROOT, "msf_loam_amd")])
    fn = ctypes.CDLL(so).search_check_c
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    (mc, ms, c, s, guess, cfg, K), _ = _mirror_case()
    gpu.set_map(mc, ms)
    want, want_hits = gpu.search_poses(c, s, guess, _config(cfg), capacity=K, want_hits=True)
    want_r = gpu.relocalize(c, s, guess, _config(cfg), n_candidates=K, max_dist=1.0, n_refine=3, min_fitness=0.5)
    cand, hits = np.zeros(K, capi.POSE_CANDIDATE_DTYPE), np.zeros_like(want_hits)
    res, n_res = np.zeros(3, capi.RELOC_RESULT_DTYPE), np.zeros(1, np.int32)
    c, s, ccfg = np.ascontiguousarray(c, np.float32), np.ascontiguousarray(s, np.float32), _config(cfg)
    n = fn(gpu.h, c.ctypes.data, len(c), s.ctypes.data, len(s), guess.ctypes.data, ctypes.addressof(ccfg), cand.ctypes.data, K,
           hits.ctypes.data, res.ctypes.data, 3, n_res.ctypes.data)
    assert n == len(want) > 0 and cand[:n].tobytes() == want.tobytes() and np.array_equal(hits, want_hits)
    assert n_res[0] == len(want_r) > 0 and res[:n_res[0]].tobytes() == want_r.tobytes()


def test_refusals(gpu):
    from msf_loam_amd import capi
    mc, ms, c, s, guess, cfg, K = sc.CASES["random"]()
    fresh = capi.Handle(0)
    try:
        with pytest.raises(capi.MsflError) as e:
            fresh.search_poses(c, s, guess, _config(cfg))
        assert e.value.status == capi.NO_MAP
        with pytest.raises(capi.MsflError) as e:
            fresh.relocalize(c, s, guess, _config(cfg))
        assert e.value.status == capi.NO_MAP
        fresh.set_pair_maps(mc, [0, len(mc)], ms, [0, len(ms)])
        with pytest.raises(capi.MsflError) as e:
            fresh.search_poses(c, s, guess, _config(cfg))
        assert e.value.status == capi.NO_MAP                                            # a pair index is resident
        fresh.set_map(mc, ms)
        want = sn.search(mc, ms, c, s, guess, cfg, K)[0]
        for kw, status in ((dict(capacity=0), capi.BAD_ARG), (dict(capacity=1025), capi.BAD_ARG)):
            with pytest.raises(capi.MsflError) as e:
                fresh.search_poses(c, s, guess, _config(cfg), **kw)
            assert e.value.status == status, kw
        tiny = _config(cfg); tiny.max_volume_bytes = 64
        with pytest.raises(capi.MsflError) as e:
            fresh.search_poses(c, s, guess, tiny)
        assert e.value.status == capi.CAPACITY
        bad = guess.copy(); bad[1] = np.nan
        with pytest.raises(capi.MsflError) as e:
            fresh.search_poses(c, s, bad, _config(cfg))
        assert e.value.status == capi.BAD_ARG
        zero = _config(cfg); zero.step = 0.0
        with pytest.raises(capi.MsflError) as e:
            fresh.search_poses(c, s, guess, zero)
        assert e.value.status == capi.BAD_ARG
        for kw in (dict(n_candidates=0), dict(n_candidates=4, n_refine=5), dict(n_refine=0), dict(min_fitness=np.nan)):
            with pytest.raises(capi.MsflError) as e:
                fresh.relocalize(c, s, guess, _config(cfg), **kw)
            assert e.value.status == capi.BAD_ARG, kw
        _same_candidates(fresh.search_poses(c, s, guess, _config(cfg), capacity=K), want)    # the refusals left the handle usable
    finally:
        fresh.close()
