"""GPU: msfl_search_pairs against the numpy model (tests/search_numpy.py applied pair by pair) and against the public single-map
calls it is defined by.  Every comparison is array_equal / tobytes(): hits over the WHOLE lattice of every pair, candidates,
counts.  No tolerance anywhere.  The shapes are those of tests/search_pairs_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import search_cases as sc
from tests import search_numpy as sn
from tests import search_pairs_cases as spc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAD = {"ragged3": (3, 5)}          # rows in front of the first pair's features: offsets that do not start at 0


def _config(cfg, **kw):
    from msf_loam_amd import capi
    c = capi.SearchConfig(step=cfg.step, half=cfg.half, n_yaw=cfg.n_yaw, yaw_min=cfg.yaw_min, yaw_step=cfg.yaw_step, yaw_wraps=cfg.yaw_wraps,
                          dilate=cfg.dilate, range=cfg.range, nms_cells=cfg.nms_cells, nms_yaws=cfg.nms_yaws, max_volume_bytes=cfg.max_volume_bytes)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _same_candidates(got, want):
    assert got.dtype == want.dtype and len(got) == len(want), (len(got), len(want))
    for name in ("h", "a", "kx", "ky", "kz", "hits", "reserved_"):
        assert np.array_equal(got[name], want[name]), name
    assert got["pose"].tobytes() == want["pose"].tobytes()
    assert got.tobytes() == want.tobytes()


def _set_maps(h, case, order=None):
    order = range(case.P) if order is None else order
    mc, mco = spc.concat([case.mc[p] for p in order], lead=2)            # (map offsets that do not start at 0 either)
    ms, mso = spc.concat([case.ms[p] for p in order])
    h.set_pair_maps(mc, mco, ms, mso)


def _scans(case, order=None, lead=(0, 0)):
    order = range(case.P) if order is None else order
    c, co = spc.concat([case.c[p] for p in order], lead=lead[0])
    s, so = spc.concat([case.s[p] for p in order], lead=lead[1])
    return c, co, s, so, np.array([case.guess[p] for p in order])


def _search(h, case, order=None, lead=(0, 0), device=False, want_hits=True, K=None):
    c, co, s, so, guesses = _scans(case, order, lead)
    if device:
        import torch
        c, s = torch.from_numpy(c).to("cuda:0"), torch.from_numpy(s).to("cuda:0")
    return h.search_pairs(c, co, s, so, guesses, _config(case.cfg), capacity=case.K if K is None else K, want_hits=want_hits)


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("name", sorted(spc.CASES))
def test_equals_the_model(gpu, name, mem):
    case = spc.CASES[name]()
    want_cand, want_hits = spc.model(name, case)
    _set_maps(gpu, case)
    cand, hits = _search(gpu, case, lead=LEAD.get(name, (0, 0)), device=mem == "device")
    assert hits.shape == want_hits.shape and hits.dtype == np.int32 and len(cand) == case.P
    for p in range(case.P):
        assert np.array_equal(hits[p], want_hits[p]), p
        _same_candidates(cand[p], want_cand[p])
    if name == "ragged3":
        assert not want_hits[0, 0].any() and want_hits[0, 1].any()        # the empty corner map: no corner hits, surf hits as ever
        assert want_hits[1, 0].any() and not want_hits[1, 1].any()        # no surf features
        assert not want_hits[2].any() and len(want_cand[2]) > 0           # the empty pair: all-zero lattice, its peaks by index
    if name.startswith("peaks_K"):
        n_peaks = [int(sn.peaks_window(want_hits[p], case.cfg).sum()) for p in range(case.P)]
        assert [len(c) for c in want_cand] == [min(case.K, n) for n in n_peaks] and all(n == 630 for n in n_peaks)
    # without the hits the candidates are the same
    if mem == "host":
        for p, c in enumerate(_search(gpu, case, lead=LEAD.get(name, (0, 0)), want_hits=False)):
            _same_candidates(c, want_cand[p])


def _few_peaks():
    return spc.pairs_case([dict(seed=60, n_map=(3, 4), n_feat=(9, 12)), dict(seed=1), dict(seed=61, n_map=(3, 4), n_feat=(9, 12))], K=64, half=(3, 2, 1),
                          n_yaw=6, yaw_step=2 * np.pi / 6, yaw_wraps=1, nms_cells=2, nms_yaws=2)


def test_slots_past_n_out(gpu):
    """Device memory gets all `capacity` slots of every pair: the found candidates, then zeros, never what an earlier search left in
    scratch.  Host memory: the slots past n_out[p] are left alone."""
    import torch
    from msf_loam_amd import capi
    busy = spc.pairs_case([dict(seed=62), dict(seed=63), dict(seed=64)], K=64, half=(3, 2, 1), n_yaw=6, nms_cells=0, nms_yaws=0)
    _set_maps(gpu, busy)
    assert [len(c) for c in _search(gpu, busy, want_hits=False)] == [64, 64, 64]          # scratch now holds 3 x 64 records
    case = _few_peaks()
    want = spc.model("few_peaks", case)[0]
    assert all(0 < len(w) < 64 for w in want)
    _set_maps(gpu, case)
    c, co, s, so, guesses = _scans(case)
    size = capi.POSE_CANDIDATE_DTYPE.itemsize
    cand = torch.full((case.P * 64 * size,), 0xff, dtype=torch.uint8, device="cuda:0")
    n_out = torch.full((case.P,), -1, dtype=torch.int32, device="cuda:0")
    gpu.search_pairs_device(case.P, torch.from_numpy(c).to("cuda:0"), co, torch.from_numpy(s).to("cuda:0"), so, guesses, _config(case.cfg), cand, 64, n_out)
    gpu.synchronize()
    raw = cand.cpu().numpy().reshape(case.P, 64 * size)
    assert n_out.cpu().numpy().tolist() == [len(w) for w in want]
    for p in range(case.P):
        _same_candidates(raw[p].view(capi.POSE_CANDIDATE_DTYPE)[:len(want[p])], want[p])
        assert not raw[p, len(want[p]) * size:].any(), p
    host = np.full((case.P, 64 * size), 0xff, np.uint8)
    n_host = np.full(case.P, -1, np.int32)
    cfg = _config(case.cfg)
    import ctypes
    assert gpu.lib.msfl_search_pairs(gpu.h, case.P, c.ctypes.data, co.ctypes.data, s.ctypes.data, so.ctypes.data, guesses.ctypes.data, ctypes.addressof(cfg),
                                     host.ctypes.data, 64, n_host.ctypes.data, None, capi.MEM_HOST) == capi.OK
    assert n_host.tolist() == [len(w) for w in want]
    for p in range(case.P):
        _same_candidates(host[p].view(capi.POSE_CANDIDATE_DTYPE)[:len(want[p])], want[p])
        assert (host[p, len(want[p]) * size:] == 0xff).all(), p


def test_chunks_of_two_equal_one_chunk(gpu, monkeypatch):
    """MSFL_SEARCH_CHUNK_PAIRS is read when a handle is made: five pairs as 2 + 2 + 1 give the bytes of five pairs at once."""
    from msf_loam_amd import capi
    case = spc.FIVE()
    want_cand, want_hits = spc.model("five", case)
    _set_maps(gpu, case)
    whole = {mem: _search(gpu, case, device=mem == "device") for mem in ("host", "device")}
    monkeypatch.setenv("MSFL_SEARCH_CHUNK_PAIRS", "2")
    h = capi.Handle(0)
    try:
        _set_maps(h, case)
        for mem in ("host", "device"):
            cand, hits = _search(h, case, device=mem == "device")
            assert hits.tobytes() == whole[mem][1].tobytes() and np.array_equal(hits, want_hits), mem
            for p in range(case.P):
                assert cand[p].tobytes() == whole[mem][0][p].tobytes(), (mem, p)
                _same_candidates(cand[p], want_cand[p])
    finally:
        h.close()


def test_equals_the_public_single_calls(gpu):
    """Three pairs, the first the room fixture the single-map test accepts: set_map(pair p) + search_poses per pair writes the same
    bytes; match_pairs_resident from each pair's first candidate is match_scan2map from it."""
    from msf_loam_amd import capi
    case = spc.ROOM()
    _set_maps(gpu, case)
    cand, hits = _search(gpu, case)
    assert hits.shape == (3, 2, 1944) and all(len(c) > 0 for c in cand)
    c, co, s, so, _ = _scans(case)
    first = np.array([cand[p][0]["pose"] for p in range(case.P)])
    poses, status, _ = gpu.match_pairs_resident(c, co, s, so, first)
    single = capi.Handle(0)
    try:
        for p in range(case.P):
            single.set_map(case.mc[p], case.ms[p])
            one, one_hits = single.search_poses(case.c[p], case.s[p], case.guess[p], _config(case.cfg), capacity=case.K, want_hits=True)
            assert np.array_equal(hits[p], one_hits), p
            _same_candidates(cand[p], one)
            st, pose, _ = single.match_scan2map(case.c[p], case.s[p], first[p])
            assert st == status[p] == 0 and np.array_equal(np.asarray(pose), poses[p]), p
    finally:
        single.close()
    f = sc.fixture("room")
    _same_candidates(cand[0], sn.search(f["mc"], f["ms"], f["corner"], f["surf"], f["guess"], f["cfg"], 16)[0])


def test_permuting_the_pairs_permutes_the_outputs(gpu):
    case = spc.CASES["far_and_negative"]()
    _set_maps(gpu, case)
    cand, hits = _search(gpu, case)
    order = [2, 0, 1]
    _set_maps(gpu, case, order)
    cand2, hits2 = _search(gpu, case, order)
    for at, p in enumerate(order):
        assert np.array_equal(hits2[at], hits[p]) and cand2[at].tobytes() == cand[p].tobytes(), (at, p)


def _registrations(h, case, with_unc):
    c, co, s, so, guesses = _scans(case)
    poses, status, _ = h.match_pairs_resident(c, co, s, so, guesses)
    unc = h.uncertainty(case.P).tobytes() if with_unc else b""
    rec = h.score_pairs(c, co, s, so, np.stack([guesses, poses], 1).reshape(-1, 7), 2 * np.arange(case.P + 1), 1.0)     # pair p: its guess, its result
    return poses.tobytes(), np.asarray(status).tobytes(), rec.tobytes(), unc


@pytest.mark.parametrize("how", ["set_pair_maps", "uncertainty", "match_pairs_batch"])
def test_calls_after_a_search_are_unchanged(how):
    """match_pairs_resident and score_pairs before and after a search_pairs (with and without hits) are byte-equal: with the
    uncertainty sink on, and on the index a match_pairs_batch left."""
    from msf_loam_amd import capi
    case = spc.FIVE()
    h = capi.Handle(0)
    try:
        if how == "uncertainty":
            h.set_uncertainty(case.P)
        if how == "match_pairs_batch":
            mc, mco = spc.concat(case.mc)
            ms, mso = spc.concat(case.ms)
            c, co, s, so, guesses = _scans(case)
            h.match_pairs_batch(mc, mco, ms, mso, c, co, s, so, guesses)
        else:
            _set_maps(h, case)
        before = _registrations(h, case, how == "uncertainty")
        want = spc.model("five", case)[0]
        for p, c in enumerate(_search(h, case)[0]):
            _same_candidates(c, want[p])
        middle = _registrations(h, case, how == "uncertainty")
        _search(h, case, device=True, want_hits=False)
        after = _registrations(h, case, how == "uncertainty")
        assert before == middle == after
    finally:
        h.close()


def _refused(call):
    from msf_loam_amd import capi
    with pytest.raises(capi.MsflError) as e:
        call()
    return e.value


def test_refusals():
    from msf_loam_amd import capi
    case = spc.CASES["far_and_negative"]()
    want = spc.model("far_and_negative", case)[0]
    cfg = _config(case.cfg)
    c, co, s, so, guesses = _scans(case)
    h = capi.Handle(0)
    try:
        assert _refused(lambda: h.search_pairs(c, co, s, so, guesses, cfg)).status == capi.NO_MAP            # nothing resident
        h.set_map(case.mc[0], case.ms[0])
        assert _refused(lambda: h.search_pairs(c, co, s, so, guesses, cfg)).status == capi.NO_MAP            # a single map is
        single = h.search_poses(case.c[0], case.s[0], case.guess[0], cfg, capacity=case.K)
        _same_candidates(single, want[0])
        _set_maps(h, case)
        before = _registrations(h, case, False)

        def still_fine():
            for p, cand in enumerate(h.search_pairs(c, co, s, so, guesses, cfg, capacity=case.K)):
                _same_candidates(cand, want[p])
            assert _registrations(h, case, False) == before

        still_fine()
        assert _refused(lambda: h.search_poses(case.c[0], case.s[0], case.guess[0], cfg)).status == capi.NO_MAP     # a pair index is resident
        assert _refused(lambda: h.relocalize(case.c[0], case.s[0], case.guess[0], cfg)).status == capi.NO_MAP
        still_fine()
        assert _refused(lambda: h.search_pairs(c, co[:3], s, so[:3], guesses[:2], cfg)).status == capi.BAD_ARG      # 2 pairs, the index holds 3
        still_fine()
        for K in (0, 1025):
            assert _refused(lambda: h.search_pairs(c, co, s, so, guesses, cfg, capacity=K)).status == capi.BAD_ARG, K
        still_fine()
        bad = guesses.copy(); bad[2, 1] = np.nan
        e = _refused(lambda: h.search_pairs(c, co, s, so, bad, cfg))
        assert e.status == capi.BAD_ARG and "pair 2" in str(e) and "pair 2" in h.last_error()
        still_fine()
        assert _refused(lambda: h.search_pairs(c, co, s, so, guesses, _config(case.cfg, max_volume_bytes=64))).status == capi.CAPACITY
        assert _refused(lambda: h.search_pairs(c, co, s, so, guesses, _config(case.cfg, step=0.0))).status == capi.BAD_ARG
        assert _refused(lambda: h.search_pairs(c, co[::-1].copy(), s, so, guesses, cfg)).status == capi.BAD_ARG     # decreasing offsets
        # the geometry rule comes before the pair index: a bad guess with the wrong pair count is the guess's refusal
        e = _refused(lambda: h.search_pairs(c, co[:3], s, so[:3], bad[1:], cfg))
        assert e.status == capi.BAD_ARG and "pair 1" in str(e)
        still_fine()
    finally:
        h.close()


def test_cpp_mirror_searches_pairs_like_ctypes(gpu, tmp_path):
    from msf_loam_amd import capi
    exe = str(tmp_path / "search_pairs_check")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "search_pairs_check.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "msf_loam_amd"), "-lmsfl_hip", "-Wl,-rpath," + os.path.join(ROOT, "msf_loam_amd")])
    case = spc.FIVE()
    K = 8
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.int32(case.P).tobytes())
        for p in range(case.P):
            for cloud in (case.mc[p], case.ms[p], case.c[p], case.s[p]):
                f.write(np.int32(len(cloud)).tobytes()); f.write(np.ascontiguousarray(cloud, np.float32).tobytes())
            f.write(np.asarray(case.guess[p], np.float64).tobytes())
        f.write(bytes(_config(case.cfg)))
        f.write(np.int32(K).tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw = open(tmp_path / "out.bin", "rb").read()
    _set_maps(gpu, case)
    here = _search(gpu, case, want_hits=False, K=K)
    at = 0
    for p in range(case.P):
        n = int(np.frombuffer(raw[at:at + 4], np.int32)[0]); at += 4
        assert n == len(here[p]) > 0 and raw[at:at + 88 * n] == here[p].tobytes(), p
        at += 88 * n
    assert at == len(raw)
    want = spc.model("five", case)[0]
    for p in range(case.P):
        _same_candidates(here[p], want[p][:K])


def test_close_loop_example_searches_every_candidate(tmp_path):
    """examples/close_loop.py --closure-map submap --closure-search is what this test is about: set_pair_maps, search_pairs, one
    score_pairs over all lattice candidates, match_pairs_resident from each pair's best."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "close_loop.py"), "--closure-map", "submap", "--closure-search"], cwd=str(tmp_path),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.splitlines()
    searched = [ln for ln in lines if ": search " in ln]
    verdicts = [ln for ln in lines if "refined fitness" in ln]
    print("\n".join(searched + verdicts + lines[-2:]))
    assert len(verdicts) > 0 and len(searched) == len(verdicts)
    assert [ln.split(":")[0] for ln in searched] == [ln.split(":")[0] for ln in verdicts]
