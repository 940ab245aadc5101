"""CPU: the pose search's model (tests/search_numpy.py) is checked against more than itself, and the library's host-only geometry
rule and refusals are checked against the model.  No GPU: msfl_search_geometry takes no handle.

  - the two statements of the count (dense volume looked up at v + k; sorted voxel keys, no volume) agree on every shape of
    tests/search_cases.py;
  - the peak rule by shifted arrays equals the pair-by-pair rule, with ties, windows 0 / 1 / 2 and yaw_wraps 0 / 1;
  - msfl_search_geometry equals the model's geometry, far from the origin and at negative coordinates too;
  - the fixture condition: on the room and the outdoor world the model's first candidate is the yaw sample nearest the truth and
    lies within 2 cells of the lattice node nearest the truth;
  - the refusals of the config."""
import os
import subprocess

import numpy as np
import pytest

from tests import search_cases as sc
from tests import search_numpy as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _capi():
    from msf_loam_amd import capi
    import os
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi


def _capi_config(capi, cfg):
    return capi.SearchConfig(step=cfg.step, half=cfg.half, n_yaw=cfg.n_yaw, yaw_min=cfg.yaw_min, yaw_step=cfg.yaw_step, yaw_wraps=cfg.yaw_wraps,
                             dilate=cfg.dilate, range=cfg.range, nms_cells=cfg.nms_cells, nms_yaws=cfg.nms_yaws,
                             max_volume_bytes=cfg.max_volume_bytes)


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_the_two_statements_of_the_count_agree(name):
    mc, ms, c, s, guess, cfg, K = sc.CASES[name]()
    dense = sn.hits_dense(mc, ms, c, s, guess, cfg)
    sparse = sn.hits_sparse(mc, ms, c, s, guess, cfg)
    assert dense.shape == (2, sn.geometry(guess, cfg).H) and dense.dtype == np.int32
    assert np.array_equal(dense, sparse)
    if name.startswith(("random", "half_x", "handmade", "far", "negative", "flush")):
        assert dense.sum() > 0                                                         # the shape exercises hits ...
        assert (dense.sum(0) < len(c) + len(s)).any()                                  # ... and misses
    if name.startswith("flush"):
        assert (dense.max(0) > 255).mean() > 0.5                                       # most counts are beyond what 8 planes hold


def test_the_shift_is_not_the_voxel_of_the_shifted_pose():
    """What the definition says it is not: counting the voxel of the point transformed by pose(a, k) gives other numbers on a
    guess off the voxel grid (f32 rounding at voxel faces), so the doc's sentence is about something real."""
    mc, ms, c, s, guess, cfg, K = sc.random_case(1, guess=np.concatenate([[5000.123, -3000.456, 20.789], sc.GUESS[3:]]), n_feat=(300, 400), step=0.3)
    g = sn.geometry(guess, cfg)
    hits = sn.hits_dense(mc, ms, c, s, guess, cfg)
    vol = [sn.dense_volume(m, g, cfg.dilate) for m in (mc, ms)]
    other = np.zeros_like(hits)
    a_, kx, ky, kz = sn.lattice_coords(cfg)
    for h in range(g.H):
        k = (kx[h] - cfg.half[0], ky[h] - cfg.half[1], kz[h] - cfg.half[2])
        for kind, feat in enumerate((c, s)):
            f = sn.voxel_f(sn.transform_point_f32(sn.pose(guess, cfg, a_[h], k), feat[:, :3]), g)
            ok = (f >= 0).all(1) & (f[:, 0] < g.dims[0]) & (f[:, 1] < g.dims[1]) & (f[:, 2] < g.dims[2])
            v = f[ok].astype(np.int64)
            other[kind, h] = vol[kind][v[:, 2], v[:, 1], v[:, 0]].sum()
    assert np.abs(other.astype(np.int64) - hits).max() <= 8 and not np.array_equal(other, hits)


@pytest.mark.parametrize("name", sorted(sc.PEAK_CASES))
def test_peak_rule_against_brute_force(name):
    mc, ms, c, s, guess, cfg, K = sc.PEAK_CASES[name]()
    hits = sn.hits_sparse(mc, ms, c, s, guess, cfg)
    brute = sn.peaks_brute(hits, cfg)
    assert np.array_equal(sn.peaks_window(hits, cfg), brute)
    total = hits.sum(0)
    assert len(np.unique(total)) < len(total)                                          # ties are in play
    if cfg.nms_cells == 0 and cfg.nms_yaws == 0:
        assert brute.all()
    assert brute[np.lexsort((np.arange(len(total)), -total))[0]]                       # the first in the order is always a peak
    cand = sn.candidates(hits, guess, cfg, K, brute)
    assert len(cand) == min(K, int(brute.sum()))
    tot = cand["hits"].sum(1)
    assert all((tot[i] > tot[i + 1]) or (tot[i] == tot[i + 1] and cand["h"][i] < cand["h"][i + 1]) for i in range(len(cand) - 1))


def test_peak_rule_on_handmade_ties():
    cfg = sn.config(half=(2, 0, 0), n_yaw=4, yaw_wraps=1, nms_cells=1, nms_yaws=1)
    hits = np.zeros((2, 20), np.int32)
    hits[0, [0, 1, 8, 19]] = 5                                                          # h = a * 5 + kx': 0 and 1 are neighbours with equal totals
    hits[1, 11] = 5
    for wraps in (0, 1):
        cfg.yaw_wraps = wraps
        pk = sn.peaks_brute(hits, cfg)
        assert np.array_equal(pk, sn.peaks_window(hits, cfg))
        assert pk[0] and not pk[1] and pk[8] and pk[11] and pk[19]                      # the tie goes to the lower index
    cfg.yaw_wraps = 1
    hits[0, 4] = 5                                                                      # (a 0, kx' 4): now 19 = (a 3, kx' 4) has an earlier equal neighbour across the wrap
    assert not sn.peaks_brute(hits, cfg)[19] and sn.peaks_brute(hits, cfg)[4]
    cfg.yaw_wraps = 0
    assert sn.peaks_brute(hits, cfg)[19]


GEOMETRY_CASES = [
    (sc.GUESS, dict()),
    (sc.GUESS, dict(range=3.0, half=(64, 1, 2), dilate=0)),
    (np.concatenate([[5000.0, -3000.0, 20.0], sc.GUESS[3:]]), dict(range=40.0, half=(4, 4, 0))),
    (np.concatenate([[-12.3, -0.2, -5.1], sc.GUESS[3:]]), dict(range=3.0, step=0.3)),
    (np.concatenate([[-0.5, 0.0, 0.5], sc.GUESS[3:]]), dict(range=7.7, step=0.7, half=(0, 0, 0), n_yaw=1)),
]


@pytest.mark.parametrize("i", range(len(GEOMETRY_CASES)))
def test_geometry_rule_equals_the_model(i):
    capi = _capi()
    guess, kw = GEOMETRY_CASES[i]
    cfg = sn.config(**kw)
    s, g = capi.search_geometry(guess, _capi_config(capi, cfg), 161, 5285)
    m = sn.geometry(guess, cfg, 161, 5285)
    assert s == capi.OK
    assert np.array(g.origin[:], np.float32).tobytes() == m.origin.tobytes() and np.float32(g.inv_step) == m.inv
    assert list(g.dims) == m.dims and g.words_per_row == m.W and list(g.n) == m.n and g.n_yaw == m.n_yaw
    assert (g.n_hypotheses, g.volume_bytes, g.scratch_bytes) == (m.H, m.volume_bytes, m.scratch_bytes)
    # the box holds every feature within `range` of any lattice node, dilated, with a cell to spare
    lo = m.origin.astype(np.float64)
    hi = lo + cfg.step * np.array(m.dims)
    reach = cfg.range + cfg.step * (np.array(cfg.half) + cfg.dilate)
    assert (lo <= guess[:3] - reach).all() and (hi >= guess[:3] + reach).all()


def test_default_config():
    capi = _capi()
    c, m = capi.SearchConfig(), sn.config()
    assert (c.step, tuple(c.half), c.n_yaw, c.yaw_min, c.yaw_step, c.yaw_wraps, c.dilate, c.range, c.nms_cells, c.nms_yaws, c.max_volume_bytes) == \
           (m.step, m.half, m.n_yaw, m.yaw_min, m.yaw_step, m.yaw_wraps, m.dilate, m.range, m.nms_cells, m.nms_yaws, m.max_volume_bytes)
    assert c.yaw_step == 2.0 * np.pi / 24.0


def test_config_refusals():
    capi = _capi()
    ok = dict(range=3.0)
    assert capi.search_geometry(sc.GUESS, capi.SearchConfig(**ok))[0] == capi.OK
    for bad in (dict(step=0.0), dict(step=-0.5), dict(step=np.nan), dict(step=np.inf), dict(range=0.0), dict(range=np.nan), dict(half=(1, -1, 0)),
                dict(n_yaw=0), dict(yaw_min=np.nan), dict(yaw_step=np.inf), dict(yaw_wraps=2), dict(dilate=2), dict(dilate=-1), dict(nms_cells=-1),
                dict(nms_yaws=-1), dict(max_volume_bytes=0)):
        s, _ = capi.search_geometry(sc.GUESS, capi.SearchConfig(**dict(ok, **bad)), allow=(capi.BAD_ARG,))
        assert s == capi.BAD_ARG, bad
    for k in range(7):
        for v in (np.nan, np.inf):
            g = sc.GUESS.copy(); g[k] = v
            assert capi.search_geometry(g, capi.SearchConfig(**ok), allow=(capi.BAD_ARG,))[0] == capi.BAD_ARG
    assert capi.search_geometry(sc.GUESS, capi.SearchConfig(**ok), -1, 0, allow=(capi.BAD_ARG,))[0] == capi.BAD_ARG
    with pytest.raises(capi.MsflError):
        capi.search_geometry(sc.GUESS, capi.SearchConfig(step=0.0))
    # capacity: the volume cap, 2^24 hypotheses, the dimension cap, the table cap
    for big in (dict(max_volume_bytes=1000), dict(half=(200, 200, 0), n_yaw=200), dict(range=1e6), dict(range=3.0, half=(1 << 21, 0, 0))):
        s, _ = capi.search_geometry(sc.GUESS, capi.SearchConfig(**dict(ok, **big)), allow=(capi.CAPACITY,))
        assert s == capi.CAPACITY, big
    assert capi.search_geometry(sc.GUESS, capi.SearchConfig(n_yaw=4096, **ok), 1 << 14, 1, allow=(capi.CAPACITY,))[0] == capi.CAPACITY
    assert capi.search_geometry(sc.GUESS, capi.SearchConfig(**ok), 1 << 24, 0, allow=(capi.CAPACITY,))[0] == capi.CAPACITY
    s, g = capi.search_geometry(sc.GUESS, capi.SearchConfig(max_volume_bytes=1000, **ok), allow=(capi.CAPACITY,))
    assert g.volume_bytes == sn.geometry(sc.GUESS, sn.config(**ok)).volume_bytes > 1000     # the refusal still says how much it wanted


def test_the_header_compiles_as_c99_with_the_search_declarations(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "search_check_c.c"), "-o", str(tmp_path / "search_check_c.o")])


def test_the_cpp_mirror_compiles_with_the_search(tmp_path):
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "search_check.cpp"), "-o", str(tmp_path / "search_check.o")])


@pytest.mark.parametrize("kind", ["room", "outdoor"])
def test_fixture_condition(kind):
    """The coarse score selects the basin: first candidate = the yaw sample nearest the truth, within 2 cells (Chebyshev) of the
    lattice node nearest the truth."""
    f = sc.fixture(kind)
    cfg, guess, truth = f["cfg"], f["guess"], f["truth"]
    hits = sn.hits_sparse(f["mc"], f["ms"], f["corner"], f["surf"], guess, cfg)
    best = sn.candidates(hits, guess, cfg, 5)[0]
    node = np.round((truth[:3] - guess[:3]) / cfg.step).astype(int)
    # the truth is the guess turned by +34 degrees: the nearest of the samples 0, 15, 30, ... is a = 2
    a_true = int(np.round((np.deg2rad(34.0) - cfg.yaw_min) / cfg.yaw_step)) % cfg.n_yaw
    print(kind, "first candidate a %d k (%d, %d, %d) hits %s; nearest node %s, yaw sample %d; best / median total %d / %d"
          % (best["a"], best["kx"], best["ky"], best["kz"], best["hits"], node, a_true, hits.sum(0).max(), np.median(hits.sum(0))))
    assert a_true == 2 and best["a"] == a_true
    assert max(abs(best["kx"] - node[0]), abs(best["ky"] - node[1]), abs(best["kz"] - node[2])) <= 2
