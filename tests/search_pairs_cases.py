"""The shapes msfl_search_pairs is held to, shared by tests/test_search_pairs_model.py (CPU) and tests/test_gpu_search_pairs.py.
TEST INFRASTRUCTURE; nothing here touches the GPU.

A case is P single-search cases of tests/search_cases.random_case that share ONE config and K: the model of the pairs call is
tests/search_numpy.search applied pair by pair.  The shapes are those at which the single search's mechanisms break (a box of
some twenty voxels a side), plus what batching adds: ragged pairs, empty sides, origins kilometres apart, a launch sized by the
largest pair."""
from types import SimpleNamespace

import numpy as np

from tests import search_cases as sc
from tests import search_numpy as sn


def pairs_case(pairs, K=16, **cfg_kw):
    """pairs: one dict of random_case keywords (seed, n_map, n_feat, guess) per pair; cfg_kw: the shared config."""
    singles = [sc.random_case(kw["seed"], n_map=kw.get("n_map", (150, 400)), n_feat=kw.get("n_feat", (40, 70)), guess=kw.get("guess", sc.GUESS), K=K,
                              **cfg_kw) for kw in pairs]
    cfg = singles[0][5]
    assert all(vars(s[5]) == vars(cfg) for s in singles)
    return SimpleNamespace(mc=[s[0] for s in singles], ms=[s[1] for s in singles], c=[s[2] for s in singles], s=[s[3] for s in singles],
                           guess=np.array([s[4] for s in singles]), cfg=cfg, K=K, P=len(singles))


def _at(xyz):
    return np.concatenate([np.asarray(xyz, np.float64), sc.GUESS[3:]])


def _turned(seed):
    """GUESS's position with another rotation: every pair's yaw lattice is round its own guess."""
    q = np.random.default_rng(seed).normal(size=4)
    return np.concatenate([sc.GUESS[:3], q / np.linalg.norm(q)])


def _ragged3():
    """Pair 0 has an empty corner map, pair 1 no surf features, pair 2 is wholly empty (no map, no features)."""
    case = pairs_case([dict(seed=101, n_map=(0, 300)), dict(seed=102, n_feat=(50, 0), guess=_turned(5)),
                       dict(seed=103, n_map=(0, 0), n_feat=(0, 0), guess=_at([-40.0, 2.0, 0.3]))])
    return case


def _room_first():
    """Pair 0 is the room fixture of tests/search_cases.py (its config is the shared one), pairs 1 and 2 the same scan from guesses
    one cell and one yaw sample away: three full-size searches."""
    f = sc.fixture("room")
    g1, g2 = sc.yawed(f["guess"], 0.1, 0.5, 0.0), sc.yawed(f["guess"], -0.2, -0.25, 0.7)
    return SimpleNamespace(mc=[f["mc"]] * 3, ms=[f["ms"]] * 3, c=[f["corner"]] * 3, s=[f["surf"]] * 3, guess=np.array([f["guess"], g1, g2]),
                           cfg=f["cfg"], K=16, P=3)


_PEAKY = dict(n_map=(3, 4), n_feat=(9, 12))            # few map points, dilated: totals of 0, 1, 2 (search_cases.PEAK_CASES)
_PEAK_CFG = dict(half=(3, 2, 1), n_yaw=6, yaw_step=2 * np.pi / 6, yaw_wraps=1)

CASES = {
    "p1": lambda: pairs_case([dict(seed=1)]),
    "ragged3": _ragged3,
    "far_and_negative": lambda: pairs_case([dict(seed=3, guess=_at([5000.0, -3000.0, 20.0])), dict(seed=4, guess=_at([-12.3, -0.2, -5.1])),
                                            dict(seed=5)]),
    "half_x_64": lambda: pairs_case([dict(seed=40, n_feat=(30, 50)), dict(seed=41, n_feat=(50, 30), guess=_turned(6))], K=64, half=(64, 1, 0), n_yaw=2),
    "no_dilate": lambda: pairs_case([dict(seed=2), dict(seed=6, guess=_turned(7))], dilate=0),
    # 630 hypotheses a pair; windows 0 / 0: every one is a peak (more than K = 1, fewer than K = 1024); windows 1 / 1: a handful
    "peaks_K1": lambda: pairs_case([dict(seed=60, **_PEAKY), dict(seed=61, **_PEAKY)], K=1, nms_cells=0, nms_yaws=0, **_PEAK_CFG),
    "peaks_K1024": lambda: pairs_case([dict(seed=60, **_PEAKY), dict(seed=61, **_PEAKY)], K=1024, nms_cells=0, nms_yaws=0, **_PEAK_CFG),
    "peaks_window_K1024": lambda: pairs_case([dict(seed=60, **_PEAKY), dict(seed=62, n_map=(0, 0), n_feat=(9, 12))], K=1024, nms_cells=1, nms_yaws=1,
                                             **_PEAK_CFG),
    # the correlate kernel's flush inside the feature loop (search_cases: mid-loop at 16 321 features of a kind) in a launch that a
    # pair of 5 + 5 features shares
    "flush_16321": lambda: pairs_case([dict(seed=90, n_map=(3000, 3000), n_feat=(16321, 5)), dict(seed=91, n_map=(3000, 3000), n_feat=(5, 5))],
                                      half=(3, 1, 0), n_yaw=2),
}
FIVE = lambda: pairs_case([dict(seed=110 + p, n_map=(100 + 30 * p, 200), n_feat=(20 + 7 * p, 35), guess=_turned(20 + p)) for p in range(5)])
ROOM = _room_first


def concat(clouds, lead=0):
    """The clouds back to back behind `lead` rows that belong to no pair -> (array, P + 1 offsets)."""
    off = lead + np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int32)
    pad = np.full((lead, 4), 7.5, np.float32)
    return np.ascontiguousarray(np.concatenate([pad] + [np.asarray(c, np.float32).reshape(-1, 4) for c in clouds]), np.float32), off


_models = {}


def model(name, case):
    """tests/search_numpy.search pair by pair -> (list of candidate arrays, hits (P, 2, H)); computed once per process and name."""
    if name not in _models:
        out = [sn.search(case.mc[p], case.ms[p], case.c[p], case.s[p], case.guess[p], case.cfg, case.K) for p in range(case.P)]
        _models[name] = ([o[0] for o in out], np.stack([o[1] for o in out]))
    return _models[name]
