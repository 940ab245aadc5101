"""CPU: the numpy model of msfl_score_poses (tests/score_numpy.py) against a naive double loop, its fixed-point rounding and tie
rule on hand-picked values, and the new declarations of include/msfl_c_api.h as C99."""
import os
import subprocess

import numpy as np

from tests import knn_grid_model as gm
from tests import score_numpy as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _cloud(xyz):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([xyz, np.zeros((len(xyz), 1), F)], 1))


def test_model_equals_a_naive_double_loop():
    rng = np.random.default_rng(7)
    m = _cloud(rng.uniform(-2, 2, (200, 3)))
    feat = _cloud(rng.uniform(-2, 2, (50, 3)))
    q = np.array([0.02, -0.01, 0.03, 1.0]); q /= np.linalg.norm(q)
    pose = np.r_[0.1, -0.2, 0.05, q]
    for max_dist in (1.0, 0.3):
        thr = sn.threshold(max_dist)
        for use_tree in (True, False):
            rec, d2, nn = sn.Model(m[:120], m[120:], use_tree).score(feat[:20], feat[20:], [pose], max_dist, want_nn=True)
            pts = sn.transform_point_f32(pose, feat[:, :3])
            for f in range(50):
                lo, hi = (0, 120) if f < 20 else (120, 200)
                best = min((gm.l2_simple(m[i, :3], pts[f]), i - lo) for i in range(lo, hi))
                assert (d2[0, f], nn[0, f]) == (best if best[0] <= thr else (F(np.inf), -1))
            for kind, sl in enumerate((slice(0, 20), slice(20, 50))):
                hit = nn[0, sl] >= 0
                assert rec["inliers"][0, kind] == hit.sum() and 0 < hit.sum()
                assert int(rec["sum_sq_q32"][0, kind]) == sum(int(np.rint(np.float64(x) * 2.0 ** 32)) for x in d2[0, sl][hit])
            assert rec["status"][0] == 0 and rec["reserved_"][0] == 0


def test_transform_is_the_double_rotation_cast_once():
    rng = np.random.default_rng(8)
    p = rng.uniform(-30, 30, (64, 3)).astype(F)
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    pose = np.r_[rng.uniform(-5, 5, 3), q]
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    want = p.astype(np.float64) @ R.T + pose[:3]
    got = sn.transform_point_f32(pose, p)
    assert got.dtype == F and np.abs(got - want).max() <= 4e-6            # half an ulp of |v| <= 64 is 3.8e-6
    assert np.array_equal(sn.transform_point_f32(np.r_[1.0, 2.0, 3.0, 0, 0, 0, 1.0], p), (p.astype(np.float64) + [1.0, 2.0, 3.0]).astype(F))


def test_fixed_point_rounding_on_hand_picked_values():
    two = lambda e: F(2.0) ** F(e)
    # ties at 2^-33 go to the even integer; values from 2^-9 on (2^23 units) are integers already
    vals = [F(0.0), two(-33), F(3) * two(-33), F(5) * two(-33), two(-32), two(-34), F(1.0), F(0.0025), F(64.0),
            np.nextafter(two(-33), F(1.0)), np.nextafter(two(-33), F(0.0))]
    want = [0, 0, 2, 2, 1, 0, 1 << 32, int(np.float64(F(0.0025)) * 2 ** 32), 1 << 38, 1, 0]
    assert sn.fixed_point(vals) == want
    assert float(F(0.0025)) * 2 ** 32 == int(float(F(0.0025)) * 2 ** 32)          # (an integer: the scaling is exact)
    # exactly thr is an inlier, one step above is not
    thr = sn.threshold(0.5)
    assert thr == F(0.25)
    m = _cloud([[0.5, 0, 0], [np.nextafter(F(0.5), F(1)), 0, 0]])
    ident = np.r_[0.0, 0, 0, 0, 0, 0, 1]
    empty = np.zeros((0, 4), F)
    rec, d2, nn = sn.Model(m[:1], empty).score(_cloud([[0, 0, 0]]), empty, [ident], 0.5, want_nn=True)
    assert rec["inliers"][0, 0] == 1 and int(rec["sum_sq_q32"][0, 0]) == 1 << 30 and nn[0, 0] == 0 and d2[0, 0] == F(0.25)
    rec, d2, nn = sn.Model(m[1:], empty).score(_cloud([[0, 0, 0]]), empty, [ident], 0.5, want_nn=True)
    assert rec["inliers"][0, 0] == 0 and rec["sum_sq_q32"][0, 0] == 0 and nn[0, 0] == -1 and np.isposinf(d2[0, 0])
    # thr is the DOUBLE product cast once: 0.1 * 0.1 in f32 arithmetic would differ
    assert sn.threshold(0.1) == F(np.float64(0.1) * np.float64(0.1)) and sn.threshold(0.1) != F(0.1) * F(0.1)


def test_ties_go_to_the_lowest_original_index_and_bad_inputs_score_nothing():
    pts = [[1, 0, 0], [0, 1, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0]]
    m = _cloud(pts)
    ident = np.r_[0.0, 0, 0, 0, 0, 0, 1]
    feat = _cloud([[0, 0, 0], [0.9, 0, 0], [0, 0.9, 0], [np.nan, 0, 0], [0, np.inf, 0]])
    for use_tree in (True, False):
        rec, d2, nn = sn.Model(m, m[::-1]).score(feat, feat, [ident, np.r_[np.nan, 0, 0, 0, 0, 0, 1], ident], 1.0, want_nn=True)
        assert nn[0, :5].tolist() == [0, 0, 1, -1, -1]            # four points at d2 = 1 from the origin: index 0; duplicates: the first
        assert nn[0, 5:].tolist() == [0, 2, 0, -1, -1]            # the reversed map: its own indices
        assert rec["inliers"].tolist() == [[3, 3], [0, 0], [3, 3]] and rec["status"].tolist() == [0, sn.BAD_ARG, 0]
        assert (nn[1] == -1).all() and np.isposinf(d2[1]).all() and rec["sum_sq_q32"][1].tolist() == [0, 0]
        assert np.array_equal(rec[0], rec[2])


def test_the_header_compiles_as_c99_with_the_score_declarations(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "score_check_c.c"), "-o", str(tmp_path / "score_check_c.o")])


def test_the_cpp_mirror_compiles_with_score_poses(tmp_path):
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "score_check.cpp"), "-o", str(tmp_path / "score_check.o")])


def test_the_walk_skips_nothing_it_needs():
    """nn1_grid's pruning (a row or end cell is skipped when its lower bound exceeds the current best distance), restated in numpy,
    against brute force: the lattice map (ties, duplicates, the gate), the generic map and the map with points on the faces of
    its box, at the default cell edge and at grown cells, thresholds at and below the index radius."""
    from tests import knn_grid_cases as kc
    rng = np.random.default_rng(3)
    n_hit, steps = 0, []
    for name in ("lattice", "generic", "faces"):
        c = kc.case(name)
        for cap in (gm.DEFAULT_CAP, 8):
            for kind, (m, feat) in enumerate(((c.mc, c.corner), (c.ms, c.surf))):
                ix = sn.WalkIndex(m, cap)
                steps.append(ix.g.steps)
                sel = rng.permutation(len(feat))[:40]
                for pose in c.poses:
                    q = sn.transform_point_f32(pose, feat[sel, :3])
                    for max_dist in (1.0, 0.5, 0.05):
                        thr = sn.threshold(max_dist)
                        d2_b, nn_b = sn.nearest(m, q, thr)
                        got = [sn.walk_nearest(ix, qq, thr) for qq in q]
                        assert [g[1] for g in got] == nn_b.tolist(), (name, cap, kind, max_dist)
                        assert np.array_equal(np.array([g[0] for g in got], F), d2_b)
                        n_hit += int((nn_b >= 0).sum())
    assert n_hit > 1000 and min(steps) == 0 and sorted(steps)[-6] >= 2, (n_hit, steps)
