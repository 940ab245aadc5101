"""CPU: the numpy statement of msfl_score_pairs (tests/score_pairs_numpy.py) on the lattice map and its reverse, so that ties and
duplicates resolve per pair, its ragged d2 / nn layout and own-cloud indices; and the declarations of the resident pair maps in
include/msfl_c_api.h as C99 and in the C++ mirror as C++14."""
import os
import subprocess

import numpy as np

from tests import knn_grid_cases as kc
from tests import knn_grid_model as gm
from tests import score_numpy as sn
from tests import score_pairs_numpy as spn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_the_header_compiles_as_c99_with_the_pair_map_declarations(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "score_pairs_check_c.c"), "-o", str(tmp_path / "score_pairs_check_c.o")])


def test_the_cpp_mirror_compiles_with_the_pair_map_methods(tmp_path):
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "score_pairs_check.cpp"), "-o", str(tmp_path / "score_pairs_check.o")])


def lattice_pairs():
    """Two pairs over the same points: the lattice map (equal f32 distances, duplicated points) and the same clouds reversed.  The scans
    differ in length, the hypotheses per pair too."""
    c = kc.case("lattice")
    maps_c, maps_s = [c.mc, np.ascontiguousarray(c.mc[::-1])], [c.ms, np.ascontiguousarray(c.ms[::-1])]
    corners, surfs = [c.corner, c.corner[:-3]], [c.surf, c.surf[5:]]
    poses = [np.array(c.poses), np.array(list(c.poses) + [kc.IDENTITY])]
    return maps_c, maps_s, corners, surfs, poses


def test_pairs_resolve_ties_and_duplicates_in_their_own_clouds():
    maps_c, maps_s, corners, surfs, poses = lattice_pairs()
    rec, d2, nn = spn.score_pairs(spn.models(maps_c, maps_s), corners, surfs, poses, 1.0)
    rec_b, d2_b, nn_b = spn.score_pairs(spn.models(maps_c, maps_s, use_tree=False), corners, surfs, poses, 1.0)
    assert rec.tobytes() == rec_b.tobytes() and np.array_equal(d2, d2_b) and np.array_equal(nn, nn_b)
    starts, total = spn.row_starts(corners, surfs, poses)
    assert len(rec) == 5 and len(starts) == 5 and len(d2) == len(nn) == total
    n0, n1 = len(corners[0]) + len(surfs[0]), len(corners[1]) + len(surfs[1])
    assert starts.tolist() == [0, n0, 2 * n0, 2 * n0 + n1, 2 * n0 + 2 * n1] and total == 2 * n0 + 3 * n1 and n0 != n1
    # the first two hypotheses are the same two poses in both pairs, and pair 1's scan is a part of pair 0's
    thr = sn.threshold(1.0)
    reordered = 0
    for hyp in range(2):
        a0, a1 = starts[hyp], starts[2 + hyp]
        for kind, (lo0, lo1, skip, n) in enumerate(((0, 0, 0, len(corners[1])), (len(corners[0]), len(corners[1]), 5, len(surfs[1])))):
            m_fwd, m_rev = (maps_c, maps_s)[kind]
            q = sn.transform_point_f32(poses[0][hyp], (corners, surfs)[kind][1][:, :3])
            d_fwd, i_fwd = d2[a0 + lo0 + skip:a0 + lo0 + skip + n], nn[a0 + lo0 + skip:a0 + lo0 + skip + n]
            d_rev, i_rev = d2[a1 + lo1:a1 + lo1 + n], nn[a1 + lo1:a1 + lo1 + n]
            assert np.array_equal(d_fwd, d_rev) and np.array_equal(i_fwd >= 0, i_rev >= 0) and (i_fwd >= 0).sum() > 10      # (the lattice scan has 17 corner features)
            for f in np.flatnonzero(i_fwd >= 0):
                # in each pair: the LOWEST own index among the points at the winning f32 distance
                for m, i in ((m_fwd, i_fwd[f]), (m_rev, i_rev[f])):
                    d = gm.l2_simple(m[:, :3], q[f])
                    assert d[i] == d_fwd[f] <= thr and d.min() == d[i] and int(np.flatnonzero(d == d[i])[0]) == i
                reordered += int(i_rev[f] != len(m_fwd) - 1 - i_fwd[f])
    assert reordered > 10                  # ties and duplicates: the reversed pair does not simply return the mirrored index


def test_the_index_word_counts_in_the_concatenated_clouds():
    maps_c, maps_s, corners, surfs, poses = lattice_pairs()
    lead = 7                                                  # unused leading points: the offsets need not start at zero
    cat = np.concatenate([np.zeros((lead, 4), F)] + maps_s)
    off = np.cumsum([lead] + [len(m) for m in maps_s])
    _, d2, nn = spn.score_pairs(spn.models(maps_c, maps_s), corners, surfs, poses, 1.0)
    starts, _ = spn.row_starts(corners, surfs, poses)
    thr = sn.threshold(1.0)
    for pair, hyp in ((0, 1), (1, 4)):
        q = sn.transform_point_f32(poses[pair][hyp - (0 if pair == 0 else 2)], surfs[pair][:, :3])
        at = starts[hyp] + len(corners[pair])
        for f in range(0, len(q), 9):
            # what the device keeps: the position among the points the index was built over, pair p owning [off[p], off[p + 1])
            d = gm.l2_simple(cat[off[pair]:off[pair + 1], :3], q[f])
            k = int(np.argmin(d)) + int(off[pair] - off[0]) if d.min() <= thr else -1
            assert spn.own_index([k], off, pair)[0] == nn[at + f]
    assert spn.own_index([-1, 12], off, 1).tolist() == [-1, 12 - len(maps_s[0])]
