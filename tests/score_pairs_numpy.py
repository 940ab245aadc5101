"""CPU statement of msfl_score_pairs in numpy: scan p is scored against pair map p only, which is tests/score_numpy.Model of that pair's
two clouds and nothing else.

TEST INFRASTRUCTURE, shared by tests/test_score_pairs_model.py (CPU) and tests/test_gpu_score_pairs.py.  Nothing here touches the GPU.

What the pair form adds to the single form is layout only:
  records   one per hypothesis, pairs in order, a pair's hypotheses in order
  d2 / nn   flat and RAGGED: the row of a hypothesis of pair p holds F(p) = n_corner(p) + n_surf(p) values, corner features first,
            rows in hypothesis order
  nn        the position in pair p's OWN map cloud of the feature's kind.  The device index word of a pair index holds the position
            in the CONCATENATED clouds (own_index undoes that); ties still go to the lowest index, and as the concatenation keeps
            every pair's order that is the lowest own index
"""
import numpy as np

from tests import score_numpy as sn

F = np.float32


def models(maps_c, maps_s, use_tree=True):
    return [sn.Model(mc, ms, use_tree) for mc, ms in zip(maps_c, maps_s)]


def score_pairs(pair_models, corners, surfs, poses, max_dist):
    """Handle.score_pairs(..., want_nn=True): (records (H,), d2 flat f32, nn flat i32); poses[p] is (n_p, 7), possibly empty."""
    recs, d2s, nns = [np.zeros(0, sn.DTYPE)], [np.zeros(0, F)], [np.zeros(0, np.int32)]
    for model, corner, surf, pp in zip(pair_models, corners, surfs, poses):
        pp = np.asarray(pp, np.float64).reshape(-1, 7)
        if len(pp) == 0:
            continue
        rec, d2, nn = model.score(corner, surf, pp, max_dist, want_nn=True)
        recs.append(rec); d2s.append(d2.reshape(-1)); nns.append(nn.reshape(-1))      # (n_p, F(p)) row-major: the pair's rows
    return np.concatenate(recs), np.concatenate(d2s), np.concatenate(nns)


def row_starts(corners, surfs, poses):
    """First d2 / nn element of every hypothesis' row, hypotheses in call order, and the total."""
    starts, at = [], 0
    for corner, surf, pp in zip(corners, surfs, poses):
        nf = len(corner) + len(surf)
        for _ in range(len(np.asarray(pp).reshape(-1, 7))):
            starts.append(at); at += nf
    return np.array(starts, np.int64), at


def own_index(concat_idx, map_off, pair):
    """The index word of a pair index (position in the concatenated clouds, counted from the first used point map_off[0]) as the
    position in pair `pair`'s own cloud; -1 stays -1."""
    concat_idx = np.asarray(concat_idx, np.int64)
    return np.where(concat_idx < 0, -1, concat_idx - (int(map_off[pair]) - int(map_off[0]))).astype(np.int32)
