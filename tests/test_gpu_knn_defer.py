"""The deferred 5-NN walk of the whole-batch kernel (knn5_scan2map_split_kernel<true>: capped row visits, the rest of a long range
walked after the ninth row) against the plain walk (MSFL_KNN_DEFER=0) and the brute-force oracle.

Every case is a batch of at least 65 536 records (16 scans of ~4 100 surf queries and a few corner queries, or as many copies of a
smaller cloud as that takes): the smallest shape that reaches the whole-batch kernel.

  same result     poses, statuses, accepted counts, iteration counts and final costs of the batch are equal bit for bit between a
                  handle created with MSFL_KNN_DEFER=0 and one with MSFL_KNN_DEFER=1.
  oracle          the records of the first scan at its first pose, through the counting 5-NN instantiation (which takes the handle's
                  walk), equal the plain walk's and match the brute-force oracle's accept set and records.
  it ran          the deferred walk evaluates at least the plain walk's candidates on every case and more on the dense block, where the
                  CPU model (tests/knn_defer_model.py) says that ranges are deferred and that the stack fills.

Cases: a thinned room map; a dense block (sheets in a 3 m cube, queries on the sheets and in a 0.75 m void in its middle, where all nine
rows exceed their caps); the lattice (exact ties and duplicates: the ambiguous-lane search after a deferred walk); a sparse map (fewer than five points
inside the gate: features refused); the grid-face case of tests/knn_grid_cases.py; one cell row of 10 000 points; clusters of exactly
2c - 1, 2c, 2c + 1 and 2c + 2 points for the centre cap c.
"""
import functools

import numpy as np
import pytest

from tests import knn_defer_model as dm
from tests import knn_grid_cases as gc
from tests import knn_grid_model as gm
from tests.test_gpu_knn_grid import _assert_same, _check_against_oracle

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ("room", "dense", "lattice", "sparse", "faces", "long_row", "cap_edges")
MIN_RECORDS = 65536
CENTRE_CAP = dm.SHIPPED_CAPS[0]


def _small_poses(n, seed):
    """n poses within 5 cm and 0.3 degrees of the identity (the first one is the identity)."""
    rng = np.random.default_rng(seed)
    out = [gc.IDENTITY]
    for _ in range(n - 1):
        v = rng.normal(0, 0.002, 3)
        q = np.r_[v, 1.0]; q /= np.linalg.norm(q)
        out.append(np.r_[rng.uniform(-0.05, 0.05, 3), q])
    return tuple(out)


def _line_corner(rng, a, b):
    """A corner map of 60 points on the segment a-b and eight queries next to it."""
    t = np.linspace(0, 1, 60)[:, None]
    line = np.asarray(a) + t * (np.asarray(b) - np.asarray(a))
    return gc.pts4(line), gc.pts4(line[rng.integers(0, 60, 8)] + rng.normal(0, 0.03, (8, 3)))


def _sheets(rng, lo, size, n, per_axis=(3, 3, 4), jitter=0.003):
    """n points on axis-aligned sheets inside the box lo + [0, size]^3."""
    total = sum(per_axis)
    out = []
    for axis, count in enumerate(per_axis):
        for k in range(count):
            m = n // total
            p = rng.uniform(0, size, (m, 3))
            p[:, axis] = size * (k + 0.5) / count + rng.normal(0, jitter, m)
            out.append(lo + p)
    return np.concatenate(out)


def _room(rng):
    from msf_loam_amd import synth
    mc, ms = synth.make_map(synth.World(ground_half=synth.ground_half_for_target(30000)))
    pick = rng.permutation(len(ms))
    keep, rest = pick[:20000], pick[20000:]
    surf = ms[rest[:4100], :3] + rng.normal(0, 0.02, (4100, 3))
    corner = mc[rng.integers(0, len(mc), 12), :3] + rng.normal(0, 0.02, (12, 3))
    return gc.Case("room", gc.pts4(mc[:, :3]), gc.pts4(ms[keep, :3]), gc.pts4(corner), gc.pts4(surf), _small_poses(16, 1))


def _dense(rng):
    lo = np.array([4.0, -2.0, 1.0])
    ms = _sheets(rng, lo, 3.0, 24000)
    # a void of 0.75 m radius round the middle of the block, which is the middle of a cell of the map's grid: for a query in it every row
    # of the neighbourhood is within the 5th distance and holds far more than its cap
    void = lo + 1.5
    ms = ms[np.linalg.norm(ms - void, axis=1) > 0.75]
    inside = ms[rng.integers(0, len(ms), 3600)] + rng.normal(0, 0.01, (3600, 3))
    hollow = void + rng.uniform(-0.1, 0.1, (500, 3))
    mc, corner = _line_corner(rng, lo + 0.2, lo + 2.8)
    return gc.Case("dense", mc, gc.pts4(ms), corner, gc.pts4(np.concatenate([inside, hollow])), _small_poses(16, 2))


def _sparse(rng):
    lo, ext = np.array([-30.0, 10.0, -5.0]), np.array([60.0, 60.0, 20.0])
    ms = lo + rng.uniform(0, 1, (3000, 3)) * ext
    surf = np.concatenate([lo + rng.uniform(0, 1, (3900, 3)) * ext, ms[rng.integers(0, 3000, 200)] + rng.normal(0, 0.1, (200, 3))])
    mc, corner = _line_corner(rng, lo + 1.0, lo + 9.0)
    return gc.Case("sparse", mc, gc.pts4(ms), corner, gc.pts4(surf), _small_poses(16, 3))


def _long_row(rng):
    ms = np.stack([rng.uniform(0, 30.0, 10000), rng.uniform(0, 0.5, 10000), 2.0 + rng.normal(0, 0.003, 10000)], 1)
    surf = ms[rng.integers(0, 10000, 4100)] + rng.normal(0, 0.02, (4100, 3))
    surf[:200, 0] += rng.choice([-0.9, 0.9], 200)                 # some whose neighbours start at the end cells of the reach
    mc, corner = _line_corner(rng, [0.5, 0.1, 2.2], [29.5, 0.4, 2.2])
    return gc.Case("long_row", mc, gc.pts4(ms), corner, gc.pts4(surf), _small_poses(16, 4))


def _cap_edges(rng):
    """1 024 clusters 3 m apart on a plane, of 2c - 1, 2c, 2c + 1 and 2c + 2 points in turn, each within 8 cm of its centre: a query at
    the centre has the whole cluster, and nothing else, in its centre row unless a cell boundary cuts the cluster."""
    c = CENTRE_CAP
    ms, surf = [], []
    for j in range(1024):
        centre = np.array([3.0 * (j % 32) + 1.37, 3.0 * (j // 32) + 0.61, 1.0])
        n = 2 * c - 1 + j % 4
        p = centre + np.c_[rng.uniform(-0.08, 0.08, (n, 2)), rng.normal(0, 0.002, n)]
        ms.append(p)
        surf.append(centre + np.c_[rng.uniform(-0.03, 0.03, (4, 2)), rng.normal(0, 0.01, 4)])
    mc, corner = _line_corner(rng, [1.0, 1.0, 1.5], [9.0, 1.2, 1.5])
    return gc.Case("cap_edges", mc, gc.pts4(np.concatenate(ms)), corner, gc.pts4(np.concatenate(surf)), _small_poses(16, 5))


@functools.lru_cache(maxsize=None)
def _case(name):
    rng = np.random.default_rng(7001 + NAMES.index(name))
    if name in ("lattice", "faces"):
        return gc.case(name)
    return {"room": _room, "dense": _dense, "sparse": _sparse, "long_row": _long_row, "cap_edges": _cap_edges}[name](rng)


def _handle(defer):
    from msf_loam_amd import capi
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MSFL_KNN_DEFER", str(defer))
        return capi.Handle(0)


@pytest.fixture(scope="module")
def handles(gpu):
    hs = {0: _handle(0), 1: _handle(1)}
    yield hs
    for h in hs.values():
        h.close()


@functools.lru_cache(maxsize=None)
def _oracle_corr(name):
    from oracle import oracle as orc
    orc.build()
    c = _case(name)
    return orc.associate_scan2map(c.mc, c.ms, c.corner, c.surf, c.poses[0], use_kdtree=False)


def _counted(h, c):
    h.set_timing(3)
    try:
        h.get_timing(reset=True)
        rec = h.associate_scan2map(c.corner, c.surf, c.poses[0])
        return rec, h.get_timing(reset=True).knn_candidates
    finally:
        h.set_timing(0)


@functools.lru_cache(maxsize=None)
def _model(name, n_queries=400):
    """The CPU model on the first surf queries of the case at its first pose (the identity): candidates of the plain and the deferred
    walk, ranges deferred, ranges walked in place on a full stack, and the lengths of the centre-row ranges."""
    c = _case(name)
    ix = dm.Index(c.ms, gm.desc_of(c.ms))
    q = c.surf[:, :3]
    pick = np.r_[0:min(n_queries // 2, len(q)), max(len(q) - n_queries // 2, 0):len(q)]
    su = dm.setup(ix, q[pick])
    out = {"plain": 0, "defer": 0, "deferred": 0, "in_place": 0}
    for i in range(len(pick)):
        d2 = gm.l2_simple(ix.pts, q[pick[i]])
        out["plain"] += dm.walk(ix, su, i, d2)[1]["cand"]
        st = dm.walk(ix, su, i, d2, caps=dm.SHIPPED_CAPS, depth=dm.SHIPPED_DEPTH)[1]
        out["defer"] += st["cand"]; out["deferred"] += st["deferred"]; out["in_place"] += st["in_place"]
    return out


@pytest.mark.parametrize("name", NAMES)
def test_the_deferred_walk_gives_the_plain_walks_batch(handles, oracle, name):
    c = _case(name)
    n_feat = len(c.corner) + len(c.surf)
    B = max(16, -(-MIN_RECORDS // n_feat))
    assert B * n_feat >= MIN_RECORDS
    co, so = np.arange(B + 1, dtype=np.int32) * len(c.corner), np.arange(B + 1, dtype=np.int32) * len(c.surf)
    guesses = np.array([c.poses[i % len(c.poses)] for i in range(B)])
    corner, surf = np.tile(c.corner, (B, 1)), np.tile(c.surf, (B, 1))
    out = {}
    for d, h in handles.items():
        h.set_map(c.mc, c.ms)
        out[d] = h.match_scan2map_batch(corner, co, surf, so, guesses, want_info=True)
    (p0, s0, i0), (p1, s1, i1) = out[0], out[1]
    assert np.array_equal(s0, s1), "case %s: statuses differ, first at scan %d" % (name, int(np.flatnonzero(s0 != s1)[0]))
    assert np.array_equal(p0.view(np.uint64), p1.view(np.uint64)), "case %s: poses differ, first at scan %d" % (
        name, int(np.flatnonzero((p0.view(np.uint64) != p1.view(np.uint64)).any(1))[0]))
    for j in range(B):
        for f in ("n_edge", "n_plane", "lm_iterations", "final_cost"):
            a, b = np.array(getattr(i0[j], f)), np.array(getattr(i1[j], f))
            assert a.tobytes() == b.tobytes(), "case %s scan %d: %s %s vs %s" % (name, j, f, a, b)
    n_plane = int(sum(i0[j].n_plane[0] for j in range(B)))
    print("%-10s B %d, %d records, statuses ok %d / %d, planes accepted in the first pass %d" % (name, B, B * n_feat, int((s0 == 0).sum()), B, n_plane))
    if name == "sparse":
        assert n_plane < B * len(c.surf) // 10                  # features are refused
    else:
        assert n_plane > B * len(c.surf) // 8, (name, n_plane)   # not equally empty


@pytest.mark.parametrize("name", NAMES)
def test_records_and_candidates_of_the_deferred_walk(handles, oracle, name):
    c = _case(name)
    recs, counts = {}, {}
    for d, h in handles.items():
        h.set_map(c.mc, c.ms)
        recs[d], counts[d] = _counted(h, c)
    _assert_same(recs[1], recs[0], "case %s: records of the deferred against the plain walk" % name)
    n_e, n_p, err = _check_against_oracle(recs[1], _oracle_corr(name), len(c.corner), "case %s, deferred walk" % name)
    m = _model(name)
    print("%-10s edges %d planes %d accepted, largest record error %.3e; candidates plain %d deferred %d (x %.4f); model on %s: x %.4f"
          % (name, n_e, n_p, err, counts[0], counts[1], counts[1] / max(counts[0], 1), m, m["defer"] / max(m["plain"], 1)))
    assert counts[1] >= counts[0] > 0, (name, counts)
    if name == "dense":
        assert m["deferred"] > 0 and m["in_place"] > 0, m         # more long ranges than the stack holds: the in-place path runs
        assert counts[1] > counts[0], counts
    if name == "sparse":
        assert m["deferred"] == 0, m
    if name == "cap_edges":
        # the centre-row ranges really have the four lengths around twice the centre cap
        ix = dm.Index(c.ms, gm.desc_of(c.ms))
        su = dm.setup(ix, c.surf[:, :3])
        lens = set()
        for i in range(len(c.surf)):
            if su["valid"][0][i]:
                lens.add(ix.start[su["base"][0][i] + su["xe"][i] + 1] - ix.start[su["base"][0][i] + su["xs"][i]])
        assert {2 * CENTRE_CAP - 1, 2 * CENTRE_CAP, 2 * CENTRE_CAP + 1, 2 * CENTRE_CAP + 2} <= lens, sorted(lens)
