"""CPU: the geometry of the scan-to-map 5-NN index, pinned by the model of tests/knn_grid_model.py on the cases of
tests/knn_grid_cases.py.  The GPU counterpart is tests/test_gpu_knn_grid.py.

What is asserted (conditions, not tolerances):

  no miss         for every case, pose and table cap in {8, 64, 4 096, 65 536, 1 M, 64 M}: every one of the brute-force top five
                  (oracle.knn_brute, FLANN L2_Simple order) of every query whose 5th distance is inside the gate lies in a cell
                  that the walk can reach and may not skip, whatever its visit order
  adversarial     at each rod's extent, 1e6 trials with the map point on a computed cell boundary and the 5th distance equal to
                  the point's own: zero misses with the descriptor the code builds -- and thousands without the kGridMaxDim
                  limit at x 6 km (trimmed end cells) and y 12 km (skipped rows), which is why the limit exists
  same descriptor a box of at most kGridMaxDim cells per axis gets the descriptor it had before the limit, bit for bit
  not vacuous     every rod has in-gate queries whose top five span two cells and two rows; every cap below a map's wanted
                  cells grows the edge; the faces case reaches grid_coord's -2 and dim + 1 clamps on every axis

The largest |u| and the smallest margin (5th distance minus the tightest lower bound that applied to a true neighbour's cell, in
cells) are printed per case (pytest -s) and recorded in docs/kernels/scan2map.md.
"""
import functools

import numpy as np
import pytest

from tests import common
from tests import knn_grid_cases as gc
from tests import knn_grid_model as gm

GATE = np.float32(1.0)


@functools.lru_cache(maxsize=None)
def _pairs(name):
    """[(kind, map cloud, q (m, 3), p (m, 3), d4 (m,), cells_of_top5 helper data)] over both maps and all poses of a case: one row
    per (in-gate query, one of its top five)."""
    from oracle import oracle as orc
    orc.build()
    c = gc.case(name)
    out = []
    for kind, cloud, queries in (("corner", c.mc, c.corner), ("surf", c.ms, c.surf)):
        if len(cloud) < 5 or len(queries) == 0:
            continue
        Q, P, D, qid = [], [], [], []
        for k, pose in enumerate(c.poses):
            moved = orc.transform_cloud(queries, pose)
            for i, q in enumerate(moved[:, :3]):
                idx, d2 = orc.knn_brute(cloud, q)
                if not d2[4] < GATE:
                    continue
                for j in range(5):
                    Q.append(q); P.append(cloud[idx[j], :3]); D.append(d2[4]); qid.append(k * len(moved) + i)
        if Q:
            out.append((kind, cloud, np.array(Q, np.float32), np.array(P, np.float32), np.array(D, np.float32), np.array(qid)))
    return out


@pytest.mark.parametrize("name", gc.NAMES)
def test_no_true_neighbour_lies_in_a_cell_the_walk_may_skip(oracle, name):
    c = gc.case(name)
    rows = _pairs(name)
    if gc.too_small(c):
        assert len(rows) <= 1            # the small map takes no query; its descriptor is still checked below
    else:
        assert sum(len(r[2]) for r in rows) >= 5 * 10, "the case has hardly any query inside the gate"
    u_max, margin = 0.0, np.inf
    for kind, cloud, Q, P, D, _ in rows:
        for cap in gm.CAPS:
            g = gm.desc_of(cloud, cap)
            assert g.n_cells <= cap and max(g.dims) <= gm.MAX_DIM
            r = gm.may_skip(g, Q, P, D)
            bad = np.flatnonzero(r["any"])
            assert len(bad) == 0, "%s %s cap %d: query %s neighbour %s: reach %s row %s end %s" % (
                name, kind, cap, Q[bad[0]], P[bad[0]], r["reach"][bad[0]], r["row"][bad[0]], r["end"][bad[0]])
            u_max, margin = max(u_max, r["u_max"]), min(margin, float(r["margin"].min()))
    for cloud in (c.mc, c.ms):           # every descriptor terminates inside its cap, empty and one-point maps included
        for cap in gm.CAPS:
            g = gm.desc_of(cloud, cap)
            assert g.n_cells <= max(cap, 1) and min(g.dims) >= (2 if len(cloud) else 1)
    print("%-14s pairs %6d  largest |u| %9.1f  smallest margin %.3e cells" % (name, sum(len(r[2]) for r in rows), u_max, margin))


@pytest.mark.parametrize("name", gc.NAMES)
def test_caps_below_the_wanted_cells_grow_the_edge_and_small_boxes_keep_their_descriptor(name):
    c = gc.case(name)
    for cloud in (c.mc, c.ms):
        if len(cloud) == 0:
            continue
        base = gm.desc_of(cloud, 64 << 20, max_dim=None)
        assert base.steps == 0 and base.want_cells == base.n_cells
        for cap in gm.CAPS:
            g, old = gm.desc_of(cloud, cap), gm.desc_of(cloud, cap, max_dim=None)
            if cap < base.want_cells:
                assert g.steps > 0 and g.cell > base.cell and float(g.inv) < float(base.inv), (name, cap)
            if max(old.dims) <= gm.MAX_DIM:
                assert g.steps == old.steps and g.dims == old.dims and g.inv == old.inv and g.inv_x == old.inv_x
                assert g.cell2 == old.cell2 and g.cellx2 == old.cellx2 and np.array_equal(g.o, old.o), (name, cap)
            else:
                assert g.steps > old.steps


def test_the_bench_and_suite_maps_keep_their_descriptor():
    """The limit changes nothing below 4 096 cells per axis: the maps the benchmark and the GPU suite register against."""
    from msf_loam_amd import synth
    worlds = [common.small_world()[1:], synth.make_map(synth.World(ground_half=synth.ground_half_for_target(30000))),
              common.other_world("outdoor")[1:], common.other_world("corridor")[1:]]
    for clouds in worlds:
        for cloud in clouds:
            for cap in (65536, 1 << 20, 64 << 20):
                g, old = gm.desc_of(cloud, cap), gm.desc_of(cloud, cap, max_dim=None)
                assert max(old.dims) <= gm.MAX_DIM
                assert tuple(np.float32(x).tobytes() for x in (g.inv, g.inv_x, g.cell2, g.cellx2)) == \
                       tuple(np.float32(x).tobytes() for x in (old.inv, old.inv_x, old.cell2, old.cellx2))
                assert g.dims == old.dims and g.want_cells == old.want_cells and g.o.tobytes() == old.o.tobytes()


@pytest.mark.parametrize("name", list(gc.RODS))
def test_rods_are_not_vacuous(oracle, name):
    """In-gate queries whose top five lie in two cells, and in two (y, z) rows, of the base-edge grid (the geometry of the
    margins) -- and in two cells of the grid the descriptor really takes at the default span."""
    rows = [r for r in _pairs(name) if r[0] == "surf"]
    assert rows
    _, cloud, Q, P, D, qid = rows[0]
    counts = {}
    for label, g in (("base", gm.desc_of(cloud, max_dim=None)), ("built", gm.desc_of(cloud))):
        pc = gm.point_cell(P, g)
        n_q = len(Q) // 5
        cells = pc.reshape(n_q, 5, 3)
        two_cells = (cells != cells[:, :1]).any(2).any(1)
        two_rows = (cells[:, :, 1:] != cells[:, :1, 1:]).any(2).any(1)
        counts[label] = (int(two_cells.sum()), int(two_rows.sum()), n_q)
    print("%-12s queries in the gate %d: top five in two cells %d / two rows %d (base edge), two cells %d (as built)"
          % (name, counts["base"][2], counts["base"][0], counts["base"][1], counts["built"][0]))
    assert counts["base"][0] >= 20 and counts["base"][1] >= 5 and counts["built"][0] >= 20
    axis, length = gc.RODS[name]
    assert gm.desc_of(cloud, max_dim=None).want_cells <= gm.DEFAULT_CAP          # the case table says: all fit the default span


def test_faces_reach_both_clamps(oracle):
    from oracle import oracle as orc
    c = gc.case("faces")
    g = gm.desc_of(c.ms)
    q = orc.transform_cloud(c.surf, c.poses[0])[:, :3]
    for a, inv in enumerate((g.inv_x, g.inv, g.inv)):
        cell = gm.grid_coord(q[:, a], g.o[a], inv, g.dims[a])
        assert cell.min() == -2 and cell.max() == g.dims[a] + 1, (a, cell.min(), cell.max(), g.dims)
        raw = np.floor(gm.u_of(q[:, a], g.o[a], inv))
        assert raw.min() < -2 and raw.max() > g.dims[a] + 1                      # the clamp really cut something
        # and queries in the first and last cell, and one cell outside on either side
        assert {-1, 0, g.dims[a] - 2, g.dims[a] - 1} <= set(cell.tolist())
    # map points exactly on every face; the last cell of every axis holds the points of the far face
    mn, mx = gm.bbox_of(c.ms)
    p = c.ms[:, :3]
    for a in range(3):
        assert (p[:, a] == mn[a]).sum() >= 40 and (p[:, a] == mx[a]).sum() >= 40


TRIALS = 1000000


@pytest.mark.parametrize("name", list(gc.RODS))
def test_adversarial_search_at_the_rods_extents(name):
    axis, length = gc.RODS[name]
    lo, hi = gc.rod_box(axis, length)
    rng = np.random.default_rng(9000 + list(gc.RODS).index(name))
    res = {}
    for label, max_dim in (("built", gm.MAX_DIM), ("no limit", None)):
        g = gm.grid_desc(lo, hi, max_dim=max_dim)
        top = g.dims[axis] - 2
        res[label] = gm.adversarial(g, axis, max(1, top - 2000), top, TRIALS, rng)
        miss, margin, u_max, kinds = res[label]
        print("%-12s %-8s dims %-16s |u| <= %8.1f  misses %6d %s  smallest margin %+.3e cells" % (name, label, g.dims, u_max, miss, kinds, margin))
    assert res["built"][0] == 0 and res["built"][1] > 0
    assert res["built"][2] <= gm.MAX_DIM + 1
    if name in ("rod_x_6km", "rod_y_12km"):
        # the search has teeth: without the limit these extents lose true neighbours
        assert res["no limit"][0] > 1000 and res["no limit"][1] < 0
        assert res["no limit"][3]["end" if axis == 0 else "row"] > 1000


def test_the_error_bound_behind_kGridMaxDim():
    """2^-22 |u| cells, the rounding error of the difference of two computed coordinates, stays below both absolute margins
    (the 1e-3 slack of axis_gap and the 0.1 % edge margin) for |u| <= MAX_DIM + 1, and would not one binade further."""
    worst = 2.0 ** -22 * (gm.MAX_DIM + 1)
    assert worst < 1.0 - 1.0 / gm.EDGE_MARGIN < float(gm.SLACK)
    assert 2.0 ** -22 * (2 * gm.MAX_DIM) > float(gm.SLACK)
    # measured: over the top cells of a MAX_DIM-cell axis the computed difference is never further off than the bound
    rng = np.random.default_rng(5)
    lo, hi = gc.rod_box(1, gm.MAX_DIM * gm.EDGE_MARGIN - 3.0)
    g = gm.grid_desc(lo, hi)
    assert g.steps == 0 and g.dims[1] > gm.MAX_DIM - 4
    v = (float(hi[1]) - rng.uniform(0, 50, 200000)).astype(np.float32)
    w = (v.astype(np.float64) - rng.uniform(0, 1, len(v))).astype(np.float32)
    true = (v.astype(np.float64) - w.astype(np.float64)) / g.cell
    got = gm.u_of(v, g.o[1], g.inv).astype(np.float64) - gm.u_of(w, g.o[1], g.inv).astype(np.float64)
    err = np.abs(got - true).max()
    print("largest error of a coordinate difference at |u| ~ %d: %.3e cells (bound %.3e)" % (g.dims[1], err, worst))
    assert err <= worst
