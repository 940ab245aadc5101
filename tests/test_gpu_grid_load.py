"""msfl_grid_load_cells / msfl_grid_crop_tiles: dumped or evicted cells come back bit for bit.  Against oracle.HybridGrid (through
the never-cropped model of tests/windowed_grid_model.py, which adds the cell list) and the tiled model of tests/tiled_grid_model.py."""
import functools
import os
import re

import numpy as np
import pytest

from tests import tiled_grid_model as tm
from tests import windowed_grid_model as wm
from tests.test_grid_store import _batches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _bs():
    return _batches(5)


def _queries():
    bs = _bs()
    return [(bs[1][0], bs[1][2]), (bs[0][0], bs[0][2])]


def _same_map(gg, m, what):
    assert gg.size() == m.size(), what
    assert np.array_equal(gg.dump(), m.dump()), what
    assert np.array_equal(gg.dump_cells(), m.dump_cells()), what
    for scan, pose in _queries():
        assert np.array_equal(gg.get_surrounded(scan, pose), m.get_surrounded(scan, pose)), what


def _snapshot(gg):
    return (gg.size(), gg.dump().tobytes(), gg.dump_cells().tobytes(), gg.get_surrounded(*_queries()[0]).tobytes())


def _split(cells, pts, pick):
    """the cells `pick` (indices) of a (cells, points) pair, with their points"""
    start = np.concatenate([[0], np.cumsum(cells[:, 3])])
    sub = [pts[start[c]:start[c + 1]] for c in pick]
    return cells[pick], (np.concatenate(sub) if sub else np.zeros((0, 4), np.float32))


@pytest.mark.parametrize("leaf,min_pool", [(0.2, None), (0.4, None), (0.4, 1024)])
def test_dump_loaded_into_a_fresh_store_is_the_same_store(gpu, oracle, monkeypatch, leaf, min_pool):
    """Four inserts into A; dump() + dump_cells() of A loaded into an empty B.  B equals A and the oracle grid; a fifth insert (its
    re-filter reads loaded slabs and loaded centroids in stored order) leaves all three equal.  With a 1 024-point minimum pool B
    compacts between the load and the insert."""
    from msf_loam_amd import capi
    if min_pool:
        monkeypatch.setenv("MSFL_GRID_MIN_POOL", str(min_pool))
    bs = _bs()
    a, b, m = capi.Grid(gpu, 3.0, leaf), capi.Grid(gpu, 3.0, leaf), wm.WindowedGrid(oracle, 3.0, leaf)
    for _, wp, _ in bs[:4]:
        a.insert_scan(wp)
        assert m.insert_scan(wp) == 0
    cells, pts = a.dump_cells(), a.dump()
    info = b.load_cells(cells, pts)
    assert info.status == capi.OK and info.as_tuple() == (len(cells), len(pts), len(cells), len(pts), 0, 0, 1)
    assert b.size() == a.size() and b.stats()["n_points"] == len(pts)
    if min_pool:
        assert b.stats()["pool_capacity_points"] < (1 << 20)
    _same_map(a, m, "A")
    _same_map(b, m, "B")
    a.insert_scan(bs[4][1]); b.insert_scan(bs[4][1])
    assert m.insert_scan(bs[4][1]) == 0
    _same_map(a, m, "A, fifth insert")
    _same_map(b, m, "B, fifth insert")
    a.close(); b.close()


@pytest.mark.parametrize("leaf", [0.2, 0.4])
def test_evict_and_reload(gpu, oracle, leaf):
    """Inserts 1, 2 -> crop_tiles (2, 2, 1) -> load_cells of exactly what it delivered: the store before the crop and the never-cropped
    oracle grid, byte for byte, also through inserts 3 and 4.  On a twin: crop, reload every other evicted cell, against the tiled
    model.  crop_tiles equals crop on the twin and the model's evicted cell list; too small a cell_capacity refuses it."""
    from msf_loam_amd import capi
    bs = _bs()
    gg, twin = capi.Grid(gpu, 3.0, leaf), capi.Grid(gpu, 3.0, leaf)
    never, tiled = wm.WindowedGrid(oracle, 3.0, leaf), tm.TiledGrid(oracle, 3.0, leaf)
    for _, wp, _ in bs[:2]:
        gg.insert_scan(wp); twin.insert_scan(wp)
        assert never.insert_scan(wp) == 0 and tiled.insert_scan(wp) == 0
    before = _snapshot(gg)
    n_pts, n_cells = gg.size()
    centre, half = bs[1][2][:3], (2, 2, 1)
    info_m, cells_m, pts_m = tiled.crop(centre, half, keep_evicted=True)
    assert len(cells_m) > 3 and info_m.n_cells > 0
    # one cell record short: refused as a whole, the counts name the need
    info, cells_e, pts_e = gg.crop_tiles(centre, half, cell_capacity=len(cells_m) - 1, allow=(capi.CAPACITY,))
    assert info.status == capi.CAPACITY and info.applied == 0 and len(cells_e) == 0 and len(pts_e) == 0
    assert (info.n_cells_evicted, info.n_points_evicted, info.n_cells, info.n_points) == (len(cells_m), len(pts_m), n_cells, n_pts)
    assert _snapshot(gg) == before
    info, cells_e, pts_e = gg.crop_tiles(centre, half, capacity=len(pts_m), cell_capacity=len(cells_m))
    info_t, ev_t = twin.crop(centre, half, keep_evicted=True)
    assert info.status == capi.OK and info.as_tuple() == info_t.as_tuple() == info_m.as_tuple()
    assert np.array_equal(pts_e, ev_t) and np.array_equal(pts_e, pts_m) and np.array_equal(cells_e, cells_m)
    assert cells_e.dtype == np.int32 and cells_e[:, 3].sum() == len(pts_e)
    _same_map(gg, tiled, "cropped")
    _same_map(twin, tiled, "twin cropped")
    # everything back
    li, flags = gg.load_cells(cells_e, pts_e, want_conflicts=True)
    assert li.status == capi.OK and li.as_tuple() == (len(cells_e), len(pts_e), n_cells, n_pts, 0, 0, 1) and not flags.any()
    assert _snapshot(gg) == before
    _same_map(gg, never, "reloaded")
    for k in (2, 3):
        gg.insert_scan(bs[k][1])
        assert never.insert_scan(bs[k][1]) == 0
        _same_map(gg, never, ("reloaded, insert", k))
    # every other evicted cell only
    pick = np.arange(0, len(cells_e), 2)
    sub_cells, sub_pts = _split(cells_e, pts_e, pick)
    li = twin.load_cells(sub_cells, sub_pts)
    assert li.as_tuple()[:2] == (len(sub_cells), len(sub_pts)) and li.applied == 1
    tiled.load_cells(wm.cell_key(sub_cells[:, :3]))
    _same_map(twin, tiled, "partial reload")
    twin.insert_scan(bs[2][1])
    assert tiled.insert_scan(bs[2][1]) == 0
    _same_map(twin, tiled, "partial reload, insert")
    gg.close(); twin.close()


def _np_surround(cells, pts, scan):
    """GetSurroundedCloud with the identity pose over a (cells, points) pair: the slabs of the cells hit by p + {-1, 0, 1}^3 m"""
    hit = set()
    for o in np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1]), -1).reshape(-1, 3):
        hit.update(wm.cell_key(wm.cell_index(scan[:, :3] + o.astype(np.float32), 3.0)).tolist())
    keys = wm.cell_key(cells[:, :3])
    return _split(cells, pts, np.array([c for c in range(len(cells)) if int(keys[c]) in hit], np.int64))[1]


def test_merge_positions(gpu):
    """Hand-made one- and two-point cells: listed cells before, between and after all live keys; into an empty store; into a table
    cropped to zero cells; an empty list.  The point of cell (1, 0, 0) lies at x = 4.5, which InsertScan would file under cell 2:
    a load does not re-derive the cell."""
    from msf_loam_amd import capi
    live_pts = np.array([[0.1, 0.2, 0.1, 0.01], [6.1, 0.2, 0.1, 0.02], [12.1, 0.2, 0.1, 0.03]], np.float32)          # cells 0, 2, 4 along x
    listed = np.array([[5, 5, -1, 1], [-3, 0, 0, 2], [1, 0, 0, 1], [3, 0, 0, 1], [7, 0, 0, 1], [0, 1, 0, 1], [2, 0, 1, 2]], np.int32)
    pts = np.array([[15.0, 15.1, -3.2, 0.1], [-9.1, 0.1, 0.0, 0.2], [-8.9, -0.4, 0.3, 0.3], [4.5, 0.2, 0.1, 0.4], [9.3, 0.0, 0.0, 0.5],
                    [21.0, 0.5, 0.5, 0.6], [0.2, 3.1, 0.0, 0.7], [6.0, 0.0, 3.0, 0.8], [6.2, 0.1, 3.3, 0.9]], np.float32)
    assert (np.diff(wm.cell_key(listed[:, :3])) > 0).all()
    scan = np.concatenate([live_pts, pts])
    pose = np.array([0, 0, 0, 0, 0, 0, 1], np.float64)
    g = capi.Grid(gpu, 3.0, 0.4)
    g.insert_scan(live_pts)
    live_cells = g.dump_cells()
    assert live_cells.tolist() == [[0, 0, 0, 1], [2, 0, 0, 1], [4, 0, 0, 1]]
    g.get_surrounded(scan, pose)                                               # the live cells carry a stamp, the loaded ones start at 0
    info = g.load_cells(listed, pts)
    assert info.as_tuple() == (7, 9, 10, 12, 0, 0, 1)
    want_cells, want_pts = wm.merge_cellwise(live_cells, live_pts, listed, pts)
    assert np.array_equal(g.dump_cells(), want_cells) and np.array_equal(g.dump(), want_pts) and g.size() == (12, 10)
    assert np.array_equal(g.get_surrounded(scan, pose), want_pts)
    near = np.array([[4.5, 0.2, 0.1, 0], [0.2, 3.1, 0.0, 0]], np.float32)
    got = g.get_surrounded(near, pose)
    assert np.array_equal(got, _np_surround(want_cells, want_pts, near)) and 0 < len(got) < 12
    g.close()
    # an empty store, then a table cropped to zero cells, then an empty list
    g = capi.Grid(gpu, 3.0, 0.4)
    for round_ in range(2):
        info = g.load_cells(listed, pts)
        assert info.as_tuple() == (7, 9, 7, 9, 0, 0, 1), round_
        assert np.array_equal(g.dump_cells(), listed) and np.array_equal(g.dump(), pts) and g.size() == (9, 7)
        assert np.array_equal(g.get_surrounded(near, pose), _np_surround(listed, pts, near))
        info = g.load_cells(np.zeros((0, 4), np.int32), np.zeros((0, 4), np.float32))
        assert info.as_tuple() == (0, 0, 7, 9, 0, 0, 1) and info.status == capi.OK
        assert np.array_equal(g.dump_cells(), listed) and np.array_equal(g.dump(), pts)
        c = g.crop((3000.0, 0, 0), (0, 0, 0))
        assert c.n_cells_evicted == 7 and g.size() == (0, 0)
    assert g.load_cells(np.zeros((0, 4), np.int32), np.zeros((0, 4), np.float32)).as_tuple() == (0, 0, 0, 0, 0, 0, 1)
    g.close()


@functools.lru_cache(maxsize=None)
def _refusal_reference(oracle_mod):
    """the oracle grid after inserts 1, 2 and after insert 3: (size, dump) each, computed once"""
    bs = _bs()
    m = oracle_mod.HybridGrid(3.0, 0.4)
    m.insert_scan(bs[0][1]); m.insert_scan(bs[1][1])
    two = (m.size(), m.dump())
    m.insert_scan(bs[2][1])
    return two, (m.size(), m.dump())


_FAR = np.array([[100, 0, 0, 1], [101, 0, 0, 1], [102, 0, 0, 2]], np.int32)
_FAR_PTS = np.array([[300.1, 0, 0, 0.1], [303.2, 0.1, 0, 0.2], [306.0, 0, 0.1, 0.3], [306.4, 0, 0.1, 0.4]], np.float32)


def _edit(cells=_FAR, pts=_FAR_PTS, **kw):
    cells, pts = cells.copy(), pts.copy()
    for k, v in kw.items():
        if k == "cell":
            cells[v[0]] = v[1]
        elif k == "point":
            pts[v[0], v[1]] = v[2]
        elif k == "drop_point":
            pts = pts[:-1]
    return cells, pts


@pytest.mark.parametrize("case", ["conflict", "nan", "inf", "descending", "duplicate", "zero_count", "negative_count", "wrong_sum", "index_8192",
                                  "index_below"])
def test_refusals_leave_the_store_as_it_was(gpu, oracle, case):
    from msf_loam_amd import capi
    bs = _bs()
    (size2, dump2), (size3, dump3) = _refusal_reference(oracle)
    g = capi.Grid(gpu, 3.0, 0.4)
    g.insert_scan(bs[0][1]); g.insert_scan(bs[1][1])
    before = _snapshot(g)
    assert g.size() == size2 and np.array_equal(g.dump(), dump2)
    if case == "conflict":
        all_cells = g.dump_cells()
        live = all_cells[[1, len(all_cells) // 2]]
        live[:, 3] = 1
        cells, pts = wm.merge_cellwise(_FAR, _FAR_PTS, live, np.full((2, 4), 0.5, np.float32))         # key order
        info, flags = g.load_cells(cells, pts, allow=(capi.BAD_ARG,), want_conflicts=True)
        is_live = np.isin(wm.cell_key(cells[:, :3]), wm.cell_key(live[:, :3]))
        assert info.status == capi.BAD_ARG and info.as_tuple() == (0, 0, size2[1], size2[0], 2, 0, 0)
        assert np.array_equal(flags, is_live.astype(np.int32)) and flags.sum() == 2
        # the caller splits the list on the flags: the others go through
        ok_cells, ok_pts = _split(cells, pts, np.flatnonzero(flags == 0))
        g2 = capi.Grid(gpu, 3.0, 0.4)
        g2.insert_scan(bs[0][1]); g2.insert_scan(bs[1][1])
        assert g2.load_cells(ok_cells, ok_pts).as_tuple() == (3, 4, size2[1] + 3, size2[0] + 4, 0, 0, 1)
        g2.close()
    elif case in ("nan", "inf"):
        cells, pts = _edit(point=(2, 1, np.nan if case == "nan" else np.inf))
        info = g.load_cells(cells, pts, allow=(capi.CAPACITY,))
        assert info.status == capi.CAPACITY and info.as_tuple() == (0, 0, size2[1], size2[0], 0, 1, 0)
    else:
        cells, pts = {
            "descending": lambda: _edit(cell=(1, [99, 0, 0, 1])),
            "duplicate": lambda: _edit(cell=(1, [100, 0, 0, 1])),
            "zero_count": lambda: _edit(cell=(1, [101, 0, 0, 0])),
            "negative_count": lambda: _edit(cell=(1, [101, 0, 0, -1])),
            "wrong_sum": lambda: _edit(drop_point=True),
            "index_8192": lambda: _edit(cell=(2, [8192, 0, 0, 2])),
            "index_below": lambda: _edit(cell=(0, [100, -8193, 0, 1])),
        }[case]()
        with pytest.raises(capi.MsflError) as e:
            g.load_cells(cells, pts)
        assert "msfl_grid_load_cells: " in str(e.value).split(") ", 1)[1] and e.value.status == capi.BAD_ARG      # msfl_last_error names the entry
    assert _snapshot(g) == before
    g.insert_scan(bs[2][1])
    assert g.size() == size3 and np.array_equal(g.dump(), dump3)
    g.close()


def test_null_arguments(gpu):
    from msf_loam_amd import capi
    g = capi.Grid(gpu, 3.0, 0.4)
    C = capi.C
    info = capi.GridLoadInfo()
    cells, pts = np.ascontiguousarray(_FAR), np.ascontiguousarray(_FAR_PTS)
    f = g.lib.msfl_grid_load_cells
    assert f(g.g, None, 0, None, 0, 0, None, None) == capi.BAD_ARG                                                   # info == NULL
    assert f(g.g, None, 3, capi._vp(pts), 4, 0, None, C.byref(info)) == capi.BAD_ARG
    assert f(g.g, capi._vp(cells), 3, None, 4, 0, None, C.byref(info)) == capi.BAD_ARG
    assert f(g.g, capi._vp(cells), -1, capi._vp(pts), 4, 0, None, C.byref(info)) == capi.BAD_ARG
    assert f(g.g, capi._vp(cells), 3, capi._vp(pts), -4, 0, None, C.byref(info)) == capi.BAD_ARG
    assert g.size() == (0, 0)
    c3, h3 = (C.c_double * 3)(0, 0, 0), (C.c_int * 3)(1, 1, 1)
    ci = capi.GridCropInfo()
    out_c = np.zeros((4, 4), np.int32)
    assert g.lib.msfl_grid_crop_tiles(g.g, c3, h3, None, 0, capi._vp(out_c), 4, 0, C.byref(ci)) == capi.BAD_ARG     # `evicted` is required
    assert g.lib.msfl_grid_crop_tiles(g.g, c3, h3, capi._vp(pts), 4, None, 4, 0, C.byref(ci)) == capi.BAD_ARG
    assert g.lib.msfl_grid_crop_tiles(g.g, c3, h3, capi._vp(pts), 4, capi._vp(out_c), 4, 0, C.byref(ci)) == capi.OK   # an empty store
    assert ci.as_tuple() == (0, 0, 0, 0, (0, 0, 0), 1)
    g.close()


def _one_block_max():
    src = open(os.path.join(ROOT, "msf_loam_amd", "csrc", "msfl_grid.cuh")).read()
    return int(eval(re.search(r"constexpr int kGridOneBlockMax = ([0-9 <]+);", src).group(1)))


@pytest.mark.parametrize("scale", [1, 2])
def test_both_table_forms_merge_the_same_way(gpu, scale):
    """scale 1: kGridOneBlockMax + 1 one-point cells, half of them loaded into a store that holds the other half, interleaved (the
    one-workgroup plan).  scale 2: twice as many, so that the listed half alone exceeds kGridOneBlockMax (the flag kernel and the
    device-wide scan) and the cell tables grow inside the load.  Against numpy set arithmetic on the keys."""
    from msf_loam_amd import capi
    n = scale * (_one_block_max() + 1)
    w = 512
    k = np.arange(n)
    idx = np.stack([k % w - w // 2, k // w - (n // w) // 2, np.zeros(n, np.int64)], axis=1)
    pts = np.zeros((n, 4), np.float32)
    pts[:, :3] = idx * 3.0 + np.array([0.3, -0.2, 0.1])
    pts[:, 3] = (k % 97) / 1000.0
    keys = wm.cell_key(wm.cell_index(pts[:, :3], 3.0))
    order = np.argsort(keys)
    by_key, cells = pts[order], np.c_[wm.key_cell(keys[order]), np.ones(n, np.int64)].astype(np.int32)
    odd = np.arange(n) % 2 == 1                                   # in key order: every other cell is live, the ones between are listed
    g = capi.Grid(gpu, 3.0, 0.4)
    g.insert_scan(by_key[odd][np.random.default_rng(5).permutation(int(odd.sum()))])
    assert g.size() == (int(odd.sum()), int(odd.sum()))
    cap_before = g.stats()["cell_capacity"]
    n_list = int((~odd).sum())
    assert (n_list > _one_block_max()) == (scale == 2)
    info = g.load_cells(cells[~odd], by_key[~odd])
    assert info.as_tuple() == (n_list, n_list, n, n, 0, 0, 1)
    assert np.array_equal(g.dump_cells(), cells) and np.array_equal(g.dump(), by_key)
    if scale == 2:
        assert cap_before < n <= g.stats()["cell_capacity"]
    # all of them again: every listed cell conflicts, nothing moves
    info, flags = g.load_cells(cells[~odd], by_key[~odd], allow=(capi.BAD_ARG,), want_conflicts=True)
    assert info.as_tuple() == (0, 0, n, n, n_list, 0, 0) and flags.all()
    assert np.array_equal(g.dump_cells(), cells) and np.array_equal(g.dump(), by_key)
    g.close()


def test_device_pointer_form_equals_the_host_form(gpu):
    import torch
    from msf_loam_amd import capi
    bs = _bs()
    src = capi.Grid(gpu, 3.0, 0.4)
    src.insert_scan(bs[0][1])
    cells, pts = src.dump_cells(), src.dump()
    src.close()
    host, dev = capi.Grid(gpu, 3.0, 0.4), capi.Grid(gpu, 3.0, 0.4)
    t = torch.from_numpy(pts).to("cuda:0")
    torch.cuda.synchronize()
    i_h = host.load_cells(cells, pts)
    i_d, flags = dev.load_cells_device(cells, t, len(pts), want_conflicts=True)
    assert i_h.as_tuple() == i_d.as_tuple() == (len(cells), len(pts), len(cells), len(pts), 0, 0, 1) and not flags.any()
    assert np.array_equal(dev.dump(), host.dump()) and np.array_equal(dev.dump(), pts) and np.array_equal(dev.dump_cells(), cells)
    assert np.array_equal(t.cpu().numpy(), pts)
    host.insert_scan(bs[1][1]); dev.insert_scan(bs[1][1])
    assert np.array_equal(dev.dump(), host.dump()) and np.array_equal(dev.dump_cells(), host.dump_cells())
    host.close(); dev.close()
