"""CPU tests of tests/tiled_grid_model.py, the model msfl_grid_load_cells is compared with."""
import numpy as np

from tests import tiled_grid_model as tm
from tests import windowed_grid_model as wm
from tests.test_grid_store import _batches


def _without(pts, keys, resolution=3.0):
    """the points of `pts` whose cell is not in `keys`"""
    k = wm.cell_key(wm.cell_index(pts[:, :3], resolution))
    return pts[~np.isin(k, np.array(sorted(keys), np.int64))]


def _same(m, o, queries):
    assert m.size() == o.size() and np.array_equal(m.dump(), o.dump())
    for scan, pose in queries:
        assert np.array_equal(m.get_surrounded(scan, pose), o.get_surrounded(scan, pose))


def test_crop_and_full_reload_is_the_never_cropped_grid(oracle):
    bs = _batches()
    queries = [(bs[1][0], bs[1][2]), (bs[0][0], bs[0][2])]
    m, never = tm.TiledGrid(oracle, 3.0, 0.4), oracle.HybridGrid(3.0, 0.4)
    for _, wp, _ in bs[:2]:
        assert m.insert_scan(wp) == 0 and never.insert_scan(wp) == 0
    cells_b = m.dump_cells()
    info, cells_e, pts_e = m.crop(bs[1][2][:3], (2, 2, 1), keep_evicted=True)
    assert info.n_cells_evicted > 0 and info.n_cells > 0 and m.size()[0] < never.size()[0]
    assert sorted(m.parked) == sorted(wm.cell_key(cells_e[:, :3]).tolist())
    m.load_cells(wm.cell_key(cells_e[:, :3]))
    assert not m.parked and np.array_equal(m.dump_cells(), cells_b)
    _same(m, never, queries)
    for _, wp, _ in bs[2:]:                                   # the re-filter of a later insert reads a loaded cell like one that never left
        assert m.insert_scan(wp) == 0 and never.insert_scan(wp) == 0
        _same(m, never, queries)


def test_partial_reload_is_the_replay_without_the_cells_still_parked(oracle):
    bs = _batches()
    queries = [(bs[1][0], bs[1][2]), (bs[0][0], bs[0][2])]
    m = tm.TiledGrid(oracle, 3.0, 0.2)
    for _, wp, _ in bs[:2]:
        assert m.insert_scan(wp) == 0
    _, cells_e, _ = m.crop(bs[1][2][:3], (2, 2, 1), keep_evicted=True)
    keys_e = wm.cell_key(cells_e[:, :3])
    assert len(keys_e) > 3
    m.load_cells(keys_e[::2])
    still = set(keys_e[1::2].tolist())
    assert set(m.parked) == still
    want = oracle.HybridGrid(3.0, 0.2)
    for _, wp, _ in bs[:2]:
        assert want.insert_scan(_without(wp, still)) == 0
    _same(m, want, queries)
    live = set(wm.cell_key(m.dump_cells()[:, :3]).tolist())
    assert set(keys_e[::2].tolist()) <= live and not (still & live)
    # a later insert creates parked cells again, from nothing; what was parked stays parked
    assert m.insert_scan(bs[2][1]) == 0 and want.insert_scan(bs[2][1]) == 0
    _same(m, want, queries)
    assert set(m.parked) == still


def test_a_second_eviction_parks_what_the_cell_held_then(oracle):
    a0, a1 = np.array([[12.1, 0.2, 0.1, 0.5]], np.float32), np.array([[12.7, 0.4, 0.1, 0.25]], np.float32)
    m = tm.TiledGrid(oracle, 3.0, 0.4)
    m.insert_scan(a0)
    m.crop((0, 0, 0), (1, 1, 1))
    m.insert_scan(a1)
    m.crop((0, 0, 0), (1, 1, 1))
    m.load_cells(list(m.parked))
    want = oracle.HybridGrid(3.0, 0.4); want.insert_scan(a1)
    assert m.size() == (1, 1) and np.array_equal(m.dump(), want.dump())
