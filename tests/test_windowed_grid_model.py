"""CPU tests of tests/windowed_grid_model.py, the model the windowed map store (msfl_grid_crop) is compared with."""
import numpy as np

from tests import windowed_grid_model as wm
from tests.test_grid_store import _batches


def _blob(center, n, seed):
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 4), np.float32)
    p[:, :3] = np.asarray(center) + rng.uniform(-1.2, 1.2, (n, 3))
    p[:, 3] = rng.uniform(0, 0.1, n)
    return p


def test_cell_index_rounds_half_away_from_zero():
    assert list(wm.cell_index(np.array([1.5, -1.5, 4.5, 1.4999, -1.4999, 0.0], np.float32), 3.0)) == [1, -1, 2, 0, 0, 0]
    idx = np.array([[0, 0, 0], [-1, 0, 0], [5, -7, 2], [-8192, 8191, 0]])
    assert np.array_equal(wm.key_cell(wm.cell_key(idx)), idx)
    assert list(np.argsort(wm.cell_key(np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0]])))) == [3, 0, 1, 2]      # z major, x minor


def test_two_cells_one_evicted_then_touched_again_starts_fresh(oracle):
    """Cells (0,0,0) and (4,0,0); a window of one cell around the origin evicts the second; a later insert into it must build
    the cell from that insert alone, while the kept cell goes on merging with its old centroids."""
    a0, b0, a1, b1 = _blob((0, 0, 0), 200, 1), _blob((12, 0, 0), 200, 2), _blob((0, 0, 0), 50, 3), _blob((12, 0, 0), 50, 4)
    m = wm.WindowedGrid(oracle, 3.0, 0.4)
    assert m.insert_scan(np.concatenate([a0, b0])) == 0
    assert m.size()[1] == 2 and [tuple(c[:3]) for c in m.dump_cells()] == [(0, 0, 0), (4, 0, 0)]
    both = oracle.HybridGrid(3.0, 0.4); both.insert_scan(np.concatenate([a0, b0]))
    assert np.array_equal(m.dump(), both.dump())
    only_b = oracle.HybridGrid(3.0, 0.4); only_b.insert_scan(b0)
    info, cells, pts = m.crop((0.2, -0.3, 0.1), (1, 1, 1), keep_evicted=True)
    assert info.as_tuple() == (1, len(only_b.dump()), 1, m.size()[0], (0, 0, 0), 1)
    assert cells.tolist() == [[4, 0, 0, len(pts)]] and np.array_equal(pts, only_b.dump())
    only_a = oracle.HybridGrid(3.0, 0.4); only_a.insert_scan(a0)
    assert m.size() == only_a.size() and np.array_equal(m.dump(), only_a.dump())
    # touched again: (0,0,0) merges with its centroids, (4,0,0) starts from b1 alone
    assert m.insert_scan(np.concatenate([b1, a1])) == 0
    want = oracle.HybridGrid(3.0, 0.4); want.insert_scan(a0); want.insert_scan(np.concatenate([b1, a1]))
    assert np.array_equal(m.dump(), want.dump()) and m.size() == want.size()
    never = oracle.HybridGrid(3.0, 0.4); never.insert_scan(np.concatenate([a0, b0])); never.insert_scan(np.concatenate([b1, a1]))
    assert not np.array_equal(m.dump(), never.dump())                      # the premise: forgetting the cell changed what it holds now
    fresh_b = oracle.HybridGrid(3.0, 0.4); fresh_b.insert_scan(b1)
    assert m.dump_cells().tolist()[1] == [4, 0, 0, fresh_b.size()[0]]
    # a crop that evicts nothing, one that evicts everything, a crop of the empty model
    before = m.dump()
    assert m.crop((0, 0, 0), (4, 0, 0)).as_tuple()[:2] == (0, 0) and np.array_equal(m.dump(), before)
    info = m.crop((300.0, 0, 0), (0, 0, 0))
    assert info.as_tuple() == (2, len(before), 0, 0, (100, 0, 0), 1) and m.size() == (0, 0) and len(m.dump()) == 0
    assert m.crop((0, 0, 0), (1, 1, 1)).as_tuple() == (0, 0, 0, 0, (0, 0, 0), 1)
    assert m.insert_scan(np.array([[3e4, 0, 0, 0]], np.float32)) == 7 and m.size() == (0, 0)


def test_dump_before_is_the_cellwise_merge_of_dump_after_and_evicted(oracle):
    """On real scans (the four 600-azimuth scans of the map-store tests): per-cell slabs concatenate to the replayed grid's
    dump (cells evolve independently), and what a crop takes out plus what it leaves is what was there."""
    bs = _batches()
    m = wm.WindowedGrid(oracle, 3.0, 0.4)
    for k, (scan, wp, pose) in enumerate(bs):
        assert m.insert_scan(wp) == 0
        if k % 2 == 1:
            cells_b, dump_b = m.dump_cells(), m.dump()
            assert cells_b[:, 3].sum() == len(dump_b) == m.size()[0] and len(cells_b) == m.size()[1]
            slabs = np.concatenate([m._cell_points(int(key)) for key in wm.cell_key(cells_b[:, :3])])
            assert np.array_equal(slabs, dump_b)
            info, cells_e, pts_e = m.crop(pose[:3] + np.array([9.0 if k == 3 else 0.0, 0, 0]), (2, 2, 1), keep_evicted=True)
            assert info.n_cells_evicted == len(cells_e) > 0 and info.n_points_evicted == len(pts_e) > 0
            assert (info.n_points, info.n_cells) == m.size() and info.n_cells > 0
            cells_m, dump_m = wm.merge_cellwise(m.dump_cells(), m.dump(), cells_e, pts_e)
            assert np.array_equal(cells_m, cells_b) and np.array_equal(dump_m, dump_b)
            inside = np.abs(m.dump_cells()[:, :3] - np.array(info.center_cell)) <= np.array([2, 2, 1])
            assert inside.all() and not (np.abs(cells_e[:, :3] - np.array(info.center_cell)) <= np.array([2, 2, 1])).all(axis=1).any()
    # the surround query sees the cropped map: a subset of what the uncropped grid delivers
    full = oracle.HybridGrid(3.0, 0.4)
    for _, wp, _ in bs:
        full.insert_scan(wp)
    s_m, s_f = m.get_surrounded(bs[3][0], bs[3][2]), full.get_surrounded(bs[3][0], bs[3][2])
    assert 0 < len(s_m) < len(s_f)
