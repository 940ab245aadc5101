"""CPU model of the windowed map store: oracle.HybridGrid (insert, surround, dump -- no removal) plus a crop.

HybridGrid::InsertScan files every point under its 3 m cell and re-runs the voxel filter over each TOUCHED cell's own
cloud (hybrid_grid.cc:503-521): cells evolve independently of each other.  The state after any sequence of inserts and
crops is therefore exactly that of a fresh oracle grid fed the history again, each historic insert reduced to the points
whose cell was not outside the window of any crop after that insert -- an evicted cell that is touched again starts from
nothing.  The model keeps the history and rebuilds by replay (O(history): fine at test sizes); a single cell's slab is
the dump of a fresh grid fed that cell's points only, which is how a dump is split into cells.

A point's cell is lround(f64(f32(p) / f32(resolution))), half away from zero (tests/test_grid_store.py::_np_grid)."""
import numpy as np

LIM = 8192          # +-8192 cells per axis (hybrid_grid.cc:460)
BITS = 14


def cell_index(v, resolution):
    """lround(double(f32 v / f32 resolution)) of an array of coordinates."""
    f = (np.asarray(v, np.float32) / np.float32(resolution)).astype(np.float64)
    return np.where(np.abs(f - np.trunc(f)) == 0.5, np.trunc(f) + np.sign(f), np.round(f)).astype(np.int64)


def cell_key(idx):
    """(n, 3) cell indices -> keys that sort like the store's table: (iz, iy, ix) ascending."""
    idx = np.asarray(idx, np.int64)
    return ((idx[..., 2] + LIM) << (2 * BITS)) | ((idx[..., 1] + LIM) << BITS) | (idx[..., 0] + LIM)


def key_cell(key):
    key = np.asarray(key, np.int64)
    m = (1 << BITS) - 1
    return np.stack([(key & m) - LIM, ((key >> BITS) & m) - LIM, (key >> (2 * BITS)) - LIM], axis=-1)


def merge_cellwise(cells_a, pts_a, cells_b, pts_b):
    """Two (cells (m, 4) {ix, iy, iz, count}, points) pairs over disjoint cell sets -> the pair of their union, cells ascending."""
    cells = np.concatenate([np.asarray(cells_a, np.int64).reshape(-1, 4), np.asarray(cells_b, np.int64).reshape(-1, 4)])
    pts = np.concatenate([np.asarray(pts_a, np.float32).reshape(-1, 4), np.asarray(pts_b, np.float32).reshape(-1, 4)])
    start = np.concatenate([[0], np.cumsum(cells[:, 3])])
    keys = cell_key(cells[:, :3])
    assert len(np.unique(keys)) == len(keys), "the two cell sets overlap"
    order = np.argsort(keys, kind="stable")
    out = [pts[start[c]:start[c + 1]] for c in order]
    return cells[order].astype(np.int32), (np.concatenate(out) if out else np.zeros((0, 4), np.float32))


class CropInfo:
    def __init__(self, n_cells_evicted, n_points_evicted, n_cells, n_points, center_cell, applied=1):
        self.n_cells_evicted, self.n_points_evicted, self.n_cells, self.n_points = n_cells_evicted, n_points_evicted, n_cells, n_points
        self.center_cell, self.applied = tuple(int(c) for c in center_cell), applied

    def as_tuple(self):
        return (self.n_cells_evicted, self.n_points_evicted, self.n_cells, self.n_points, self.center_cell, self.applied)


class WindowedGrid:
    """insert_scan / crop / dump / dump_cells / size / get_surrounded with the semantics of msfl_grid_*."""

    def __init__(self, oracle, resolution=3.0, leaf=0.2):
        self.o, self.resolution, self.leaf = oracle, float(resolution), float(leaf)
        self.history = []           # per insert: (points, {cell key: indices of the cell's live points, scan order})
        self._grid = None           # replay of the history, dropped by a crop that evicts

    # ---- the history ----
    def insert_scan(self, pts):
        pts = np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 4))
        if len(pts) == 0:
            return 0
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(pts[:, :3]).all()
            idx = cell_index(np.where(np.isfinite(pts[:, :3]), pts[:, :3], 0), self.resolution)
        if not ok or (idx < -LIM).any() or (idx >= LIM).any():
            rc = self.o.HybridGrid(self.resolution, self.leaf).insert_scan(pts)
            assert rc != 0
            return rc                                           # dropped as a whole
        keys = cell_key(idx)
        order = np.argsort(keys, kind="stable")
        ks, first = np.unique(keys[order], return_index=True)
        groups = {int(k): g for k, g in zip(ks, np.split(order, first[1:]))}
        self.history.append((pts, groups))
        if self._grid is not None:
            assert self._grid.insert_scan(pts) == 0
        return 0

    def _live_keys(self):
        keys = set()
        for _, groups in self.history:
            keys.update(groups)
        return sorted(keys)

    def _replayed(self):
        if self._grid is None:
            g = self.o.HybridGrid(self.resolution, self.leaf)
            for pts, groups in self.history:
                if groups:
                    live = np.sort(np.concatenate(list(groups.values())))       # the surviving points in scan order
                    assert g.insert_scan(pts[live]) == 0
            self._grid = g
        return self._grid

    def _cell_points(self, key):
        """One cell's slab: a fresh grid fed that cell's points only."""
        g = self.o.HybridGrid(self.resolution, self.leaf)
        for pts, groups in self.history:
            if key in groups:
                assert g.insert_scan(pts[groups[key]]) == 0
        assert g.size()[1] == 1
        return g.dump()

    # ---- the store's interface ----
    def size(self):
        return self._replayed().size()

    def dump(self):
        return self._replayed().dump()

    def get_surrounded(self, scan, pose):
        return self._replayed().get_surrounded(scan, pose)

    def dump_cells(self):
        keys = self._live_keys()
        if not keys:
            return np.zeros((0, 4), np.int32)
        counts = [len(self._cell_points(k)) for k in keys]
        return np.concatenate([key_cell(np.array(keys)), np.array(counts)[:, None]], axis=1).astype(np.int32)

    def crop(self, center, half_cells, keep_evicted=False, counts=True):
        """Returns the CropInfo, or (info, evicted cells (m, 4), evicted points) taken from the state before.  counts=False: only
        forget (no replay; returns None), for long runs that compare the map at the end."""
        c = cell_index(np.asarray(center, np.float64).astype(np.float32), self.resolution)
        half = np.asarray(half_cells, np.int64)
        assert (half >= 0).all()
        keys = self._live_keys()
        out = [k for k in keys if (np.abs(key_cell(k) - c) > half).any()]
        ev = [self._cell_points(k) for k in out] if counts else []
        n_before = self.size() if counts else None
        if out:
            gone = set(out)
            for _, groups in self.history:
                for k in gone.intersection(groups):
                    del groups[k]
            self.history = [h for h in self.history if h[1]]
            self._grid = None
        if not counts:
            return None
        n_ev = int(sum(len(e) for e in ev))
        info = CropInfo(len(out), n_ev, n_before[1] - len(out), n_before[0] - n_ev, c)
        if not keep_evicted:
            return info
        cells = (np.concatenate([key_cell(np.array(out)), np.array([len(e) for e in ev])[:, None]], axis=1).astype(np.int32)
                 if out else np.zeros((0, 4), np.int32))
        return info, cells, (np.concatenate(ev) if ev else np.zeros((0, 4), np.float32))
