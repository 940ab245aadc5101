"""CPU model of the map store with msfl_grid_carve (docs/kernels/grid_store.md, "Carve").

A store that lost single centroids cannot be expressed as a replayed history of inserts (tests/windowed_grid_model.py), so this
model keeps an explicit point list per cell.  HybridGrid::InsertScan files every point under its 3 m cell and re-runs the voxel
filter over each TOUCHED cell's own cloud (hybrid_grid.cc:503-521), so an insert sets

    cell = oracle.voxel_grid(concat(stored points, the new points of that cell in arrival order), leaf)

which equals oracle.HybridGrid bit for bit (tests/test_carve_model.py pins it).  The surround query asks the oracle which cells a
scan marks through a probe grid that holds one point per live cell, at the cell's centre.

The carve itself follows the definition step by step in f32: the bisection tables come from the library (msfl_carve_tables), the
inverse pose and the transform from oracle.quat_rotate / oracle.transform_cloud."""
import numpy as np

from tests.windowed_grid_model import LIM, CropInfo, cell_index, cell_key, key_cell

F = np.float32


class CarveInfo:
    def __init__(self, n_points_removed, n_cells_emptied, n_cells, n_points, n_tested, n_pixels, applied=1):
        self.n_points_removed, self.n_cells_emptied, self.n_cells, self.n_points = n_points_removed, n_cells_emptied, n_cells, n_points
        self.n_tested, self.n_pixels, self.applied = n_tested, n_pixels, applied

    def as_tuple(self):
        return (self.n_points_removed, self.n_cells_emptied, self.n_cells, self.n_points, self.n_tested, self.n_pixels, self.applied)


def _bisect(pred, hi):
    """lo = 0, hi: while hi - lo > 1, mid = (lo + hi) >> 1 goes to lo where pred(mid) holds, else to hi.  Per element."""
    lo = np.zeros(len(hi), np.int64)
    hi = hi.copy()
    while True:
        act = hi - lo > 1
        if not act.any():
            return lo
        mid = (lo + hi) >> 1
        ok = pred(mid) & act
        lo = np.where(ok, mid, lo)
        hi = np.where(act & ~ok, mid, hi)


def pixels(xyz, cfg, tables):
    """(has pixel, r, row, col) of sensor-frame points (n, 3) f32, as the kernels decide it."""
    cc, cs, ec, es = tables
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    n_col, n_row, half = int(cfg.n_col), int(cfg.n_row), int(cfg.n_col) // 2
    with np.errstate(all="ignore"):
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        rho2 = x * x + y * y
        rho = np.sqrt(rho2)
        r = np.sqrt(rho2 + z * z)
        assert rho2.dtype == F and r.dtype == F
        has = finite & (rho2 != 0) & (r >= F(cfg.min_range)) & ~(r > F(cfg.max_range))
        f = lambda k: z * ec[k] - rho * es[k]
        has &= ~((f(0) < 0) | (f(n_row) >= 0))
        upper = (y > 0) | ((y == 0) & (x > 0))
        xp, yp = np.where(upper, x, -x), np.where(upper, y, -y)
        n = len(x)
        col = _bisect(lambda mid: cc[mid] * yp - cs[mid] * xp >= 0, np.full(n, half, np.int64)) + np.where(upper, 0, half)
        row = _bisect(lambda mid: z * ec[mid] - rho * es[mid] >= 0, np.full(n, n_row, np.int64))
    return has, r, row, col


def range_image(scan, cfg, tables):
    """near (n_row, n_col) f32: the minimum range per pixel, +inf where empty."""
    near = np.full(int(cfg.n_row) * int(cfg.n_col), np.inf, F)
    scan = np.asarray(scan, F).reshape(-1, 4)
    has, r, row, col = pixels(scan[:, :3], cfg, tables)
    np.minimum.at(near, (row * int(cfg.n_col) + col)[has], r[has])
    return near.reshape(int(cfg.n_row), int(cfg.n_col))


def limit_image(near, cfg):
    """lim: 0 where the centre pixel is empty, else the minimum of near over rows +-window_row (clamped) and columns +-window_col
    (wrapping)."""
    n_row = near.shape[0]
    m = near.copy()
    for dr in range(-int(cfg.window_row), int(cfg.window_row) + 1):
        rows = np.clip(np.arange(n_row) + dr, 0, n_row - 1)
        for dc in range(-int(cfg.window_col), int(cfg.window_col) + 1):
            m = np.minimum(m, np.roll(near[rows], -dc, axis=1))
    return np.where(np.isinf(near), F(0), m).astype(F)


def inverse_pose(oracle, pose):
    """conj(q) and -rotate(conj(q), t), in f64."""
    pose = np.asarray(pose, np.float64)
    qc = np.array([-pose[3], -pose[4], -pose[5], pose[6]])
    return np.concatenate([-oracle.quat_rotate(qc, pose[:3]), qc])


def sees_through(oracle, pts, pose, lim, cfg, tables):
    """(removed, tested) flags of stored points (n, 4) under the limit image `lim`."""
    pts = np.ascontiguousarray(np.asarray(pts, F).reshape(-1, 4))
    if len(pts) == 0:
        return np.zeros(0, bool), np.zeros(0, bool)
    local = oracle.transform_cloud(pts, inverse_pose(oracle, pose))
    has, r, row, col = pixels(local[:, :3], cfg, tables)
    with np.errstate(all="ignore"):
        reach = (r * (F(1) + F(cfg.margin_rel))) + F(cfg.margin_abs)
        assert reach.dtype == F
        gone = has & (reach < lim[np.where(has, row, 0), np.where(has, col, 0)])
    return gone, has


class CarveGrid:
    """insert_scan / carve / crop / crop_tiles / load_cells / dump / dump_cells / size / get_surrounded with the semantics of msfl_grid_*."""

    def __init__(self, oracle, resolution=3.0, leaf=0.2):
        self.o, self.resolution, self.leaf = oracle, float(resolution), float(leaf)
        self.cells = {}             # cell key -> (m, 4) f32, m > 0, stored order

    def insert_scan(self, pts):
        pts = np.ascontiguousarray(np.asarray(pts, F).reshape(-1, 4))
        if len(pts) == 0:
            return 0
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(pts[:, :3]).all()
            idx = cell_index(np.where(np.isfinite(pts[:, :3]), pts[:, :3], 0), self.resolution)
        if not ok or (idx < -LIM).any() or (idx >= LIM).any():
            return 7                                            # dropped as a whole
        keys = cell_key(idx)
        order = np.argsort(keys, kind="stable")
        ks, first = np.unique(keys[order], return_index=True)
        for k, g in zip(ks, np.split(order, first[1:])):
            old = self.cells.get(int(k), np.zeros((0, 4), F))
            self.cells[int(k)] = self.o.voxel_grid(np.concatenate([old, pts[g]]), self.leaf)
        return 0

    def _keys(self):
        return sorted(self.cells)

    def size(self):
        return int(sum(len(v) for v in self.cells.values())), len(self.cells)

    def dump(self):
        return np.concatenate([self.cells[k] for k in self._keys()]) if self.cells else np.zeros((0, 4), F)

    def dump_cells(self, keys=None):
        keys = self._keys() if keys is None else keys
        if not keys:
            return np.zeros((0, 4), np.int32)
        return np.concatenate([key_cell(np.array(keys)), np.array([len(self.cells[k]) for k in keys])[:, None]], axis=1).astype(np.int32)

    def get_surrounded(self, scan, pose):
        keys = self._keys()
        if not keys:
            return np.zeros((0, 4), F)
        probe = np.zeros((len(keys), 4), F)
        probe[:, :3] = key_cell(np.array(keys)) * self.resolution          # a cell's centre is filed under that cell
        probe[:, 3] = np.arange(len(keys))
        g = self.o.HybridGrid(self.resolution, 1.0)
        assert g.insert_scan(probe) == 0 and g.size() == (len(keys), len(keys))
        hit = g.get_surrounded(scan, pose)[:, 3].astype(np.int64)
        assert (np.diff(hit) > 0).all()
        return np.concatenate([self.cells[keys[i]] for i in hit]) if len(hit) else np.zeros((0, 4), F)

    def crop(self, center, half_cells, keep_evicted=False):
        """The CropInfo, or (info, evicted cells (m, 4), evicted points) taken from the state before."""
        c = cell_index(np.asarray(center, np.float64).astype(F), self.resolution)
        half = np.asarray(half_cells, np.int64)
        out = [k for k in self._keys() if (np.abs(key_cell(k) - c) > half).any()]
        cells = self.dump_cells(out)
        ev = [self.cells.pop(k) for k in out]
        n_ev = int(sum(len(e) for e in ev))
        info = CropInfo(len(out), n_ev, len(self.cells), self.size()[0], c)
        if not keep_evicted:
            return info
        return info, cells, (np.concatenate(ev) if ev else np.zeros((0, 4), F))

    def load_cells(self, cells, pts):
        cells, pts = np.asarray(cells, np.int64).reshape(-1, 4), np.asarray(pts, F).reshape(-1, 4)
        start = np.concatenate([[0], np.cumsum(cells[:, 3])])
        assert start[-1] == len(pts)
        for j, k in enumerate(cell_key(cells[:, :3])):
            assert int(k) not in self.cells and cells[j, 3] > 0
            self.cells[int(k)] = pts[start[j]:start[j + 1]].copy()

    def carve(self, scan, pose, cfg, tables, keep_removed=False, capacity=None):
        """(CarveInfo, removed points in dump order or None).  More removed points than `capacity` (with keep_removed): refused, the
        store unchanged, applied = 0, the counts filled."""
        near = range_image(scan, cfg, tables)
        lim = limit_image(near, cfg)
        n_pixels = int(np.isfinite(near).sum())
        plan, n_tested = {}, 0
        for k in self._keys():
            gone, tested = sees_through(self.o, self.cells[k], pose, lim, cfg, tables)
            n_tested += int(tested.sum())
            if gone.any():
                plan[k] = gone
        n_gone = int(sum(g.sum() for g in plan.values()))
        n_emptied = int(sum(g.all() for g in plan.values()))
        n_pts, n_cells = self.size()
        if keep_removed and capacity is not None and n_gone > capacity:
            return CarveInfo(n_gone, n_emptied, n_cells, n_pts, n_tested, n_pixels, 0), np.zeros((0, 4), F)
        removed = [self.cells[k][plan[k]] for k in sorted(plan)]
        for k, gone in plan.items():
            if gone.all():
                del self.cells[k]
            else:
                self.cells[k] = self.cells[k][~gone]
        info = CarveInfo(n_gone, n_emptied, n_cells - n_emptied, n_pts - n_gone, n_tested, n_pixels, 1)
        return info, ((np.concatenate(removed) if removed else np.zeros((0, 4), F)) if keep_removed else None)
