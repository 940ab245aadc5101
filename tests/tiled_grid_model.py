"""CPU model of the map store with tiles: tests/windowed_grid_model.py plus a way back.

A crop PARKS the per-cell history it removes instead of deleting it; load_cells(keys) puts it back under the inserts it came
from, in their original order.  Cells evolve independently (hybrid_grid.cc:503-521 re-runs the filter over each touched
cell's own cloud), so the claim the store is held to is: after any crop and reload the store equals a fresh
oracle.HybridGrid fed the history minus the cells still parked.  A loaded cell is one that never left.

A cell evicted a second time parks what it held then; the tile of the first eviction is gone, as it is for a caller who
overwrites the buffer of the first crop."""
import numpy as np

from tests import windowed_grid_model as wm


class TiledGrid(wm.WindowedGrid):
    def __init__(self, oracle, resolution=3.0, leaf=0.2):
        super().__init__(oracle, resolution, leaf)
        self._entries = []          # every insert ever: (points, groups) -- the same dicts the history holds
        self.parked = {}            # cell key -> [(insert ordinal, indices of the cell's points in that insert)]

    def insert_scan(self, pts):
        n = len(self.history)
        rc = super().insert_scan(pts)
        if len(self.history) > n:
            self._entries.append(self.history[-1])
        return rc

    def crop(self, center, half_cells, keep_evicted=False, counts=True):
        c = wm.cell_index(np.asarray(center, np.float64).astype(np.float32), self.resolution)
        half = np.asarray(half_cells, np.int64)
        for k in self._live_keys():
            if (np.abs(wm.key_cell(k) - c) > half).any():
                self.parked[k] = [(n, groups[k]) for n, (_, groups) in enumerate(self._entries) if k in groups]
        return super().crop(center, half_cells, keep_evicted=keep_evicted, counts=counts)

    def load_cells(self, keys):
        """Parked cells back, by key (wm.cell_key of {ix, iy, iz}).  A key that is live or was never parked is an error."""
        live = set(self._live_keys())
        for k in (int(k) for k in keys):
            assert k in self.parked and k not in live, k
            for n, idx in self.parked.pop(k):
                self._entries[n][1][k] = idx
        self.history = [e for e in self._entries if e[1]]
        self._grid = None
