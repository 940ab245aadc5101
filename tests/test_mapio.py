"""msf_loam_amd/mapio.py on the CPU: the file round trip, and a refusal for each rule msfl_grid_load_cells applies."""
import numpy as np
import pytest

from msf_loam_amd import mapio

CELLS = np.array([[5, 5, -1, 1], [-3, 0, 0, 2], [1, 0, 0, 1], [0, 1, 0, 1]], np.int32)
POINTS = np.array([[15.0, 15.1, -3.2, 0.1], [-9.1, 0.1, 0.0, 0.2], [-8.9, -0.4, 0.3, 0.3], [4.5, 0.2, 0.1, 0.4], [0.2, 3.1, 0.0, 0.7]], np.float32)


def test_round_trip_is_bit_exact(tmp_path):
    p = str(tmp_path / "corner.npz")
    pts = POINTS.copy()
    pts[0, 0] = np.nextafter(np.float32(15.0), np.float32(16.0))           # not a short decimal
    pts[1, 3] = np.float32(np.nan)                                         # the intensity is carried, not judged
    mapio.write_map(p, 3.0, 0.2, CELLS, pts)
    r, l, cells, points = mapio.read_map(p)
    assert (r, l) == (3.0, float(np.float32(0.2)))
    assert cells.dtype == np.int32 and points.dtype == np.float32
    assert cells.tobytes() == CELLS.tobytes() and points.tobytes() == pts.tobytes()
    mapio.write_map(p, 3.0, 0.4, CELLS[:0], POINTS[:0])                    # an empty store is a map too
    r, l, cells, points = mapio.read_map(p)
    assert cells.shape == (0, 4) and points.shape == (0, 4)


def test_keys_sort_like_the_store():
    assert (np.diff(mapio.cell_keys(CELLS)) > 0).all()
    assert list(np.argsort(mapio.cell_keys(np.array([[1, 0, 0, 1], [0, 1, 0, 1], [0, 0, 1, 1], [0, 0, 0, 1]])))) == [3, 0, 1, 2]
    assert mapio.cell_keys(np.array([[-8192, -8192, -8192, 1]]))[0] == 0 and mapio.cell_keys(np.array([[8191, 8191, 8191, 1]]))[0] == (1 << 42) - 1


def _bad(**kw):
    cells, pts = CELLS.copy(), POINTS.copy()
    if "cell" in kw:
        cells[kw["cell"][0]] = kw["cell"][1]
    if "point" in kw:
        pts[kw["point"][0], kw["point"][1]] = kw["point"][2]
    if kw.get("drop_point"):
        pts = pts[:-1]
    return cells, pts


RULES = {
    "zero count": (_bad(cell=(2, [1, 0, 0, 0])), "count <= 0"),
    "negative count": (_bad(cell=(2, [1, 0, 0, -1])), "count <= 0"),
    "index 8192": (_bad(cell=(3, [8192, 1, 0, 1])), "outside"),
    "index -8193": (_bad(cell=(0, [5, 5, -8193, 1])), "outside"),
    "descending": (_bad(cell=(2, [-4, 0, 0, 1])), "ascending"),
    "duplicate": (_bad(cell=(2, [-3, 0, 0, 1])), "ascending"),
    "wrong sum": (_bad(drop_point=True), "sum"),
    "nan": (_bad(point=(3, 2, np.nan)), "finite"),
    "inf": (_bad(point=(0, 0, -np.inf)), "finite"),
    "cells shape": ((CELLS[:, :3], POINTS), "cells"),
    "cells dtype": ((CELLS.astype(np.float32), POINTS), "cells"),
    "points shape": ((CELLS, POINTS[:, :3]), "points"),
    "points dtype": ((CELLS, POINTS.astype(np.float64)), "points"),
}


@pytest.mark.parametrize("rule", sorted(RULES))
def test_each_rule_refuses_on_write_and_on_read(tmp_path, rule):
    (cells, pts), word = RULES[rule]
    p = str(tmp_path / "m.npz")
    with pytest.raises(mapio.MapFileError, match=word):
        mapio.write_map(p, 3.0, 0.4, cells, pts)
    # a file written by other means is refused when read
    with open(p, "wb") as f:
        np.savez(f, format=np.int32(mapio.FORMAT), resolution=np.float32(3.0), leaf=np.float32(0.4), cells=cells, points=pts)
    with pytest.raises(mapio.MapFileError, match=word):
        mapio.read_map(p)


def test_other_files_are_refused(tmp_path):
    p = str(tmp_path / "m.npz")
    with open(p, "wb") as f:
        np.savez(f, cells=CELLS, points=POINTS)
    with pytest.raises(mapio.MapFileError, match="not a map file"):
        mapio.read_map(p)
    with open(p, "wb") as f:
        np.savez(f, format=np.int32(99), resolution=np.float32(3.0), leaf=np.float32(0.4), cells=CELLS, points=POINTS)
    with pytest.raises(mapio.MapFileError, match="format"):
        mapio.read_map(p)
    with pytest.raises(mapio.MapFileError, match="positive"):
        mapio.write_map(p, 3.0, 0.0, CELLS, POINTS)


class _FakeGrid:
    """dump_cells / dump / load_cells of capi.Grid, on the host"""

    def __init__(self, cells=CELLS[:0], points=POINTS[:0], resolution=3.0, leaf=0.4):
        self.cells, self.points, self.resolution, self.leaf = cells, points, resolution, leaf

    def dump_cells(self):
        return self.cells

    def dump(self):
        return self.points

    def load_cells(self, cells, points):
        self.cells, self.points = cells, points
        return len(cells), len(points)


def test_save_grid_and_load_grid(tmp_path):
    p = str(tmp_path / "surf.npz")
    assert mapio.save_grid(p, _FakeGrid(CELLS, POINTS)) == (4, 5)
    g = _FakeGrid()
    assert mapio.load_grid(p, g) == (4, 5)
    assert g.cells.tobytes() == CELLS.tobytes() and g.points.tobytes() == POINTS.tobytes()
    with pytest.raises(mapio.MapFileError, match="leaf"):
        mapio.load_grid(p, _FakeGrid(leaf=0.2))
    with pytest.raises(mapio.MapFileError, match="resolution"):
        mapio.load_grid(p, _FakeGrid(resolution=2.0))
