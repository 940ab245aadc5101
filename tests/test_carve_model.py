"""CPU: the model of the map store with msfl_grid_carve (tests/carve_numpy.py) -- its per-cell form against oracle.HybridGrid, the
hand cases of the definition (docs/kernels/grid_store.md, "Carve"), and the library's bisection tables against numpy."""
import numpy as np
import pytest

from tests import carve_cases as cc
from tests import carve_numpy as cn
from tests.test_grid_store import _batches


@pytest.mark.parametrize("leaf,n_points", [(0.2, 24683), (0.4, 16677)])
def test_per_cell_store_equals_the_oracle_grid(oracle, leaf, n_points):
    """Four inserts: sizes, dump and two surround queries equal oracle.HybridGrid's bit for bit after each."""
    bs = _batches()
    m, g = cn.CarveGrid(oracle, 3.0, leaf), oracle.HybridGrid(3.0, leaf)
    for scan, wp, pose in bs:
        assert m.insert_scan(wp) == 0 and g.insert_scan(wp) == 0
        assert m.size() == g.size()
        assert np.array_equal(m.dump(), g.dump())
        for sc, ps in ((scan, pose), (bs[0][0], bs[0][2])):
            assert np.array_equal(m.get_surrounded(sc, ps), g.get_surrounded(sc, ps))
    assert m.size()[0] == n_points
    assert m.dump_cells()[:, 3].sum() == n_points and len(m.dump_cells()) == g.size()[1]
    assert m.insert_scan(np.array([[3e4, 0, 0, 0]], np.float32)) == 7 and m.size() == g.size()


def _config(**kw):
    from msf_loam_amd import capi
    return capi.carve_config(**kw), capi


def _hand_store(oracle, leaf):
    m = cn.CarveGrid(oracle, 3.0, leaf)
    stored = oracle.transform_cloud(cc.hand_points(), cc.HAND_POSE)
    assert m.insert_scan(stored) == 0
    assert m.size()[0] == len(stored)                           # no voxel merged two of the labelled points
    return m


@pytest.mark.parametrize("leaf", [0.2, 0.4])
@pytest.mark.parametrize("window_col,window_row", [(1, 1), (0, 1), (1, 0)])
def test_hand_cases(oracle, leaf, window_col, window_row):
    """The blob in front of the wall, the point short of the margin and the near point go; the wall, what lies behind it, points
    in an empty pixel, outside the field of view, below min_range, beyond max_range and inside the margin stay.  The point beside
    the pole goes only with window_col = 0, the far ground between two beams only with window_row = 0."""
    cfg, capi = _config(window_col=window_col, window_row=window_row)
    tables = capi.carve_tables(cfg)
    m = _hand_store(oracle, leaf)
    before = cc.classes(m.dump())
    n_before = m.size()[0]
    info, removed = m.carve(cc.hand_scan(), cc.HAND_POSE, cfg, tables, keep_removed=True)
    assert cc.classes(m.dump()) == cc.hand_expected(window_col, window_row)
    gone = cc.classes(removed)
    assert gone[cc.BLOB] == 9 and gone[cc.NEAR_GONE] == 1 and gone[cc.MARGIN_GONE] == 1
    assert (cc.BESIDE_POLE in gone) == (window_col == 0) and (cc.FAR_GROUND in gone) == (window_row == 0)
    assert {k: gone.get(k, 0) + cc.classes(m.dump()).get(k, 0) for k in before} == before
    assert info.applied == 1 and info.n_points_removed == len(removed) == n_before - m.size()[0] and (info.n_points, info.n_cells) == m.size()
    # tested: everything but the two points outside the field of view, the one below min_range and the one beyond max_range
    assert info.n_tested == n_before - 4
    assert info.n_pixels == 160 * 16 + 40 * 16 + 80 * 8
    assert info.n_cells_emptied > 0 and m.dump_cells()[:, 3].min() > 0 and m.dump_cells()[:, 3].sum() == m.size()[0]


def test_pixels_of_the_hand_scan(oracle):
    """Every ray of the hand scan lands in the pixel it was built for; y == 0 on both signs of x, a point on the axis, a NaN."""
    cfg, capi = _config()
    tables = capi.carve_tables(cfg)
    near = cn.range_image(cc.hand_scan(), cfg, tables)
    cols = np.flatnonzero(np.isfinite(near).any(axis=0))
    assert np.array_equal(cols, np.r_[0:80, 200:280, 580:620, 640:720])
    assert np.isfinite(near[:, 0:80]).all() and np.isfinite(near[:8, 200:280]).all() and np.isinf(near[8:, 200:280]).all()
    assert abs(near[8, 0] - 10.0 / (np.cos(np.deg2rad(0.25)) * np.cos(np.deg2rad(1.0)))) < 1e-5 and near[3, 600] == np.float32(3.0)
    pts = np.array([[2, 0, 0.01], [-2, 0, 0.01], [0, 2, 0.01], [0, -2, 0.01], [0, 0, 1], [np.nan, 1, 0], [2, 0, -0.01]], np.float32)
    has, r, row, col = cn.pixels(pts, cfg, tables)
    assert has.tolist() == [True, True, True, True, False, False, True]
    assert col[[0, 1, 2, 3, 6]].tolist() == [0, 360, 180, 540, 0] and row[[0, 6]].tolist() == [8, 7]


def test_limit_image_wraps_columns_and_clamps_rows():
    from msf_loam_amd import capi
    cfg = capi.carve_config(n_col=8, n_row=3, window_col=2, window_row=1)
    near = np.full((3, 8), np.inf, np.float32)
    near[0, 7], near[2, 1], near[1, 4] = 5.0, 7.0, 9.0
    lim = cn.limit_image(near, cfg)
    want = np.zeros((3, 8), np.float32)
    want[0, 7], want[2, 1], want[1, 4] = 5.0, 7.0, 9.0           # each alone in its window ...
    assert np.array_equal(lim, want)
    near[1, 0] = 6.0                                             # ... until (1, 0) joins: two columns from 7 across the seam, one row from both
    lim = cn.limit_image(near, cfg)
    want[1, 0], want[2, 1] = 5.0, 6.0
    assert np.array_equal(lim, want)


def test_refusal_leaves_the_model_unchanged(oracle):
    cfg, capi = _config()
    tables = capi.carve_tables(cfg)
    m = _hand_store(oracle, 0.2)
    before, cells = m.dump(), m.dump_cells()
    info, removed = m.carve(cc.hand_scan(), cc.HAND_POSE, cfg, tables, keep_removed=True, capacity=10)
    assert info.applied == 0 and info.n_points_removed == 11 and len(removed) == 0 and (info.n_points, info.n_cells) == m.size()
    assert np.array_equal(m.dump(), before) and np.array_equal(m.dump_cells(), cells)
    info2, removed = m.carve(cc.hand_scan(), cc.HAND_POSE, cfg, tables, keep_removed=True, capacity=11)
    assert info2.applied == 1 and len(removed) == 11 and info2.as_tuple()[4:6] == info.as_tuple()[4:6]


@pytest.mark.parametrize("kw", [{}, {"n_col": 2, "n_row": 1}, {"n_col": 2048, "n_row": 128, "elev_low_deg": -89.5, "elev_high_deg": 89.5},
                                {"n_col": 600, "n_row": 7, "elev_low_deg": -24.8, "elev_high_deg": 2.0}])
def test_tables_against_numpy(kw):
    """cc, cs = cos, sin(2 pi k / n_col); ec, es = cos, sin of the row boundaries: within 1 ulp of f32 of numpy's f64 values."""
    from msf_loam_amd import capi
    cfg = capi.carve_config(**kw)
    cc_, cs_, ec_, es_ = capi.carve_tables(cfg)
    a = 2.0 * np.pi * np.arange(cfg.n_col // 2) / cfg.n_col
    e = np.deg2rad(np.float64(cfg.elev_low_deg) + (np.float64(cfg.elev_high_deg) - np.float64(cfg.elev_low_deg)) * np.arange(cfg.n_row + 1) / cfg.n_row)
    for got, want in ((cc_, np.cos(a)), (cs_, np.sin(a)), (ec_, np.cos(e)), (es_, np.sin(e))):
        assert got.dtype == np.float32 and len(got) == len(want)
        w32 = want.astype(np.float32)
        assert (np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(w32)).astype(np.float64)).all()
    assert cc_[0] == 1.0 and cs_[0] == 0.0


def test_config_limits():
    from msf_loam_amd import capi
    for kw in ({"n_col": 3}, {"n_col": 0}, {"n_col": 2050}, {"n_row": 0}, {"n_row": 129}, {"elev_low_deg": 20.0}, {"elev_high_deg": 90.0},
               {"elev_low_deg": -90.0}, {"min_range": -0.1}, {"max_range": 0.2}, {"margin_abs": -1.0}, {"margin_rel": -0.5}, {"window_col": 5},
               {"window_row": -1}, {"max_range": float("inf")}, {"margin_abs": float("nan")}):
        with pytest.raises(capi.MsflError) as e:
            capi.carve_tables(capi.carve_config(**kw))
        assert e.value.status == capi.BAD_ARG, kw
