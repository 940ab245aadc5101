"""CPU: the model of msfl_grid_render / msfl_scan_novelty (tests/novelty_numpy.py) against hand cases, the configuration through the
library's host-only functions, and the preconditions of the dense-wall scene that tests/test_gpu_novelty.py runs on the device
(docs/kernels/novelty.md)."""
import ctypes

import numpy as np
import pytest

from tests import carve_numpy as cn
from tests import novelty_cases as nc
from tests import novelty_numpy as nn

F = np.float32
IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1.0])


def _capi():
    from tests.test_capi_symbols import _lib
    return _lib()


def _ray(col, row, r, n_col=36, n_row=4):
    az, el = np.deg2rad((col + 0.5) * 360.0 / n_col), np.deg2rad(-16.0 + (row + 0.5) * 32.0 / n_row)
    return [r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), 0.5]


def _setup(**kw):
    capi = _capi()
    cfg = capi.novelty_config(n_col=36, n_row=4, **kw)
    return cfg, capi.carve_tables(cfg.image), np.full((4, 36), np.inf, F)


def test_one_point_per_class_and_the_strict_test():
    cfg, tables, img = _setup(window_col=0, window_row=0, margin_rel=0.0, margin_abs=0.5)
    img[1, 3], img[1, 5] = 10.0, 2.0
    # (3, 4, 0): r = 5 exactly, elevation 0 (row 2), azimuth 53.13 degrees (column 5)
    scan = np.array([[0, 0, 5, 0], [np.nan, 1, 1, 0], _ray(7, 1, 5.0), _ray(3, 1, 5.0), _ray(5, 1, 5.0), [3, 4, 0, 0]], F)
    has, r, row, col = cn.pixels(scan[:, :3], cfg.image, tables)
    assert has.tolist() == [False, False, True, True, True, True] and (row[5], col[5], r[5]) == (2, 5, F(5.0))
    assert nn.classify(scan, img, cfg, tables).tolist() == [nn.NONE, nn.NONE, nn.UNSEEN, nn.IN_FRONT, nn.COVERED, nn.UNSEEN]
    img[2, 5] = 5.5                                              # r_hi = 5 * 1 + 0.5 == mlim: the test is strict
    assert nn.classify(scan, img, cfg, tables)[5] == nn.COVERED
    img[2, 5] = np.nextafter(F(5.5), F(np.inf))
    assert nn.classify(scan, img, cfg, tables)[5] == nn.IN_FRONT
    # the mask and the counts
    cls = nn.classify(scan, img, cfg, tables)
    masked = nn.mask(scan, cls, (1 << nn.NONE) | (1 << nn.COVERED))
    kept = np.isin(cls, (nn.NONE, nn.COVERED))
    assert masked[kept].tobytes() == scan[kept].tobytes() and np.array_equal(masked[:, 3], scan[:, 3])
    assert (masked[~kept, :3].view(np.uint32) == 0x7FC00000).all()
    assert nn.info(cls, img, 0b0101) == ((2, 1, 1, 2), 3, 3, 1)


def test_support_one_short_and_just_enough():
    cfg, tables, img = _setup(window_col=1, window_row=0)
    img[1, 9], img[1, 11] = 20.0, 30.0                           # two of the three window positions of column 10
    scan = np.array([_ray(10, 1, 5.0)], F)
    mlim, support = nn.window(img, cfg)
    assert support[1, 10] == 2 and mlim[1, 10] == F(20.0) and support[1, 9] == 1 and support[1, 12] == 1 and support[1, 13] == 0
    for min_support, want in ((3, nn.UNSEEN), (2, nn.IN_FRONT), (1, nn.IN_FRONT)):
        cfg.min_support = min_support
        assert nn.classify(scan, img, cfg, tables)[0] == want


def test_the_window_wraps_across_the_column_seam():
    cfg, tables, img = _setup(window_col=2, window_row=0)
    img[2, 34], img[2, 1] = 20.0, 30.0
    scan = np.array([_ray(0, 2, 5.0), _ray(35, 2, 5.0), _ray(32, 2, 5.0), _ray(31, 2, 5.0), _ray(3, 2, 25.0), _ray(4, 2, 5.0)], F)
    mlim, support = nn.window(img, cfg)
    assert (support[2, 0], mlim[2, 0]) == (2, F(20.0)) and (support[2, 35], mlim[2, 35]) == (2, F(20.0))
    assert nn.classify(scan, img, cfg, tables).tolist() == [nn.IN_FRONT, nn.IN_FRONT, nn.IN_FRONT, nn.UNSEEN, nn.IN_FRONT, nn.UNSEEN]
    cfg.image.window_col = 1
    assert nn.classify(scan, img, cfg, tables).tolist() == [nn.IN_FRONT, nn.IN_FRONT, nn.UNSEEN, nn.UNSEEN, nn.UNSEEN, nn.UNSEEN]
    cfg.image.window_col = 0
    assert (nn.classify(scan, img, cfg, tables) == nn.UNSEEN).all()


def test_clamped_rows_count_the_edge_row_again():
    cfg, tables, img = _setup(window_col=0, window_row=1, min_support=2)
    img[0, 4], img[1, 6], img[3, 8], img[2, 10] = 20.0, 20.0, 20.0, 20.0
    scan = np.array([_ray(4, 0, 5.0), _ray(6, 0, 5.0), _ray(8, 3, 5.0), _ray(10, 3, 5.0)], F)
    _, support = nn.window(img, cfg)
    assert (support[0, 4], support[0, 6], support[3, 8], support[3, 10]) == (2, 1, 2, 1)
    assert nn.classify(scan, img, cfg, tables).tolist() == [nn.IN_FRONT, nn.UNSEEN, nn.IN_FRONT, nn.UNSEEN]
    # an empty centre pixel does not void the window
    cfg.min_support = 1
    assert nn.classify(scan, img, cfg, tables).tolist() == [nn.IN_FRONT] * 4


def test_accumulate_is_commutative_over_two_stores(oracle):
    capi = _capi()
    cfg = capi.novelty_config()
    tables = capi.carve_tables(cfg.image)
    rng = np.random.default_rng(11)
    a, b = cn.CarveGrid(oracle, 3.0, 0.2), cn.CarveGrid(oracle, 3.0, 0.4)
    for g in (a, b):
        pts = np.zeros((400, 4), F)
        pts[:, :3] = rng.uniform(-12.0, 12.0, (400, 3)) * [1, 1, 0.15]
        assert g.insert_scan(pts) == 0
    ia, ta = nn.render(a, nc.POSE, cfg, tables)
    ib, tb = nn.render(b, nc.POSE, cfg, tables)
    ab, _ = nn.render(b, nc.POSE, cfg, tables, image=ia)
    ba, _ = nn.render(a, nc.POSE, cfg, tables, image=ib)
    assert ta > 100 and tb > 100 and np.isfinite(ia).sum() > 50 and (ia != ib).any()
    assert ab.tobytes() == ba.tobytes() == np.minimum(ia, ib).tobytes()
    empty, t0 = nn.render(cn.CarveGrid(oracle, 3.0, 0.2), nc.POSE, cfg, tables)
    assert t0 == 0 and np.isinf(empty).all() and empty.shape == (16, 720)


def test_the_defaults_and_the_limits_of_the_image():
    capi = _capi()
    cfg, carve = capi.novelty_config(), capi.carve_config()
    assert ctypes.sizeof(capi.NoveltyConfig) == 48 and ctypes.sizeof(capi.NoveltyInfo) == 32 and ctypes.sizeof(capi.GridRenderInfo) == 8
    assert (cfg.image.window_col, cfg.image.window_row, cfg.min_support, cfg.keep_classes) == (2, 1, 1, 0b0111)
    cfg.image.window_col, cfg.image.window_row = carve.window_col, carve.window_row
    assert bytes(cfg.image) == bytes(carve)                      # otherwise the carve's defaults
    assert (capi.NOV_NONE, capi.NOV_UNSEEN, capi.NOV_COVERED, capi.NOV_IN_FRONT) == (0, 1, 2, 3) == (nn.NONE, nn.UNSEEN, nn.COVERED, nn.IN_FRONT)
    with pytest.raises(TypeError):
        capi.novelty_config(no_such_field=1)
    for kw in ({"n_col": 3}, {"n_row": 129}, {"window_col": 5}, {"max_range": 0.1}, {"elev_low_deg": float("nan")}):
        with pytest.raises(capi.MsflError):
            capi.carve_tables(capi.novelty_config(**kw).image)
    lib = capi.load()
    assert lib.msfl_scan_novelty(None, None, 0, None, None, None, None, None, capi.MEM_HOST) == capi.BAD_ARG
    assert lib.msfl_grid_render(None, None, None, None, 0, capi.MEM_HOST, None) == capi.BAD_ARG
    assert lib.msfl_grids_scan_novelty(None, 1, None, 0, None, None, None, None, None, None, capi.MEM_HOST) == capi.BAD_ARG
    lib.msfl_novelty_default_config(None)                        # a null pointer is ignored


@pytest.mark.parametrize("window_col", [2, 0])
def test_dense_wall_scene_preconditions(oracle, window_col):
    capi = _capi()
    cfg = nc.config(capi, window_col)
    tables = capi.carve_tables(cfg.image)
    stored = oracle.transform_cloud(nc.map_points_sensor(), nc.POSE)
    m, g = cn.CarveGrid(oracle, 3.0, nc.LEAF), oracle.HybridGrid(3.0, nc.LEAF)
    assert m.insert_scan(stored) == 0 and g.insert_scan(stored) == 0
    # the store holds exactly the inserted points
    assert g.size()[0] == len(stored) == 116 and m.size() == g.size() and m.dump().tobytes() == g.dump().tobytes()
    assert sorted(map(bytes, m.dump())) == sorted(map(bytes, stored))
    img, n_tested = nn.render(m, nc.POSE, cfg, tables)
    occupied = np.isfinite(img)
    assert n_tested == 116 and occupied[:, nc.wall_cols()].all() and not occupied[:, list(nc.BLOCK)].any()
    assert np.abs(img[occupied] - 10.0).max() < 1e-3
    _, support = nn.window(img, cfg)
    zero = sorted(set(np.nonzero(support == 0)[1].tolist()))
    assert zero == (list(nc.MIDDLE) if window_col == 2 else list(nc.BLOCK))
    a, b, c = nc.scan_parts()
    assert (nn.classify(a, img, cfg, tables) == nn.COVERED).all() and len(a) == 116
    assert (nn.classify(b, img, cfg, tables) == nn.IN_FRONT).all() and len(b) == 8
    assert (nn.classify(c, img, cfg, tables) == nn.UNSEEN).all() and len(c) == 12
    assert np.array_equal(nn.classify(nc.scan(), img, cfg, tables), nc.expected())
