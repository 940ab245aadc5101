"""msfl_grid_render, msfl_scan_novelty and msfl_grids_scan_novelty against the model of tests/novelty_numpy.py, byte for byte: images,
classes, masked clouds and the info records (docs/kernels/novelty.md)."""
import ctypes
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import carve_numpy as cn
from tests import novelty_cases as nc
from tests import novelty_numpy as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

F = np.float32
IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1.0])


def _pose(seed, at=(0.0, 0.0, 0.0), scale=1.0):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4) * [0.15, 0.15, 1.0, 1.0]             # mostly yaw, some tilt
    q /= np.linalg.norm(q)
    return np.concatenate([np.asarray(at, np.float64) + rng.uniform(-2.0, 2.0, 3) * [1, 1, 0.3], q * scale])


def _cloud(seed, n=4000, at=(0.0, 0.0, 0.0), half=(7.4, 7.4, 1.4)):
    """n points in a slab of 5 x 5 cells of 3 m round `at`."""
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 4), F)
    p[:, :3] = np.asarray(at, np.float64) + rng.uniform(-1.0, 1.0, (n, 3)) * half
    p[:, 3] = np.arange(n) / 1000.0
    return p


def _stores(gpu, oracle, pts, leaf):
    from msf_loam_amd import capi
    gg, m = capi.Grid(gpu, 3.0, leaf), cn.CarveGrid(oracle, 3.0, leaf)
    gg.insert_scan(pts)
    assert m.insert_scan(pts) == 0 and gg.size() == m.size()
    return gg, m


def _render_both(gg, m, pose, cfg, what, image=None):
    """Host-memory render on the store and on the model; returns the image."""
    from msf_loam_amd import capi
    want, n_tested = nn.render(m, pose, cfg, capi.carve_tables(cfg), image=image)
    got, info = gg.render(pose, cfg, image=image, accumulate=image is not None)
    print(what, "render", info.n_tested, n_tested, int(np.isfinite(want).sum()))
    assert info.status == capi.OK and (info.n_tested, info.applied) == (n_tested, 1), (what, info.n_tested, n_tested)
    assert got.tobytes() == want.tobytes(), what
    return got


def _render_device(gg, pose, cfg, image=None):
    import torch
    d_pose = torch.from_numpy(np.ascontiguousarray(pose, np.float64)).to("cuda:0")
    d_img = torch.from_numpy(np.ascontiguousarray(image, F)).to("cuda:0") if image is not None else torch.zeros((cfg.n_row, cfg.n_col), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    info = gg.render_device(d_pose, cfg, d_img, accumulate=image is not None, want_info=True)
    return d_img.cpu().numpy(), info


# ---- render -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("leaf", [0.2, 0.4])
@pytest.mark.parametrize("seed", [3, 4, 5])
def test_render_random_store(gpu, oracle, seed, leaf):
    """A few thousand points in 25 cells, a pose with rotation; host and device memory."""
    from msf_loam_amd import capi
    cfg = capi.carve_config()
    gg, m = _stores(gpu, oracle, _cloud(seed), leaf)
    assert 20 <= gg.size()[1] <= 30
    pose = _pose(seed)
    img = _render_both(gg, m, pose, cfg, (seed, leaf))
    assert 500 < np.isfinite(img).sum() < img.size
    dev, info = _render_device(gg, pose, cfg)
    assert dev.tobytes() == img.tobytes() and info.applied == 1 and info.n_tested > 500
    gg.close()


def test_render_far_from_the_origin_and_with_a_scaled_quaternion(gpu, oracle):
    """A pose at (5 000, -3 000, 20) m; a quaternion scaled by 1.1 is used as given and switches the cull off."""
    from msf_loam_amd import capi
    at = (5000.0, -3000.0, 20.0)
    cfg = capi.carve_config()
    gg, m = _stores(gpu, oracle, _cloud(7, at=at), 0.4)
    img = _render_both(gg, m, _pose(7, at), cfg, "far")
    assert np.isfinite(img).sum() > 500
    scaled = _render_both(gg, m, _pose(7, at, scale=1.1), cfg, "scaled")
    assert np.isfinite(scaled).sum() > 100 and scaled.tobytes() != img.tobytes()
    gg.close()


def test_render_empty_store_long_cell_and_cells_out_of_range(gpu, oracle):
    from msf_loam_amd import capi
    cfg = capi.carve_config()
    gg, m = _stores(gpu, oracle, np.zeros((0, 4), F), 0.2)
    img = _render_both(gg, m, IDENTITY, cfg, "empty")
    assert np.isinf(img).all() and img.view(np.uint32).max() == 0x7F800000
    gg.close()
    # one cell of more than 256 points: the slab loop runs twice and more
    gg, m = _stores(gpu, oracle, _cloud(8, n=1200, at=(6.0, 0.0, 0.0), half=(1.4, 1.4, 1.4)), 0.03)
    assert gg.size()[1] == 1 and gg.size()[0] > 1000
    _render_both(gg, m, _pose(8), cfg, "long cell")
    gg.close()
    # cells beyond max_range: a short range leaves most of the 25 near cells culled, two far clusters lie beyond the default range
    pts = np.concatenate([_cloud(9), _cloud(10, n=300, at=(150.0, 20.0, 0.0)), _cloud(11, n=300, at=(-96.0, 30.0, 3.0), half=(4.0, 4.0, 1.0))])
    gg, m = _stores(gpu, oracle, pts, 0.4)
    for max_range in (5.0, 100.0):
        c = capi.carve_config(max_range=max_range)
        img = _render_both(gg, m, _pose(9), c, ("max_range", max_range))
        assert 0 < np.isfinite(img).sum() and img[np.isfinite(img)].max() <= max_range
    gg.close()


@pytest.mark.parametrize("n_col,n_row", [(2, 1), (2048, 128)])
def test_render_smallest_and_largest_image(gpu, oracle, n_col, n_row):
    from msf_loam_amd import capi
    cfg = capi.carve_config(n_col=n_col, n_row=n_row)
    gg, m = _stores(gpu, oracle, _cloud(12), 0.2)
    pose = _pose(12)
    img = _render_both(gg, m, pose, cfg, (n_col, n_row))
    assert img.shape == (n_row, n_col) and np.isfinite(img).sum() == (2 if n_col == 2 else np.isfinite(img).sum()) > 0
    dev, _ = _render_device(gg, pose, cfg)
    assert dev.tobytes() == img.tobytes()
    gg.close()


def test_render_accumulates_in_either_order(gpu, oracle):
    """Two stores into one image in both orders, host and device memory: the element-wise minimum of the two separate renders."""
    from msf_loam_amd import capi
    cfg = capi.carve_config()
    a, ma = _stores(gpu, oracle, _cloud(13), 0.2)
    b, mb = _stores(gpu, oracle, _cloud(14, half=(7.4, 7.4, 0.5)), 0.4)
    pose = _pose(13)
    ia, ib = _render_both(a, ma, pose, cfg, "a"), _render_both(b, mb, pose, cfg, "b")
    want = np.minimum(ia, ib)
    assert (ia != ib).any() and (want != ia).any() and (want != ib).any()
    ab, ba = _render_both(b, mb, pose, cfg, "a then b", image=ia), _render_both(a, ma, pose, cfg, "b then a", image=ib)
    assert ab.tobytes() == ba.tobytes() == want.tobytes()
    d_ab, _ = _render_device(b, pose, cfg, image=ia)
    d_ba, _ = _render_device(a, pose, cfg, image=ib)
    assert d_ab.tobytes() == d_ba.tobytes() == want.tobytes()
    a.close(); b.close()


def test_render_only_reads_the_store(gpu, oracle):
    """Dump, cell list and a following carve are byte-equal with and without a render in between."""
    from msf_loam_amd import capi
    from tests.test_grid_store import _batches
    bs = _batches()
    cfg = capi.carve_config(margin_abs=0.0, margin_rel=0.0, window_col=0, window_row=0)
    a, b = capi.Grid(gpu, 3.0, 0.4), capi.Grid(gpu, 3.0, 0.4)
    for k in (0, 1):
        a.insert_scan(bs[k][1]); b.insert_scan(bs[k][1])
    img, info = a.render(bs[2][2], cfg)
    assert info.n_tested > 1000 and np.isfinite(img).sum() > 500
    _render_device(a, bs[2][2], cfg)
    assert a.size() == b.size() and a.dump().tobytes() == b.dump().tobytes() and a.dump_cells().tobytes() == b.dump_cells().tobytes()
    ia, ra = a.carve(bs[2][0], bs[2][2], cfg, keep_removed=True)
    ib, rb = b.carve(bs[2][0], bs[2][2], cfg, keep_removed=True)
    assert ia.as_tuple() == ib.as_tuple() and ia.n_points_removed > 0 and ra.tobytes() == rb.tobytes()
    a.render(bs[3][2], cfg)                                      # the carved table, the other parity
    assert a.dump().tobytes() == b.dump().tobytes() and a.dump_cells().tobytes() == b.dump_cells().tobytes()
    a.close(); b.close()


def test_render_refusals(gpu, oracle):
    import torch
    from msf_loam_amd import capi
    gg, m = _stores(gpu, oracle, _cloud(15, n=500), 0.4)
    cfg = capi.carve_config()
    img = np.full((16, 720), 7.0, F)
    pose = np.ascontiguousarray(IDENTITY)
    vp, lib = capi._vp, gg.lib
    info = capi.GridRenderInfo()
    assert lib.msfl_grid_render(gg.g, None, None, vp(img), 0, capi.MEM_HOST, None) == capi.BAD_ARG
    assert lib.msfl_grid_render(gg.g, vp(pose), None, None, 0, capi.MEM_HOST, None) == capi.BAD_ARG
    for kw in ({"n_col": 3}, {"n_row": 0}, {"elev_low_deg": 30.0}, {"max_range": 0.1}, {"window_col": 5}, {"min_range": float("nan")}):
        with pytest.raises(capi.MsflError) as e:
            gg.render(pose, capi.carve_config(**kw))
        assert e.value.status == capi.BAD_ARG and "msfl_grid_render" in str(e.value)
    bad = np.array([0, np.nan, 0, 0, 0, 0, 1.0])
    assert lib.msfl_grid_render(gg.g, vp(bad), None, vp(img), 0, capi.MEM_HOST, ctypes.byref(info)) == capi.BAD_ARG
    assert (img == 7.0).all()                                    # refused before anything was staged
    assert lib.msfl_grid_render(gg.g, vp(pose), None, vp(img), 0, capi.MEM_HOST, None) == capi.OK      # the defaults, no info
    assert img.tobytes() == nn.render(m, pose, cfg, capi.carve_tables(cfg))[0].tobytes()
    # a device-resident pose that is not finite: all +inf without accumulate, untouched with it, applied = 0, the status when info is read
    d_bad = torch.from_numpy(bad).to("cuda:0")
    d_img = torch.full((16, 720), 7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    r = gg.render_device(d_bad, cfg, d_img, accumulate=True, want_info=True, allow=(capi.BAD_ARG,))
    assert r.status == capi.BAD_ARG and (r.n_tested, r.applied) == (0, 0) and (d_img.cpu().numpy() == 7.0).all()
    r = gg.render_device(d_bad, cfg, d_img, want_info=True, allow=(capi.BAD_ARG,))
    assert r.status == capi.BAD_ARG and r.applied == 0 and np.isinf(d_img.cpu().numpy()).all()
    assert gg.render_device(d_bad, cfg, d_img) is None            # without info the call only enqueues
    gpu.synchronize()
    gg.close()


# ---- label --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _label_scene():
    """(map image (16, 720), scan of 5 000 points) for the default geometry: a synthetic map image with holes and a scan of random
    points with every special case in front."""
    rng = np.random.default_rng(21)
    img = rng.uniform(2.0, 30.0, (16, 720)).astype(F)
    img[rng.random((16, 720)) < 0.55] = np.inf                    # sparse, like a feature store
    img[:, 100:140] = np.inf
    img[0, :8], img[15, 712:] = 9.0, 9.0                          # the corners of the seam
    n = 5000
    scan = np.zeros((n, 4), F)
    az, el, r = rng.uniform(0, 2 * np.pi, n), np.deg2rad(rng.uniform(-19.0, 19.0, n)), rng.uniform(0.2, 40.0, n)
    scan[:, :3] = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], axis=1)
    scan[:, 3] = np.arange(n) / 1000.0
    special = [[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [0, 0, 5], [0, 0, -5], [0.3, 0, 0], [np.nextafter(F(0.3), F(0)), 0, 0], [100, 0, 0],
               [np.nextafter(F(100), F(200)), 0, 0], [5, 0, 5], [5, 0, -5], [-5, 0, 0.1], [0, 5, 0.1], [0, -5, 0.1], [5, 0, 0]]
    scan[:len(special), :3] = np.array(special, F)
    return img, scan


def _label_both(gpu, scan, img, cfg, what, device=False):
    from msf_loam_amd import capi
    tables = capi.carve_tables(cfg.image)
    cls = nn.classify(scan, img, cfg, tables)
    want_masked, want_info = nn.mask(scan, cls, cfg.keep_classes), nn.info(cls, img, cfg.keep_classes)
    if device:
        import torch
        n = len(scan)
        d_scan = torch.from_numpy(np.ascontiguousarray(scan)).to("cuda:0") if n else None
        d_img = torch.from_numpy(np.ascontiguousarray(img)).to("cuda:0")
        d_cls = torch.full((max(n, 1),), 9, dtype=torch.uint8, device="cuda:0")
        d_masked = torch.zeros((max(n, 1), 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        info = gpu.scan_novelty_device(d_scan, n, d_img, cfg, d_cls, d_masked, want_info=True)
        out = dict(cls=d_cls.cpu().numpy()[:n], masked=d_masked.cpu().numpy()[:n], info=info)
    else:
        out = gpu.scan_novelty(scan, img, cfg)
    print(what, "novelty", out["info"].as_tuple(), want_info)
    assert out["info"].status == capi.OK and out["info"].as_tuple() == want_info, (what, out["info"].as_tuple(), want_info)
    assert np.array_equal(out["cls"], cls), what
    assert out["masked"].tobytes() == want_masked.tobytes(), what
    return cls


@pytest.mark.parametrize("support", ["one", "max"])
@pytest.mark.parametrize("window_col,window_row", [(0, 0), (2, 1), (4, 4)])
def test_label_sizes_windows_and_support(gpu, window_col, window_row, support):
    from msf_loam_amd import capi
    img, scan = _label_scene()
    full = (2 * window_col + 1) * (2 * window_row + 1)
    cfg = capi.novelty_config(window_col=window_col, window_row=window_row, min_support=1 if support == "one" else full)
    for n in (0, 1, 63, 64, 65, 257, len(scan)):
        part = scan[len(scan) - n:] if n in (63, 257) else scan[:n]
        cls = _label_both(gpu, part, img, cfg, (window_col, window_row, support, n), device=n in (0, 65, len(scan)))
    counts = np.bincount(cls, minlength=4)
    assert counts[nn.NONE] > 100 and counts[nn.UNSEEN] > 100                 # the case is worth its time only if the classes occur
    assert counts[nn.IN_FRONT] > 100 or support == "max"
    assert counts[nn.COVERED] > 100 or (support == "max" and full > 1)
    assert cls[:9].tolist()[:5] == [nn.NONE] * 5 and cls[6] == nn.NONE and cls[8] == nn.NONE and cls[9] == nn.NONE and cls[10] == nn.NONE
    assert cls[5] != nn.NONE and cls[7] != nn.NONE                            # min_range and max_range exactly have a pixel


def test_label_every_keep_mask_and_the_fourth_field(gpu):
    from msf_loam_amd import capi
    img, scan = _label_scene()
    part = scan[:200].copy()
    part[:, 3] = np.arange(200) + 0.25
    seen = set()
    for keep in range(16):
        cls = _label_both(gpu, part, img, capi.novelty_config(keep_classes=keep), ("keep", keep), device=keep % 2 == 1)
        seen |= set(cls.tolist())
    assert seen == {nn.NONE, nn.UNSEEN, nn.COVERED, nn.IN_FRONT}


def test_label_refusals(gpu):
    from msf_loam_amd import capi
    img, scan = _label_scene()
    part = np.ascontiguousarray(scan[:100])
    n = len(part)
    cfg = capi.novelty_config()
    cls, masked, info = np.full(n, 9, np.uint8), np.zeros((n, 4), F), capi.NoveltyInfo()
    vp, lib = capi._vp, gpu.lib
    call = lambda **kw: lib.msfl_scan_novelty(gpu.h, vp(kw.get("scan", part)), kw.get("n", n), vp(kw.get("img", img)), ctypes.byref(kw.get("cfg", cfg)),
                                              vp(kw.get("cls", cls)), vp(kw.get("masked", masked)), ctypes.byref(info), capi.MEM_HOST)
    assert call(n=-1) == capi.BAD_ARG and call(scan=None) == capi.BAD_ARG and call(cls=None) == capi.BAD_ARG and call(img=None) == capi.BAD_ARG
    assert call(masked=part) == capi.BAD_ARG and "overlaps" in gpu.last_error()        # masked_out aliases the scan
    assert call(masked=part[n // 2:]) == capi.BAD_ARG                                # ... or overlaps it
    for kw in ({"min_support": 0}, {"min_support": 16}, {"keep_classes": -1}, {"keep_classes": 16}, {"n_col": 3}, {"window_row": 5},
               {"window_col": 0, "window_row": 0, "min_support": 2}):
        assert call(cfg=capi.novelty_config(**kw)) == capi.BAD_ARG, kw
    assert (cls == 9).all() and (masked == 0).all()                                  # nothing was written by a refused call
    assert call(cfg=capi.novelty_config(min_support=15)) == capi.OK
    # cfg = NULL: the defaults; masked_out = info = NULL; a scan that saw nothing
    assert lib.msfl_scan_novelty(gpu.h, vp(part), n, vp(img), None, vp(cls), None, None, capi.MEM_HOST) == capi.OK
    assert np.array_equal(cls, nn.classify(part, img, cfg, capi.carve_tables(cfg.image)))
    assert lib.msfl_scan_novelty(gpu.h, None, 0, vp(img), None, None, None, ctypes.byref(info), capi.MEM_HOST) == capi.OK
    assert info.as_tuple() == ((0, 0, 0, 0), int(np.isfinite(img).sum()), 0, 1)


@pytest.mark.parametrize("window_col", [2, 0])
def test_dense_wall_scene(gpu, oracle, window_col):
    """The scene whose preconditions tests/test_novelty_model.py checks: covered, in front and unseen, at both window widths."""
    from msf_loam_amd import capi
    cfg = nc.config(capi, window_col)
    stored = oracle.transform_cloud(nc.map_points_sensor(), nc.POSE)
    gg, m = _stores(gpu, oracle, stored, nc.LEAF)
    assert gg.size()[0] == 116
    img = _render_both(gg, m, nc.POSE, cfg.image, ("wall", window_col))
    cls = _label_both(gpu, nc.scan(), img, cfg, ("wall", window_col))
    assert np.array_equal(cls, nc.expected())
    out = capi.grids_scan_novelty([gg], nc.scan(), nc.POSE, cfg, want_image=True)
    assert np.array_equal(out["cls"], nc.expected()) and out["image"].tobytes() == img.tobytes()
    assert out["info"].as_tuple() == ((0, 12, 116, 8), 116, 128, 1)
    gg.close()


# ---- composite ----------------------------------------------------------------------------------------------------------------------

def _two_stores(gpu, oracle):
    a, ma = _stores(gpu, oracle, _cloud(31), 0.2)
    b, mb = _stores(gpu, oracle, _cloud(32, half=(7.4, 7.4, 0.5)), 0.4)
    return a, b


def _world_scan(seed, pose, n=3000):
    """Random points round the sensor, some of them non-finite, in the sensor frame."""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 4), F)
    s[:, :3] = rng.uniform(-1.0, 1.0, (n, 3)) * [9.0, 9.0, 1.5]
    s[:, 3] = np.arange(n) / 1000.0
    s[::97, 0] = np.nan
    return s


@pytest.mark.parametrize("n_grids", [1, 2])
def test_composite_equals_the_chain_of_public_calls(gpu, oracle, n_grids):
    import torch
    from msf_loam_amd import capi
    cfg = capi.novelty_config(keep_classes=0b0110)
    grids = list(_two_stores(gpu, oracle))[:n_grids]
    pose = _pose(33)
    scan = _world_scan(34, pose)
    # the chain, host memory
    img, _ = grids[0].render(pose, cfg.image)
    for g in grids[1:]:
        img, _ = g.render(pose, cfg.image, image=img, accumulate=True)
    want = gpu.scan_novelty(scan, img, cfg)
    assert len(set(want["cls"].tolist())) == 4                                       # every class occurs
    got = capi.grids_scan_novelty(grids, scan, pose, cfg, want_image=True)
    assert got["image"].tobytes() == img.tobytes() and np.array_equal(got["cls"], want["cls"]) and got["masked"].tobytes() == want["masked"].tobytes()
    assert got["info"].as_tuple() == want["info"].as_tuple()
    # device memory: with the image, and without it (the image stays in the handle's scratch)
    n = len(scan)
    d_scan, d_pose = torch.from_numpy(scan).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(pose)).to("cuda:0")
    for with_image in (True, False):
        d_cls = torch.full((n,), 9, dtype=torch.uint8, device="cuda:0")
        d_masked = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
        d_img = torch.zeros((cfg.image.n_row, cfg.image.n_col), dtype=torch.float32, device="cuda:0") if with_image else None
        torch.cuda.synchronize()
        info = capi.grids_scan_novelty_device(grids, d_scan, n, d_pose, cfg, d_cls, d_masked, d_img, want_info=True)
        assert info.as_tuple() == want["info"].as_tuple()
        assert np.array_equal(d_cls.cpu().numpy(), want["cls"]) and d_masked.cpu().numpy().tobytes() == want["masked"].tobytes()
        if with_image:
            assert d_img.cpu().numpy().tobytes() == img.tobytes()
    for g in grids:
        g.close()


def test_composite_refusals(gpu, oracle):
    import torch
    from msf_loam_amd import capi
    a, b = _two_stores(gpu, oracle)
    cfg = capi.novelty_config()
    pose = np.ascontiguousarray(_pose(35))
    scan = _world_scan(36, pose, n=500)
    n = len(scan)
    cls, masked, img, info = np.full(n, 9, np.uint8), np.full((n, 4), 5.0, F), np.full((16, 720), 7.0, F), capi.NoveltyInfo()
    vp, lib = capi._vp, gpu.lib
    arr = (ctypes.c_void_p * 9)(*([a.g.value, b.g.value] * 4 + [a.g.value]))
    call = lambda grids=arr, n_grids=2, p=pose, s=scan, m=masked: lib.msfl_grids_scan_novelty(grids, n_grids, vp(s), n, vp(p), ctypes.byref(cfg), vp(cls), vp(m),
                                                                                           vp(img), ctypes.byref(info), capi.MEM_HOST)
    assert call(n_grids=0) == capi.BAD_ARG and call(n_grids=9) == capi.BAD_ARG and call(grids=None) == capi.BAD_ARG
    assert call(p=None) == capi.BAD_ARG and call(s=None) == capi.BAD_ARG and call(m=scan) == capi.BAD_ARG
    other = capi.Handle(0)
    c = capi.Grid(other, 3.0, 0.4)
    mixed = (ctypes.c_void_p * 2)(a.g.value, c.g.value)
    assert call(grids=mixed) == capi.BAD_ARG and "one handle" in gpu.last_error()
    c.close(); other.close()
    assert call(p=np.array([0, 0, np.inf, 0, 0, 0, 1.0])) == capi.BAD_ARG               # a host pose that is not finite
    assert (cls == 9).all() and (masked == 5.0).all() and (img == 7.0).all()           # the outputs of every refused call are untouched
    assert call(n_grids=8) == capi.OK and info.applied == 1
    # a device-resident pose that is not finite: all NONE, an empty image, applied = 0
    d_scan = torch.from_numpy(scan).to("cuda:0")
    d_bad = torch.from_numpy(np.array([0, 0, 0, np.nan, 0, 0, 1.0])).to("cuda:0")
    d_cls = torch.full((n,), 9, dtype=torch.uint8, device="cuda:0")
    d_masked = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
    d_img = torch.full((16, 720), 7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    r = capi.grids_scan_novelty_device([a, b], d_scan, n, d_bad, cfg, d_cls, d_masked, d_img, want_info=True, allow=(capi.BAD_ARG,))
    assert r.status == capi.BAD_ARG and r.as_tuple() == ((n, 0, 0, 0), 0, n, 0)
    assert (d_cls.cpu().numpy() == nn.NONE).all() and np.isinf(d_img.cpu().numpy()).all()
    assert d_masked.cpu().numpy().tobytes() == scan.tobytes()                          # NONE is kept by the defaults: the scan passes
    a.close(); b.close()


# ---- stream-ordered use ---------------------------------------------------------------------------------------------------------------

def _extract_device(gpu, d_pts, d_ring, n):
    """msfl_extract_features_batch on the device arrays of one scan; the outputs as numpy arrays."""
    import torch
    from msf_loam_amd import capi
    t = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda:0")
    out = dict(full=t((n, 4), torch.float32), ring=t((n,), torch.int16), curvature=t((n,), torch.float32), label=t((n,), torch.uint8),
               sharp=t((n,), torch.int32), less_sharp=t((n,), torch.int32), flat=t((n,), torch.int32), less_flat=t((n,), torch.int32))
    d_cnt, d_status = t((5, 1), torch.int32), t((1,), torch.int32)
    f = capi.FeaturesBatch()
    f.full_pts, f.full_ring, f.curvature, f.label = (out[k].data_ptr() for k in ("full", "ring", "curvature", "label"))
    f.sharp_idx, f.less_sharp_idx, f.flat_idx, f.less_flat_idx = (out[k].data_ptr() for k in ("sharp", "less_sharp", "flat", "less_flat"))
    f.n_full, f.n_sharp, f.n_less_sharp, f.n_flat, f.n_less_flat = (d_cnt[k].data_ptr() for k in range(5))
    off = np.array([0, n], np.int32)
    torch.cuda.synchronize()
    s = gpu.lib.msfl_extract_features_batch(gpu.h, 1, capi._vp(d_pts), capi._vp(d_ring), capi._vp(off), ctypes.byref(f), capi._vp(d_status), capi.MEM_DEVICE)
    assert s == capi.OK, gpu.last_error()
    gpu.synchronize()
    c = d_cnt.cpu().numpy()[:, 0]
    assert int(d_status.cpu().numpy()[0]) == 0
    cnt = dict(full=c[0], ring=c[0], curvature=c[0], label=c[0], sharp=c[1], less_sharp=c[2], flat=c[3], less_flat=c[4])
    return {k: v.cpu().numpy()[:cnt[k]] for k, v in out.items()}


def test_masked_cloud_goes_straight_into_extraction(gpu, oracle):
    """Device memory, info = NULL: nothing waits between the labels and the extraction.  The feature lists equal those of the
    model-masked cloud, the contract tests/test_gpu_segment.py pins for the segmentation."""
    import torch
    from msf_loam_amd import capi, synth
    from tests import common
    w, _, _ = common.small_world(20000)
    poses = synth.random_poses(2, synth.SEED + 3)
    first, _ = synth.make_scan(w, poses[0], synth.SEED + 50, n_az=600)
    pts, ring = synth.make_scan(w, poses[1], synth.SEED + 51, n_az=600)
    cfg = capi.novelty_config()
    gg, m = _stores(gpu, oracle, oracle.transform_cloud(first, poses[0]), 0.4)
    tables = capi.carve_tables(cfg.image)
    img, _ = nn.render(m, poses[1], cfg, tables)
    cls = nn.classify(pts, img, cfg, tables)
    masked = nn.mask(pts, cls, cfg.keep_classes)
    assert 20 < (cls == nn.IN_FRONT).sum() < len(pts) // 4 and np.array_equal(np.isnan(masked[:, 0]), cls == nn.IN_FRONT)
    want = gpu.extract_features(masked, ring)
    n = len(pts)
    d_scan, d_ring = torch.from_numpy(pts).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(ring).view(np.int16)).to("cuda:0")
    d_pose = torch.from_numpy(np.ascontiguousarray(poses[1], np.float64)).to("cuda:0")
    d_cls, d_masked = torch.zeros((n,), dtype=torch.uint8, device="cuda:0"), torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert capi.grids_scan_novelty_device([gg], d_scan, n, d_pose, cfg, d_cls, d_masked) is None
    got = _extract_device(gpu, d_masked, d_ring, n)
    assert np.array_equal(d_cls.cpu().numpy(), cls) and len(want["full"]) > 1000
    for k in ("full", "curvature", "label", "sharp", "less_sharp", "flat", "less_flat"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["ring"].view(np.uint16).tobytes() == want["ring"].tobytes()
    gg.close()


# ---- example --------------------------------------------------------------------------------------------------------------------------

def test_example_runs_and_its_unfiltered_variant_is_clean_maps_pass_1(gpu):
    """examples/filter_moving.py --scans 20 is what this test is about.  No bar on the ghost counts: they are measurements."""
    from msf_loam_amd import capi, synth
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "examples", "filter_moving.py"), "--scans", "20"], cwd=ROOT).decode()
    res = json.loads(out.strip().splitlines()[-1])
    assert res["scans"] == 20 and res["label_from"] == 10 and set(res) >= {"config", "unfiltered", "feature_stores", "full_store", "prototype_cpu"}
    for variant in ("unfiltered", "feature_stores", "full_store"):
        v = res[variant]
        assert set(v) >= {"corner", "surf", "static_withheld", "static_returns", "box_returns", "box_in_front", "box_in_front_share"}
        for store in ("corner", "surf"):
            assert set(v[store]) >= {"ghosts", "points", "sha256"} and v[store]["points"] > 0
    assert res["unfiltered"]["static_withheld"] == 0 and res["feature_stores"]["box_returns"] > 0
    # pass 1 of examples/clean_map.py, from its own pieces
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import clean_map as cm
    import replay_synthetic as rp
    world, truth, centres = synth.World(ground_half=45.0), rp.trajectory(20), cm.box_centres(20)
    stores = {"corner": capi.Grid(gpu, 3.0, 0.2), "surf": capi.Grid(gpu, 3.0, 0.4)}
    for k in range(20):
        pts, ring = cm.scan_with_box(world, truth[k], centres[k], synth.SEED + 7000 + k)
        f = gpu.extract_features(pts, ring)
        for name, key in (("corner", "less_sharp"), ("surf", "less_flat")):
            stores[name].insert_scan(gpu.transform_cloud(gpu.voxel_downsample(f["full"][f[key]], stores[name].leaf), truth[k]))
    for name, g in stores.items():
        dump = g.dump()
        assert res["unfiltered"][name]["points"] == len(dump) and res["unfiltered"][name]["sha256"] == hashlib.sha256(dump.tobytes()).hexdigest()
        assert res["unfiltered"][name]["ghosts"] == int(cm.is_ghost(dump, centres, world).sum())
        g.close()
