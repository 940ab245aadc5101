"""GPU: msfl_segment_scans against the numpy model (tests/segment_numpy.py).  Every output array and every info field is compared
with array_equal (NaN by bit pattern): classes, component ids, the masked cloud and the ten counters per scan."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segment_cases as sc
import segment_numpy as sn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = sc.hand_scenes()
STRESS = sc.stress_scenes()


def _c_config(cfg):
    from msf_loam_amd import capi
    return capi.SegmentConfig(**vars(cfg))


def _info_rows(info):
    """SEGMENT_INFO_DTYPE records as the model's (n, 10) int32 rows."""
    return np.ascontiguousarray(info).view(np.int32).reshape(-1, 10)


def _assert_equal(got, want, what=""):
    assert sn.same_bits(got["cls"], want["cls"]), what + " cls"
    assert sn.same_bits(got["segment"], want["segment"]), what + " segment"
    assert sn.same_bits(got["masked"], want["masked"]), what + " masked"
    assert np.array_equal(_info_rows(got["info"]), np.atleast_2d(want["info"])), (what, _info_rows(got["info"]), want["info"])


def _host(gpu, pts, ring, off, cfg):
    return gpu.segment_scans(pts, ring, off, _c_config(cfg))


def _device(gpu, pts, ring, off, cfg, want_info=True):
    import torch
    d_pts = torch.from_numpy(np.ascontiguousarray(pts)).to("cuda:0")
    d_ring = torch.from_numpy(np.ascontiguousarray(ring).view(np.int16)).to("cuda:0")
    torch.cuda.synchronize()
    out = gpu.segment_scans(d_pts, d_ring, off, _c_config(cfg), want_info=want_info)
    gpu.synchronize()
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}


@pytest.mark.parametrize("scene", HAND, ids=[s[0] for s in HAND])
def test_hand_scenes(gpu, scene):
    name, pts, ring, cfg, want_cls = scene
    got = _host(gpu, pts, ring, [0, len(pts)], cfg)
    assert got["cls"].tolist() == want_cls.tolist()
    _assert_equal(got, sn.segment_scans(pts, ring, [0, len(pts)], cfg), name)


@pytest.mark.parametrize("scene", STRESS, ids=[s[0] for s in STRESS])
def test_component_shapes(gpu, scene):
    name, pts, ring, cfg, want_cls, n_comp = scene
    rng = np.random.default_rng(3)
    for order in (np.arange(len(pts)), rng.permutation(len(pts))):
        got = _host(gpu, pts[order], ring[order], [0, len(pts)], cfg)
        _assert_equal(got, sn.segment_scans(pts[order], ring[order], [0, len(pts)], cfg), name)
        assert got["info"]["n_components"][0] == n_comp and got["info"]["n_segments"][0] == n_comp


@pytest.mark.parametrize("shape", [(2, 4), (16, 1800), (64, 2048), (128, 2048)], ids=lambda s: "%dx%d" % s)
def test_seeded_images(gpu, shape):
    pts, ring, cfg = sc.random_image(100 + shape[0], *shape)
    want = sn.segment_scans(pts, ring, [0, len(pts)], cfg)
    _assert_equal(_host(gpu, pts, ring, [0, len(pts)], cfg), want, "host %dx%d" % shape)
    _assert_equal(_device(gpu, pts, ring, [0, len(pts)], cfg), want, "device %dx%d" % shape)
    if shape[0] >= 16:
        assert len(pts) > 0.9 * shape[0] * shape[1] and all(want["info"][0, k] > 0 for k in range(8))


@pytest.fixture(scope="module")
def ragged():
    pts, ring, off, cfg = sc.ragged_batch()
    return pts, ring, off, cfg, sn.segment_scans(pts, ring, off, cfg)


def test_ragged_batch_equals_the_model_and_single_calls(gpu, ragged):
    pts, ring, off, cfg, want = ragged
    assert off[6] == off[5] and off[18] - off[17] == 1
    _assert_equal(_host(gpu, pts, ring, off, cfg), want, "batch")
    for b in range(len(off) - 1):
        one = gpu.segment_scan(pts[off[b]:off[b + 1]], ring[off[b]:off[b + 1]], _c_config(cfg))
        for k in ("cls", "segment", "masked"):
            assert sn.same_bits(one[k], want[k][off[b]:off[b + 1]]), (b, k)
        assert np.array_equal(_info_rows(one["info"])[0], want["info"][b]), b


def test_ragged_batch_device_memory_and_no_info(gpu, ragged):
    pts, ring, off, cfg, want = ragged
    _assert_equal(_device(gpu, pts, ring, off, cfg), want, "device")
    quiet = _device(gpu, pts, ring, off, cfg, want_info=False)
    assert quiet["info"] is None
    for k in ("cls", "segment", "masked"):
        assert sn.same_bits(quiet[k], want[k]), k


def test_ragged_batch_in_chunks_of_five(gpu, ragged, monkeypatch):
    from msf_loam_amd import capi
    pts, ring, off, cfg, want = ragged
    monkeypatch.setenv("MSFL_SEG_CHUNK_SCANS", "5")
    h = capi.Handle(0)
    try:
        _assert_equal(h.segment_scans(pts, ring, off, _c_config(cfg)), want, "chunks of 5")
    finally:
        h.close()


def test_a_batch_that_does_not_start_at_zero(gpu, ragged):
    """off[0] > 0: only the region [off[0], off[n_scans]) of every array is read and written."""
    pts, ring, off, cfg, want = ragged
    sub = off[10:21]
    got = _host(gpu, pts, ring, sub, cfg)
    lo, hi = sub[0], sub[-1]
    for k in ("cls", "segment", "masked"):
        assert sn.same_bits(got[k][lo:hi], want[k][lo:hi]), k
    assert not got["cls"][:lo].any() and not got["cls"][hi:].any()
    assert np.array_equal(_info_rows(got["info"]), want["info"][10:20])


def test_shuffled_scan_gives_the_same_classes(gpu):
    """No two points of a pixel share a range, so the winner does not depend on the order of the points."""
    pts, ring = sc.sweep("outdoor")
    cfg = sn.config()
    assert len(np.unique(pts[:, :3], axis=0)) == len(pts)
    a = _host(gpu, pts, ring, [0, len(pts)], cfg)
    perm = np.random.default_rng(9).permutation(len(pts))
    b = _host(gpu, pts[perm], ring[perm], [0, len(pts)], cfg)
    assert np.array_equal(a["cls"][perm], b["cls"]) and np.array_equal(a["segment"][perm], b["segment"])
    assert sn.same_bits(a["masked"][perm], b["masked"]) and np.array_equal(_info_rows(a["info"]), _info_rows(b["info"]))


@pytest.mark.parametrize("kind", ["room", "outdoor"])
@pytest.mark.parametrize("rows", ["uniform", "table"])
def test_real_sweeps(gpu, kind, rows):
    pts, ring = sc.sweep(kind, 1)
    cfg = sn.config() if rows == "uniform" else sn.config(row_elev_deg=[-15.0 + 2.0 * k + 0.125 * (k % 3) for k in range(16)])
    want = sn.segment_scans(pts, ring, [0, len(pts)], cfg)
    _assert_equal(_host(gpu, pts, ring, [0, len(pts)], cfg), want, kind + " " + rows)
    assert want["info"][0, sn.GROUND] > 5000 and want["info"][0, sn.SEGMENT] > 1000


def test_masked_cloud_through_extraction(gpu):
    """Extraction of masked_out equals extraction of the host-compacted kept points, bit for bit in every output."""
    pts, ring = sc.sweep("outdoor", 2)
    out = gpu.segment_scan(pts, ring)
    keep = np.isin(out["cls"], (sn.GROUND, sn.SEGMENT))
    assert 0.5 * len(pts) < keep.sum() < len(pts) and np.array_equal(np.isnan(out["masked"][:, 0]), ~keep)
    a = gpu.extract_features(out["masked"], ring)
    b = gpu.extract_features(pts[keep], ring[keep])
    assert a["rc"] == 0 and b["rc"] == 0 and len(a["full"]) > 1000
    for k in ("full", "ring", "curvature", "label", "sharp", "less_sharp", "flat", "less_flat"):
        assert sn.same_bits(a[k], b[k]), k


def test_raw_single_scan_entry_point(gpu):
    """msfl_segment_scan called raw (cfg = NULL: the defaults; segment_out = masked_out = info = NULL)."""
    from msf_loam_amd import capi
    pts, ring = sc.sweep("room")
    cls = np.zeros(len(pts), np.uint8)
    s = gpu.lib.msfl_segment_scan(gpu.h, capi._vp(pts), capi._vp(ring), len(pts), None, capi._vp(cls), None, None, None, capi.MEM_HOST)
    assert s == capi.OK
    assert np.array_equal(cls, sn.segment_scan(pts, ring, sn.config())["cls"])


def test_refusals(gpu):
    from msf_loam_amd import capi
    name, pts, ring, cfg, _ = HAND[3]
    n = len(pts)
    import test_segment_model as tm
    for bad in tm.BAD:
        with pytest.raises(capi.MsflError) as e:
            gpu.segment_scan(pts, ring, capi.SegmentConfig(**{**dict(n_col=1800, n_row=16), **bad}))
        assert e.value.status == capi.BAD_ARG, bad
    c = _c_config(cfg)
    cls, info = np.zeros(n, np.uint8), np.zeros(1, capi.SEGMENT_INFO_DTYPE)
    vp, lib = capi._vp, gpu.lib
    off = np.array([0, n], np.int32)
    call = lambda **kw: lib.msfl_segment_scans(gpu.h, kw.get("n_scans", 1), vp(kw.get("pts", pts)), vp(kw.get("ring", ring)), vp(kw.get("off", off)),
                                               ctypes.byref(c), vp(kw.get("cls", cls)), None, vp(kw.get("masked")), vp(info), capi.MEM_HOST)
    assert call() == capi.OK
    assert call(n_scans=-1) == capi.BAD_ARG and call(off=None) == capi.BAD_ARG
    assert call(off=np.array([0, -1], np.int32)) == capi.BAD_ARG and call(off=np.array([-1, n - 1], np.int32)) == capi.BAD_ARG
    assert call(pts=None) == capi.BAD_ARG and call(ring=None) == capi.BAD_ARG and call(cls=None) == capi.BAD_ARG
    assert call(masked=pts) == capi.BAD_ARG                                         # masked_out aliases pts
    assert call(masked=pts[n // 2:]) == capi.BAD_ARG                                # ... or overlaps it
    assert "overlaps" in gpu.last_error()
    assert lib.msfl_segment_scan(gpu.h, vp(pts), vp(ring), -1, ctypes.byref(c), vp(cls), None, None, None, capi.MEM_HOST) == capi.BAD_ARG
    assert lib.msfl_segment_scans(None, 1, vp(pts), vp(ring), vp(off), None, vp(cls), None, None, None, capi.MEM_HOST) == capi.BAD_ARG
    assert call(n_scans=0) == capi.OK
    # after the refusals the handle segments as before
    _assert_equal(_host(gpu, pts, ring, [0, n], cfg), sn.segment_scans(pts, ring, [0, n], cfg), "after refusals")


def _example(args, cwd):
    run = subprocess.run([sys.executable] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    return run.stdout


def test_segment_scan_example_runs(tmp_path):
    """examples/segment_scan.py is what this test is about: it finishes and its class counts add up to the sweep."""
    import json
    out = _example([os.path.join(ROOT, "examples", "segment_scan.py"), "--json"], str(tmp_path))
    rec = json.loads(out.strip().splitlines()[-1])
    assert sum(rec["class_counts"].values()) == rec["n_points"] > 10000
    assert sum(sum(v.values()) for v in rec["by_kind"].values()) == rec["n_points"]
    assert set(rec["raw"]) == set(rec["masked"]) and rec["masked"]["n_less_flat"] > 0


def test_replay_with_segmentation_runs(tmp_path):
    """examples/replay_synthetic.py --segment is what this test is about: the masked device cloud goes through msfl_slam_add_scan."""
    import json
    out = _example([os.path.join(ROOT, "examples", "replay_synthetic.py"), "--scans", "4", "--segment"], str(tmp_path))
    rec = json.loads([l for l in out.strip().splitlines() if l.startswith("{")][-1])
    seg = rec["segment"]
    assert sum(seg["class_counts"].values()) == seg["n_points"] > 4 * 10000 and "ate_m" in seg
