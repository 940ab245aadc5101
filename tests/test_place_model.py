"""CPU: the place-recognition plumbing (header, exports, record layout) and the numpy model of its definition
(tests/place_numpy.py) on synthetic worlds and on hand-made points.  The GPU side is tests/test_gpu_place.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import place_numpy as pn
from msf_loam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["msfl_places_default_config", "msfl_places_create", "msfl_places_destroy", "msfl_places_set_stream", "msfl_places_synchronize",
         "msfl_places_size", "msfl_places_last_error", "msfl_places_add", "msfl_places_add_descriptors", "msfl_places_get",
         "msfl_places_query", "msfl_places_query_entries"]


def test_header_library_and_binding_agree():
    from msf_loam_amd import capi
    text = open(os.path.join(ROOT, "include", "msfl_c_api.h")).read()
    assert re.search(r"#define\s+MSFL_API_VERSION\s+1\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), "not declared: " + n
        assert n in capi.EXPORTED
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(capi.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), "missing export: " + n
    assert ctypes.sizeof(capi.PlaceMatch) == 24 and capi.PLACE_MATCH_DTYPE.itemsize == 24
    assert capi.load().msfl_api_version() == 1
    c = capi.PlaceConfig()
    lib.msfl_places_default_config(ctypes.byref(c))
    assert (c.n_ring, c.n_sector, c.min_range, c.max_range, c.height_offset, c.capacity) == (20, 60, 0.3, 80.0, 2.0, 16384)


def test_place_yaw():
    from msf_loam_amd import capi
    assert capi.place_yaw(0, 60) == 0.0
    assert np.isclose(capi.place_yaw(15, 60), np.pi / 2) and np.isclose(capi.place_yaw(54, 60), -np.deg2rad(36.0))
    assert np.isclose(capi.place_yaw(30, 60), np.pi)                       # (-pi, pi]
    assert np.allclose(capi.place_yaw(np.array([15, 45]), 60), [np.pi / 2, -np.pi / 2])


def _revisit(pose, yaw_deg):
    p = np.array(pose, np.float64)
    p[0] += 0.5
    p[1] += 0.3
    q = synth.quat_mul(p[3:], synth.quat_from_rotvec([0.0, 0.0, np.deg2rad(yaw_deg)]))
    p[3:] = q / np.linalg.norm(q)
    return p


@pytest.mark.parametrize("kind", ["outdoor", "room"])
def test_model_recognises_revisited_places(kind):
    cfg = pn.Config()
    w = synth.World(kind=kind)
    poses = synth.world_poses(w, 8)
    db = np.stack([pn.describe(cfg, synth.make_scan(w, poses[i], 100 + i)[0]) for i in range(8)])
    case = 0
    for place in (0, 3, 5):
        for yaw, shift in ((90.0, 15), (-36.0, 54)):
            q = pn.describe(cfg, synth.make_scan(w, _revisit(poses[place], yaw), 900 + case)[0])
            case += 1
            full = pn.query(q, db, k=2)
            assert full["index"][0] == place and full["shift"][0] == shift, (kind, place, yaw, full)
            assert full["distance"][0] < full["distance"][1]
            d2 = pn.ring_key_d2(q, db)
            assert place in np.argsort(d2, kind="stable")[:3]
            pre = pn.query(q, db, n_prefilter=4, k=1)
            assert pre["index"][0] == place and pre["shift"][0] == shift and pre["distance"][0] == full["distance"][0]


def test_model_axes_and_ring_edges():
    cfg = pn.Config()
    pts = np.zeros((4, 4), np.float32)
    pts[:, :2] = [[5, 0], [0, 5], [-5, 0], [0, -5]]
    ring, sector, v, keep = pn.bins(cfg, pts)
    assert keep.all() and list(sector) == [0, 15, 30, 45] and list(ring) == [1, 1, 1, 1]
    assert np.all(v == np.float32(2.0))
    # a point whose r2 is exactly a table entry belongs to the ring that starts there; the outer edge is outside
    for k in (1, 2, 7, 19):
        x = np.float32(k * 4.0)                                           # 4 m rings: x*x is the table's value exactly
        assert x * x == cfg.e2[k]
        r, _, _, kp = pn.bins(cfg, np.array([[x, 0, 0, 0]], np.float32))
        assert kp[0] and r[0] == k
        r, _, _, kp = pn.bins(cfg, np.array([[np.nextafter(x, np.float32(0)), 0, 0, 0]], np.float32))
        assert kp[0] and r[0] == k - 1
    assert np.float32(80.0) * np.float32(80.0) == cfg.e2[20]
    assert not pn.bins(cfg, np.array([[80.0, 0, 0, 0]], np.float32))[3][0]
    assert pn.bins(cfg, np.array([[np.nextafter(np.float32(80.0), np.float32(0)), 0, 0, 0]], np.float32))[3][0]
    # below min_range, at or below the height floor, not finite: skipped
    bad = np.array([[0.1, 0.1, 0, 0], [5, 0, -2.0, 0], [5, 0, -3.0, 0], [np.nan, 1, 0, 0], [1, np.inf, 0, 0], [1, 1, np.nan, 0]], np.float32)
    assert not pn.bins(cfg, bad)[3].any()


def test_model_distance_and_shift_of_a_rolled_descriptor():
    cfg = pn.Config()
    rng = np.random.default_rng(3)
    D = (rng.uniform(0, 5, (20, 60)) * (rng.uniform(size=(20, 60)) < 0.6)).astype(np.float32)
    for s in (0, 1, 15, 59):
        m = pn.query(D, np.roll(D, s, axis=1)[None], k=1)               # entry column j + s holds query column j
        assert m["shift"][0] == s and abs(m["distance"][0]) < 1e-15
    z = np.zeros_like(D)
    m = pn.query(z, D[None], k=2)
    assert m["index"].tolist() == [0, -1] and np.isinf(m["distance"]).all() and m["n_columns"].tolist() == [0, 0]
    del cfg


def test_place_file_is_checked_when_it_is_read(tmp_path):
    from msf_loam_amd import mapio
    cfg = dict(n_ring=np.int32(4), n_sector=np.int32(6), min_range=0.3, max_range=20.0, height_offset=2.0, capacity=np.int32(8))
    good = np.random.default_rng(1).uniform(0, 3, (3, 4, 6)).astype(np.float32)

    def write(name, desc, **over):
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            np.savez(f, places_format=np.int32(over.pop("fmt", mapio.PLACES_FORMAT)), descriptors=desc, **{**cfg, **over})
        return path

    c, d = mapio.read_places(write("good.npz", good))
    assert c == dict(n_ring=4, n_sector=6, min_range=0.3, max_range=20.0, height_offset=2.0, capacity=8) and np.array_equal(d, good)
    bad = good.copy()
    for v in (-1.0, np.nan, np.inf):
        bad[1, 2, 3] = v
        with pytest.raises(mapio.MapFileError):
            mapio.read_places(write("bad.npz", bad))
    for path in (write("shape.npz", good[:, :3]), write("dtype.npz", good.astype(np.float64)), write("fmt.npz", good, fmt=2)):
        with pytest.raises(mapio.MapFileError):
            mapio.read_places(path)
    with open(tmp_path / "other.npz", "wb") as f:
        np.savez(f, cells=np.zeros((0, 4), np.int32))
    with pytest.raises(mapio.MapFileError):
        mapio.read_places(str(tmp_path / "other.npz"))
