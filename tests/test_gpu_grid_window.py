"""Windowed local map: msfl_grid_crop / msfl_grid_dump_cells / msfl_grid_stats and msfl_slam_set_map_window against the
model of tests/windowed_grid_model.py (oracle.HybridGrid replayed over the surviving history), bit for bit."""
import os
import re
import sys

import numpy as np
import pytest

from msf_loam_amd import synth
from tests import windowed_grid_model as wm
from tests.test_grid_store import _batches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
import replay_synthetic as rp  # noqa: E402

pytestmark = pytest.mark.gpu


def _same_map(gg, m, queries, what):
    assert gg.size() == m.size(), what
    assert np.array_equal(gg.dump(), m.dump()), what
    assert np.array_equal(gg.dump_cells(), m.dump_cells()), what
    for scan, pose in queries:
        assert np.array_equal(gg.get_surrounded(scan, pose), m.get_surrounded(scan, pose)), what


@pytest.mark.parametrize("leaf", [0.2, 0.4])
def test_crop_equals_the_model(gpu, oracle, leaf):
    """Inserts 1, 2 -> crop (2, 2, 1) around scan 2's pose -> inserts 3, 4 (evicted cells are created again, from nothing) -> crop
    around a centre 9 m further on (some of them go again).  After every step the store equals the model: sizes, dump, cell
    list, two surround queries, the crop's counts and the evicted points; and dump_before is the cell-wise merge of dump_after
    and what was evicted."""
    from msf_loam_amd import capi
    bs = _batches()
    queries = [(bs[1][0], bs[1][2]), (bs[0][0], bs[0][2])]
    gg, m = capi.Grid(gpu, 3.0, leaf), wm.WindowedGrid(oracle, 3.0, leaf)
    centre = np.array(bs[1][2][:3], np.float64)
    seen_again, inserted = 0, 0
    for step, action in enumerate(("insert", "insert", "crop", "insert", "insert", "crop")):
        if action == "insert":
            wp = bs[inserted][1]
            inserted += 1
            assert m.insert_scan(wp) == 0
            gg.insert_scan(wp)
        else:
            cells_b, dump_b = gg.dump_cells(), gg.dump()
            info_m, cells_e, pts_e = m.crop(centre, (2, 2, 1), keep_evicted=True)
            info_g, ev_g = gg.crop(centre, (2, 2, 1), keep_evicted=True)
            assert info_g.status == capi.OK and info_g.as_tuple() == info_m.as_tuple(), (step, info_g.as_tuple(), info_m.as_tuple())
            assert info_g.n_cells_evicted > 0 and info_g.n_cells > 0
            assert np.array_equal(ev_g, pts_e), step
            cells_a = gg.dump_cells()
            gone = np.array(sorted(set(map(tuple, cells_b.tolist())) - set(map(tuple, cells_a.tolist())), key=lambda c: (c[2], c[1], c[0])), np.int32)
            assert np.array_equal(gone, cells_e), step
            cells_mg, dump_mg = wm.merge_cellwise(cells_a, gg.dump(), gone, ev_g)
            assert np.array_equal(cells_mg, cells_b) and np.array_equal(dump_mg, dump_b), step
            if step == 2:
                first_gone = set(map(tuple, cells_e[:, :3].tolist()))
            else:
                seen_again = len(first_gone & set(map(tuple, cells_b[:, :3].tolist())))
                assert len(first_gone & set(map(tuple, cells_e[:, :3].tolist()))) > 0          # ... and some are evicted again
            centre = centre + np.array([9.0, 0.0, 0.0])
        _same_map(gg, m, queries, (leaf, step, action))
    assert seen_again > 0                                            # cells evicted by the first crop were created again by inserts 3, 4
    gg.close()


def test_crop_edges(gpu, oracle):
    import torch
    from msf_loam_amd import capi
    bs = _batches()
    scan, wp, pose = bs[0]
    gg = capi.Grid(gpu, 3.0, 0.4)
    # an empty grid
    info = gg.crop((1.0, 2.0, 3.0), (1, 1, 1))
    assert info.as_tuple() == (0, 0, 0, 0, (0, 1, 1), 1) and gg.size() == (0, 0) and len(gg.dump()) == 0 and len(gg.dump_cells()) == 0
    assert gg.stats()["n_cells"] == 0
    # everything goes; the next insert and query equal a fresh grid's
    gg.insert_scan(wp)
    n_pts, n_cells = gg.size()
    info, ev = gg.crop((3000.0, 0, 0), (1, 1, 1), keep_evicted=True)
    fresh = oracle.HybridGrid(3.0, 0.4); fresh.insert_scan(wp)
    assert info.as_tuple() == (n_cells, n_pts, 0, 0, (1000, 0, 0), 1) and np.array_equal(ev, fresh.dump())
    assert gg.size() == (0, 0) and len(gg.dump()) == 0 and len(gg.dump_cells()) == 0 and len(gg.get_surrounded(scan, pose)) == 0
    assert gg.crop((0, 0, 0), (0, 0, 0)).as_tuple() == (0, 0, 0, 0, (0, 0, 0), 1)             # a table cropped to zero cells, cropped again
    gg.insert_scan(bs[1][1])
    fresh = oracle.HybridGrid(3.0, 0.4); fresh.insert_scan(bs[1][1])
    assert gg.size() == fresh.size() and np.array_equal(gg.dump(), fresh.dump())
    assert np.array_equal(gg.get_surrounded(bs[1][0], bs[1][2]), fresh.get_surrounded(bs[1][0], bs[1][2]))
    # nothing goes
    before, cells_before = gg.dump(), gg.dump_cells()
    info, ev = gg.crop(bs[1][2][:3], (60, 60, 60), keep_evicted=True)
    assert info.as_tuple()[:4] == (0, 0) + gg.size()[::-1] and info.applied == 1 and len(ev) == 0
    assert np.array_equal(gg.dump(), before) and np.array_equal(gg.dump_cells(), cells_before)
    assert np.array_equal(gg.get_surrounded(bs[1][0], bs[1][2]), fresh.get_surrounded(bs[1][0], bs[1][2]))
    # one point short of the room needed: refused as a whole, the counts name the need, the retry succeeds
    centre = bs[1][2][:3]
    m = wm.WindowedGrid(oracle, 3.0, 0.4); m.insert_scan(bs[1][1])
    info_m, cells_e, pts_e = m.crop(centre, (2, 2, 1), keep_evicted=True)
    assert len(pts_e) > 1
    info, ev = gg.crop(centre, (2, 2, 1), keep_evicted=True, capacity=len(pts_e) - 1, allow=(capi.CAPACITY,))
    assert info.status == capi.CAPACITY and info.applied == 0 and len(ev) == 0
    assert (info.n_cells_evicted, info.n_points_evicted) == (len(cells_e), len(pts_e)) and (info.n_points, info.n_cells) == fresh.size()
    assert np.array_equal(gg.dump(), before) and np.array_equal(gg.dump_cells(), cells_before) and gg.size() == fresh.size()
    assert np.array_equal(gg.get_surrounded(bs[1][0], bs[1][2]), fresh.get_surrounded(bs[1][0], bs[1][2]))
    # the device-pointer form on a twin grid equals the host form
    twin = capi.Grid(gpu, 3.0, 0.4); twin.insert_scan(bs[1][1])
    dev = torch.zeros((len(pts_e), 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    info_d = twin.crop_device(centre, (2, 2, 1), dev, len(pts_e))
    info, ev = gg.crop(centre, (2, 2, 1), keep_evicted=True, capacity=len(pts_e))
    assert info.status == capi.OK and info.as_tuple() == info_m.as_tuple() == info_d.as_tuple()
    assert np.array_equal(ev, pts_e) and np.array_equal(dev.cpu().numpy(), pts_e)
    assert np.array_equal(gg.dump(), m.dump()) and np.array_equal(twin.dump(), m.dump()) and np.array_equal(twin.dump_cells(), m.dump_cells())
    twin.close()
    # half_cells = 0 keeps exactly the centre cell; a centre on a half-integer cell boundary follows lround (away from zero)
    for x, cx in ((1.5, 1), (-1.5, -1), (1.4999, 0), (-1.4999, 0), (4.5, 2)):
        g2 = capi.Grid(gpu, 3.0, 0.4)
        pts = np.array([[-3.0, 0.2, 0.1, 0], [0.1, 0.2, 0.1, 0], [3.0, 0.2, 0.1, 0], [6.0, 0.2, 0.1, 0], [0.1, 3.2, 0.1, 0], [0.1, 0.2, 3.1, 0]], np.float32)
        g2.insert_scan(pts)
        info = g2.crop((x, 0.0, 0.0), (0, 0, 0))
        assert tuple(info.center_cell) == (cx, 0, 0) and g2.dump_cells().tolist() == [[cx, 0, 0, 1]], (x, g2.dump_cells().tolist())
        assert info.n_cells_evicted == 5 and g2.size() == (1, 1)
        g2.close()
    # bad arguments
    for centre_bad, half_bad in (((0, 0, 0), (-1, 0, 0)), ((0, 0, 0), (0, 0, -2)), ((np.nan, 0, 0), (1, 1, 1)), ((0, np.inf, 0), (1, 1, 1)), ((0, 0, 1e39), (1, 1, 1))):
        with pytest.raises(capi.MsflError) as e:
            gg.crop(centre_bad, half_bad)
        assert e.value.args and "msfl_grid_crop" in str(e.value)
    c3, h3 = (capi.C.c_double * 3)(0, 0, 0), (capi.C.c_int * 3)(1, 1, 1)
    assert gg.lib.msfl_grid_crop(gg.g, c3, h3, None, 0, 0, None) == capi.BAD_ARG                  # info == NULL
    assert np.array_equal(gg.dump(), m.dump())
    gg.close()


def _one_block_max():
    src = open(os.path.join(ROOT, "msf_loam_amd", "csrc", "msfl_grid.cuh")).read()
    return int(eval(re.search(r"constexpr int kGridOneBlockMax = ([0-9 <]+);", src).group(1)))


def test_both_table_forms_keep_the_same_cells(gpu):
    """More than kGridOneBlockMax live cells take the device-wide scans, fewer the one-workgroup form.  One isolated point per
    cell (its own centroid), the smallest count above the threshold and a smaller grid around the same window: cell list and
    evicted points against numpy set arithmetic on the keys."""
    from msf_loam_amd import capi
    n_big = _one_block_max() + 1
    nx = 512
    centre, half = (7.0, -10.0, 0.4), np.array([100, 60, 0])
    kept = {}
    for n in (n_big, 400 * 300):
        k = np.arange(n)
        w = nx if n == n_big else 400
        idx = np.stack([k % w - w // 2, k // w - (n // w) // 2, np.zeros(n, np.int64)], axis=1)
        pts = np.zeros((n, 4), np.float32)
        pts[:, :3] = idx * 3.0 + np.array([0.3, -0.2, 0.1])
        pts[:, 3] = (k % 97) / 1000.0
        pts = pts[np.random.default_rng(5).permutation(n)]
        g = capi.Grid(gpu, 3.0, 0.4)
        g.insert_scan(pts)
        assert g.size() == (n, n)
        keys = wm.cell_key(wm.cell_index(pts[:, :3], 3.0))
        by_key = pts[np.argsort(keys)]
        cells = wm.key_cell(np.sort(keys))
        c = wm.cell_index(np.array(centre, np.float32), 3.0)
        inside = (np.abs(cells - c) <= half).all(axis=1)
        assert 0 < inside.sum() == (2 * half[0] + 1) * (2 * half[1] + 1) < n
        info, ev = g.crop(centre, half, keep_evicted=True)
        assert info.as_tuple() == (int((~inside).sum()), int((~inside).sum()), int(inside.sum()), int(inside.sum()), tuple(c), 1)
        assert np.array_equal(ev, by_key[~inside])
        assert np.array_equal(g.dump_cells(), np.c_[cells[inside], np.ones(inside.sum(), np.int64)].astype(np.int32))
        assert np.array_equal(g.dump(), by_key[inside])
        kept[n] = g.dump_cells()
        g.close()
    assert np.array_equal(kept[n_big], kept[400 * 300])


def test_memory_stops_growing(gpu, oracle, monkeypatch):
    """300 copies of one 5 000-point cloud, 1.5 m further along x each, a small minimum pool so that the store compacts.  Cropped to
    (3, 3, 2) cells after every insert, the cell count and both capacities are at insert 300 what they were at insert 150, and the
    map equals the model.  Coordinates are multiples of 1/64 m and the leaf is 0.5 m, so cells (3 m) and voxels repeat exactly every
    two inserts and the counts of the two even inserts can be compared.
    Without the crop the map grows with the distance driven.  (The count of a union of translates is sub-additive, n(300) <=
    2 n(150) whatever the cloud; growth is linear, n(k) = c (k + a) with 0 <= a <= 16, the number of 1.5 m steps the 24 m cloud
    spans, so n(300) / n(150) >= 316 / 166 = 1.90: asserted as > 1.8, and as more than twice the windowed map.  Measured: 504 279 /
    257 679 = 1.957 without the crop, 13 527 points in the window.)"""
    from msf_loam_amd import capi
    monkeypatch.setenv("MSFL_GRID_MIN_POOL", "1024")
    rng = np.random.default_rng(11)
    cloud = np.zeros((5000, 4), np.float32)
    cloud[:, :3] = rng.integers(-768, 768, (5000, 3)) / 64.0 * np.array([1.0, 1.0, 0.25])       # +-12 m x +-12 m x +-3 m
    cloud[:, 3] = rng.uniform(0, 0.1, 5000)
    half = (3, 3, 2)
    g_win, g_free, m = capi.Grid(gpu, 3.0, 0.5), capi.Grid(gpu, 3.0, 0.5), wm.WindowedGrid(oracle, 3.0, 0.5)
    stats_win, stats_free = {}, {}
    for k in range(1, 301):
        pts = cloud.copy()
        pts[:, 0] += np.float32(1.5 * (k - 1))
        g_win.insert_scan(pts); g_free.insert_scan(pts); m.insert_scan(pts)
        c = (1.5 * (k - 1), 0.0, 0.0)
        info = g_win.crop(c, half)
        if k % 75 == 0:
            assert info.as_tuple() == m.crop(c, half).as_tuple(), k
        else:
            m.crop(c, half, counts=False)
        if k in (150, 300):
            stats_win[k], stats_free[k] = g_win.stats(), g_free.stats()
    a, b = stats_win[150], stats_win[300]
    print("windowed", a, b, "free", stats_free[150], stats_free[300])
    assert a["n_cells"] == b["n_cells"] > 0 and a["pool_capacity_points"] == b["pool_capacity_points"] and a["cell_capacity"] == b["cell_capacity"]
    assert b["pool_top"] <= b["pool_capacity_points"] and b["device_bytes"] >= 16 * b["pool_capacity_points"]
    assert g_win.size() == m.size() and np.array_equal(g_win.dump(), m.dump()) and np.array_equal(g_win.dump_cells(), m.dump_cells())
    assert stats_free[300]["n_points"] > 1.8 * stats_free[150]["n_points"] and stats_free[300]["n_points"] > 2 * a["n_points"]
    assert stats_free[300]["n_cells"] > 2 * b["n_cells"]
    g_win.close(); g_free.close()


def _records(recs):
    """The records as bytes, without the pool top of the two stores: when a store compacts follows from which reports the host had
    seen when it planned the insert, i.e. from timing in the pipelined form."""
    from msf_loam_amd import capi
    out = []
    for r in recs:
        c = capi.SlamResult.from_buffer_copy(bytes(r))
        c.grid_corner[2] = c.grid_surf[2] = 0
        out.append(bytes(c))
    return out


def _windowed_oracle_loop(oracle, world, truth, window):
    from tests.test_gpu_replay import OracleBackendRigid3d
    maps, infos = {}, []
    est, _ = rp.run(OracleBackendRigid3d(oracle), world, truth, maps_out=maps, map_window=window, window_out=infos,
                    new_grids=lambda: (wm.WindowedGrid(oracle, 3.0, 0.2), wm.WindowedGrid(oracle, 3.0, 0.4)))
    return est, maps, infos


def test_slam_step_tight_window_matches_the_windowed_oracle_loop(oracle):
    """40 scans of the room loop with a (2, 2, 1) window after every scan (most of the 60 x 40 m room is forgotten at once), pipelined
    and synchronous, against the oracle-driven loop on the windowed model cropped at the cell of each scan's pose_map."""
    n, window = 40, ((2, 2, 1), 1)
    world = synth.World(ground_half=45.0)
    truth = rp.trajectory(n)
    scans = [synth.make_scan(world, truth[k], synth.SEED + 5000 + k) for k in range(n)]
    est_o, maps_o, infos_o = _windowed_oracle_loop(oracle, world, truth, window)
    runs = {}
    for pipelined in (False, True):
        maps_g, infos_g = {}, []
        est_g, recs, _ = rp.run_slam(world, truth, pipelined=pipelined, scans=scans, maps_out=maps_g, map_window=window, window_out=infos_g)
        d = np.array([synth.pose_error(a, b) for a, b in zip(est_g, est_o)])
        assert d[:, 0].max() < 1e-6 and d[:, 1].max() < 1e-6, (pipelined, d.max(axis=0), int(d[:, 0].argmax()))
        for k in ("corner", "surf"):
            assert maps_g[k].shape == maps_o[k].shape, (k, maps_g[k].shape, maps_o[k].shape)
            assert np.abs(maps_g[k] - maps_o[k]).max() < 1e-4
        assert len(infos_g) == n
        for k in range(n):
            for side in (0, 1):
                assert infos_g[k][side].as_tuple() == infos_o[k][side].as_tuple(), (pipelined, k, side)
            assert tuple(recs[k].grid_corner[:2]) == (infos_g[k][0].n_points, infos_g[k][0].n_cells)         # the record reports the sizes after the crop
            assert tuple(recs[k].grid_surf[:2]) == (infos_g[k][1].n_points, infos_g[k][1].n_cells)
        assert all(r.status_extract == 0 and r.status_insert == 0 for r in recs)
        assert any(i[0].n_cells_evicted > 0 for i in infos_g) and any(i[1].n_cells_evicted > 0 for i in infos_g)
        runs[pipelined] = (est_g, _records(recs), [(i[0].as_tuple(), i[1].as_tuple()) for i in infos_g], maps_g)
    assert np.array_equal(runs[False][0], runs[True][0]) and runs[False][1] == runs[True][1] and runs[False][2] == runs[True][2]
    for k in ("corner", "surf"):
        assert np.array_equal(runs[False][3][k], runs[True][3][k])


def test_slam_step_wide_window_changes_nothing(oracle):
    """A window of 23 cells (the 60 m cut of GetSurroundedCloud + 1 m of probes + half a cell + one scan's motion) evicts nothing a
    registration could see -- in the room nothing at all: poses and records equal the run with the window off bit for bit, and so
    does a run that sets the window and turns it off again before the first scan.  (The synchronous form: there every field of the
    record, the stores' pool top included, is a function of the input alone.)"""
    n = 40
    world = synth.World(ground_half=45.0)
    truth = rp.trajectory(n)
    scans = [synth.make_scan(world, truth[k], synth.SEED + 5000 + k) for k in range(n)]
    maps_off, maps_on, maps_unset, infos = {}, {}, {}, []
    est_off, recs_off, _ = rp.run_slam(world, truth, pipelined=False, scans=scans, maps_out=maps_off)
    est_on, recs_on, _ = rp.run_slam(world, truth, pipelined=False, scans=scans, maps_out=maps_on, map_window=((23, 23, 23), 1), window_out=infos)

    def unset(slam, k):
        if k == 0:
            slam.set_map_window(None, 0)
    infos_unset = []
    est_unset, recs_unset, _ = rp.run_slam(world, truth, pipelined=False, scans=scans, maps_out=maps_unset, map_window=((2, 2, 1), 1), slam_hook=unset,
                                           window_out=infos_unset)
    for est, recs, maps in ((est_on, recs_on, maps_on), (est_unset, recs_unset, maps_unset)):
        assert np.array_equal(est, est_off)
        assert [bytes(r) for r in recs] == [bytes(r) for r in recs_off]
        for k in ("corner", "surf"):
            assert np.array_equal(maps[k], maps_off[k])
    assert all(i[side].applied == 1 and i[side].n_cells_evicted == 0 for i in infos for side in (0, 1))
    assert all((i[0].n_points, i[0].n_cells) == tuple(r.grid_corner[:2]) and (i[1].n_points, i[1].n_cells) == tuple(r.grid_surf[:2]) for i, r in zip(infos, recs_on))
    assert all(i[side].as_tuple() == (0, 0, 0, 0, (0, 0, 0), 0) for i in infos_unset for side in (0, 1))     # no crop ran: all-zero records


def test_cpp_mirror_crops_like_the_ctypes_binding(gpu, tmp_path):
    """HybridGrid::Crop and LaserSlam::SetMapWindow / MapWindow / ClearMapWindow (include/msfl/scan_matcher.hpp), compiled with
    plain g++ (tests/cpp/window_check.cpp), against the same calls through capi."""
    import struct
    import subprocess
    from msf_loam_amd import capi
    exe = str(tmp_path / "window_check")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "window_check.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "msf_loam_amd"), "-lmsfl_hip", "-Wl,-rpath," + os.path.join(ROOT, "msf_loam_amd")])
    bs = _batches()
    wp, centre, half = bs[0][1], np.array(bs[0][2][:3], np.float64), (2, 2, 1)
    n = 4
    world = synth.World(ground_half=45.0)
    truth = rp.trajectory(n)
    scans = [synth.make_scan(world, truth[k], synth.SEED + 5000 + k, n_az=600) for k in range(n)]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<ff", 3.0, 0.4)); f.write(centre.astype("<f8").tobytes()); f.write(struct.pack("<iii", *half))
        f.write(struct.pack("<i", len(wp))); f.write(np.ascontiguousarray(wp, "<f4").tobytes())
        f.write(struct.pack("<i", n))
        for pts, ring in scans:
            rec = np.zeros(len(pts), np.dtype([("p", "<f4", 4), ("ring", "<i4")]))
            rec["p"], rec["ring"] = pts, ring
            f.write(struct.pack("<i", len(pts))); f.write(rec.tobytes())
    subprocess.check_call([exe, str(fin), str(fout)])
    raw = open(fout, "rb").read()
    g = capi.Grid(gpu, 3.0, 0.4)
    g.insert_scan(wp)
    info, ev = g.crop(centre, half, keep_evicted=True)
    g.close()
    assert info.n_cells_evicted > 0
    assert raw[:32] == bytes(info) and struct.unpack("<i", raw[32:36])[0] == len(ev) and raw[36:36 + 16 * len(ev)] == ev.tobytes()
    raw = raw[36 + 16 * len(ev):]
    assert len(raw) == n * 64
    slam = capi.Slam(0, max_scan_points=max(len(p) for p, _ in scans), max_rings=int(max(r.max() for _, r in scans)) + 1)
    slam.set_map_window(half, 1)
    for k in range(n):
        if k == n - 1:
            slam.set_map_window(None)
        slam.add_scan(*scans[k])
        a, b = slam.get_map_window(k)
        assert raw[64 * k:64 * k + 64] == bytes(a) + bytes(b), k
        assert (a.applied, b.applied) == ((1, 1) if k < n - 1 else (0, 0))
    assert raw[64 * (n - 1):] == bytes(64)
    slam.close()
