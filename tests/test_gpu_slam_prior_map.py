"""Localising in a saved map: a mapping session (the oracle-driven loop on the CPU, scans 0..19 of the room loop) leaves two stores;
their dump() + dump_cells(), written as map files, are loaded into a fresh device-resident SLAM session (msfl_grid_load_cells
through Slam.grids()) before its first scan, and scans 20..29 are fed.  Expected: the oracle-driven loop carried on over scans
20..29 with the same, already filled grids."""
import os
import sys

import numpy as np
import pytest

from msf_loam_amd import mapio, synth
from tests import windowed_grid_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
import replay_synthetic as rp  # noqa: E402

pytestmark = pytest.mark.gpu

N_MAP, N = 20, 30


def _records(recs):
    """The records as bytes, without the pool top of the two stores (when a store compacts follows from which reports the host had
    seen when it planned the insert: timing, in the pipelined form)."""
    from msf_loam_amd import capi
    out = []
    for r in recs:
        c = capi.SlamResult.from_buffer_copy(bytes(r))
        c.grid_corner[2] = c.grid_surf[2] = 0
        out.append(bytes(c))
    return out


def test_a_session_localises_in_a_loaded_map(oracle, tmp_path):
    from msf_loam_amd import capi
    from tests.test_gpu_replay import OracleBackendRigid3d
    world = synth.World(ground_half=45.0)
    truth = rp.trajectory(N)
    scans = [synth.make_scan(world, truth[k], synth.SEED + 5000 + k) for k in range(N)]
    # the mapping session, on the CPU
    grids = (wm.WindowedGrid(oracle, 3.0, 0.2), wm.WindowedGrid(oracle, 3.0, 0.4))              # never cropped: oracle.HybridGrid + the cell list
    rp.run(OracleBackendRigid3d(oracle), world, truth[:N_MAP], scans=scans[:N_MAP], new_grids=lambda: grids)
    prefix = str(tmp_path / "room")
    saved = {}
    for g, side, leaf in zip(grids, ("corner", "surf"), (0.2, 0.4)):
        saved[side] = (g.dump_cells(), g.dump())
        assert len(saved[side][0]) > 10
        mapio.write_map("%s.%s.npz" % (prefix, side), 3.0, leaf, *saved[side])
    # expected: the same loop carried on in the same grids
    maps_o = {}
    est_o, _ = rp.run(OracleBackendRigid3d(oracle), world, truth[N_MAP:], scans=scans[N_MAP:], new_grids=lambda: grids, maps_out=maps_o)
    runs = {}
    for pipelined in (False, True):
        maps_g, seen = {}, {}

        def look(slam, k):
            if k == 0:                                                  # the stores hold the saved map before the first scan, bit for bit
                for g, side in zip(slam.grids(), ("corner", "surf")):
                    seen[side] = (g.dump_cells(), g.dump())
        est_g, recs, _ = rp.run_slam(world, truth[N_MAP:], pipelined=pipelined, scans=scans[N_MAP:], maps_out=maps_g, load_map=prefix, slam_hook=look)
        for side in ("corner", "surf"):
            assert np.array_equal(seen[side][0], saved[side][0]) and np.array_equal(seen[side][1], saved[side][1]), side
        r0 = recs[0]
        assert r0.status_mapping == 0 and r0.n_map_corner > 10 and r0.n_map_surf > 50 and sum(r0.mapping.lm_iterations) > 0
        assert r0.status_mapping != capi.MAP_TOO_SMALL                   # what scan 0 reports without the load
        assert all(r.status_extract == 0 and r.status_insert == 0 and r.status_mapping == 0 for r in recs)
        d = np.array([synth.pose_error(a, b) for a, b in zip(est_g, est_o)])
        print("pipelined", pipelined, "max pose difference (m, rad)", d.max(axis=0))
        assert d[:, 0].max() < 1e-6 and d[:, 1].max() < 1e-6, (pipelined, d.max(axis=0), int(d[:, 0].argmax()))
        for k in ("corner", "surf"):
            assert maps_g[k].shape == maps_o[k].shape, (k, maps_g[k].shape, maps_o[k].shape)
            assert np.abs(maps_g[k] - maps_o[k]).max() < 1e-4
            assert len(maps_g[k]) > len(saved[k][1])
        runs[pipelined] = (est_g, _records(recs), maps_g)
    assert np.array_equal(runs[False][0], runs[True][0]) and runs[False][1] == runs[True][1]
    for k in ("corner", "surf"):
        assert np.array_equal(runs[False][2][k], runs[True][2][k])
