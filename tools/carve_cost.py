#!/usr/bin/env python3
"""Cost of one msfl_grid_carve call next to msfl_grid_insert_scan and msfl_grid_crop, in one session (a sibling of grid_scaling.py).

A store of about --map-points points is grown from grid_scaling.py's translating scans (6 000 points each: ground and two
walls).  Then, alternating, at positions spread along the track:
  * carve   one 16 x 1 800 scan of the synthetic room (28.8 k rays, ~27 k returns), default configuration, through the host API
            (wall clock round the call: the copy of the scan, the launches, the wait for the report), once with the scan in host
            memory and once with scan and pose resident on the device;
  * insert  one 6 000-point scan_at cloud, host memory;
  * crop    a window that keeps every cell (three launches and the report).
Prints one JSON line: median, 10th and 90th percentile in ms of each, the store's size and what the carves removed.
"""
import argparse, gc, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from msf_loam_amd import capi, synth
from grid_scaling import scan_at, _spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=60)
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda:0")
    h = capi.Handle()
    g = capi.Grid(h, 3.0, 0.2)
    rng = np.random.default_rng(7)
    k = 0
    while g.size()[0] < a.map_points:
        g.insert_scan(scan_at(rng, k, 6000)[0]); k += 1
    n_scans = k
    size0 = g.size()
    world = synth.World(ground_half=45.0)
    scan, _ = synth.make_scan(world, np.array([0, 0, 1.8, 0, 0, 0, 1.0]), synth.SEED + 1)
    d_scan = torch.from_numpy(np.ascontiguousarray(scan)).to("cuda:0")
    d_pose = torch.zeros(7, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    t = {"carve_host": [], "carve_device": [], "insert": [], "crop": []}
    removed, tested = [], []
    gc.collect(); gc.disable()
    for i in range(a.reps + 4):
        kk = (i * 7919) % n_scans
        c = scan_at(np.random.default_rng(i), kk, 1)[1]
        pose = np.array([c[0], c[1], 1.8, 0, 0, 0, 1.0])
        d_pose.copy_(torch.from_numpy(pose)); torch.cuda.synchronize()
        t0 = time.perf_counter(); info, _ = g.carve(scan, pose); t1 = time.perf_counter()
        info_d = g.carve_device(d_scan, len(scan), d_pose); t2 = time.perf_counter()
        p = scan_at(rng, kk, 6000)[0]
        t3 = time.perf_counter(); g.insert_scan(p); t4 = time.perf_counter()
        g.crop(c, (8000, 8000, 8000)); t5 = time.perf_counter()
        if i >= 4:                                                       # the first calls allocate
            t["carve_host"].append(t1 - t0); t["carve_device"].append(t2 - t1); t["insert"].append(t4 - t3); t["crop"].append(t5 - t4)
            removed.append(info.n_points_removed); tested.append(info.n_tested)
        assert info_d.n_points_removed == 0 or info_d.applied == 1
    print(json.dumps({"scan_points": len(scan), "store_points": size0[0], "store_cells": size0[1], "store_points_end": g.size()[0],
                      "removed_per_carve_median": float(np.median(removed)), "tested_per_carve_median": float(np.median(tested)),
                      **{name: _spread(v) for name, v in t.items()}}), flush=True)
    g.close(); h.close()


if __name__ == "__main__":
    main()
