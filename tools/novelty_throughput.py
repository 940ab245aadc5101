#!/usr/bin/env python3
"""Time per call of msfl_grid_render, msfl_scan_novelty and msfl_grids_scan_novelty next to msfl_grid_carve and
msfl_grid_insert_scan on the same stores and scan, in one session (a sibling of carve_cost.py).

Two shapes:
  track    carve_cost.py's store: about --map-points points grown from grid_scaling.py's translating scans, once at a 0.2 m leaf
           ("corner") and once at 0.4 m ("surf"); the scan is one 16 x 1 800 sweep of the synthetic room.
  outdoor  the outdoor world's sampled map (synth.make_map: corner and surf clouds) in the same two stores, the scan one sweep of
           that world at one of its poses.
Everything is resident on the device (scan, pose, image, outputs; info = NULL for the three new calls, so they only enqueue).  HIP
events on the handle's stream bracket --reps calls after --warmup calls; the figure is the bracket divided by the calls.  The carve
and the insert wait for their report inside every call, so their figures hold that wait; the new calls are also timed with info read
back, which makes them wait the same way.  Writes one JSON line, and --out (default profiles/novelty_throughput.json).
"""
import argparse, ctypes as C, gc, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from msf_loam_amd import capi, synth
from grid_scaling import scan_at


def _bracket(torch, stream, fn, warmup, reps):
    """ms per call: HIP events on `stream` round `reps` calls after `warmup` calls."""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return round(a.elapsed_time(b) / reps, 5)


def shape(torch, h, stream, name, corner_pts, surf_pts, scan, pose, a):
    dev = "cuda:0"
    stores = {"corner": capi.Grid(h, 3.0, 0.2), "surf": capi.Grid(h, 3.0, 0.4)}
    for g, pts in ((stores["corner"], corner_pts), (stores["surf"], surf_pts)):
        for i in range(0, len(pts), 6000):
            g.insert_scan(pts[i:i + 6000])
    cfg = capi.novelty_config()
    n = len(scan)
    d_scan = torch.from_numpy(np.ascontiguousarray(scan)).to(dev)
    d_pose = torch.from_numpy(np.ascontiguousarray(pose, np.float64)).to(dev)
    d_img = torch.zeros((cfg.image.n_row, cfg.image.n_col), dtype=torch.float32, device=dev)
    d_cls = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_masked = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    extra = scan_at(np.random.default_rng(1), 0, 6000)[0]
    extra[:, :3] += np.asarray(pose[:3], np.float32) - extra[:, :3].mean(axis=0)
    d_extra = torch.from_numpy(extra).to(dev)
    torch.cuda.synchronize()
    both = [stores["corner"], stores["surf"]]
    t = lambda fn: _bracket(torch, stream, fn, a.warmup, a.reps)
    res = {"store_points": {k: g.size()[0] for k, g in stores.items()}, "store_cells": {k: g.size()[1] for k, g in stores.items()}, "scan_points": n}
    for k, g in stores.items():
        res["render_" + k] = t(lambda: g.render_device(d_pose, cfg.image, d_img))
        res["render_" + k + "_with_info"] = t(lambda: g.render_device(d_pose, cfg.image, d_img, want_info=True))
        res["tested_" + k] = g.render_device(d_pose, cfg.image, d_img, want_info=True).n_tested
    stores["corner"].render_device(d_pose, cfg.image, d_img)
    stores["surf"].render_device(d_pose, cfg.image, d_img, accumulate=True)
    res["scan_novelty"] = t(lambda: h.scan_novelty_device(d_scan, n, d_img, cfg, d_cls, d_masked))
    res["scan_novelty_with_info"] = t(lambda: h.scan_novelty_device(d_scan, n, d_img, cfg, d_cls, d_masked, want_info=True))
    res["composite"] = t(lambda: capi.grids_scan_novelty_device(both, d_scan, n, d_pose, cfg, d_cls, d_masked))
    res["composite_with_info"] = t(lambda: capi.grids_scan_novelty_device(both, d_scan, n, d_pose, cfg, d_cls, d_masked, want_info=True))
    info = capi.grids_scan_novelty_device(both, d_scan, n, d_pose, cfg, d_cls, d_masked, want_info=True)
    res["classes"] = dict(zip(capi.NOV_CLASS_NAMES, info.n_class)); res["map_pixels"] = info.n_map_pixels
    # the yardsticks, on the same stores and scan (both wait for their report inside the call)
    for k, g in stores.items():
        res["carve_" + k] = t(lambda: g.carve_device(d_scan, n, d_pose, cfg.image))
        res["insert_6000_" + k] = t(lambda: g.lib.msfl_grid_insert_scan(g.g, capi._vp(d_extra), len(extra), capi.MEM_DEVICE))
    for g in both:
        g.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-points", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "novelty_throughput.json"))
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda:0")
    stream = torch.cuda.Stream()
    h = capi.Handle()
    h.set_stream(stream.cuda_stream)
    gc.collect(); gc.disable()
    res = {"reps": a.reps, "warmup": a.warmup, "unit": "ms per call"}
    # track: the carve's store
    rng = np.random.default_rng(7)
    pts = np.concatenate([scan_at(rng, k, 6000)[0] for k in range(max(a.map_points // 5500, 1))])
    room = synth.World(ground_half=45.0)
    k_mid = max(a.map_points // 5500, 1) // 2
    c = scan_at(np.random.default_rng(0), k_mid, 1)[1]
    scan, _ = synth.make_scan(room, np.array([0, 0, 1.8, 0, 0, 0, 1.0]), synth.SEED + 1)
    res["track"] = shape(torch, h, stream, "track", pts, pts, scan, np.array([c[0], c[1], 1.8, 0, 0, 0, 1.0]), a)
    # outdoor: the sampled map of the outdoor world
    out = synth.World(kind="outdoor")
    mc, ms = synth.make_map(out)
    pose = synth.world_poses(out, 1)[0]
    scan, _ = synth.make_scan(out, pose, synth.SEED + 2)
    res["outdoor"] = shape(torch, h, stream, "outdoor", mc, ms, scan, pose, a)
    h.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
