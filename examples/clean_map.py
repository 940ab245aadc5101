#!/usr/bin/env python3
"""Clean a map of what moved: msfl_grid_carve on the synthetic room.

A sensor drives the loop of replay_synthetic.py through the room while a 1 m box moves along an inner loop ahead of it.  A ray
that hits the box (a slab test in numpy) returns the box instead of the floor, wall or pole behind it.

  pass 1  builds the corner and the surf store from the scans' features at the true poses, exactly as the mapping loop files
          them (less-sharp points at a 0.2 m leaf, less-flat points at 0.4 m): the box leaves a trail of ghost points, one box
          per scan.
  pass 2  carves both stores with every k-th FULL scan at its true pose (the full cloud is the evidence: a feature list is
          too sparse to see through anything).

Printed: the ghost points -- stored points inside any position the box took, above the floor and off every pole -- before and
after, and the static points the carves took with them.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from msf_loam_amd import synth  # noqa: E402
import replay_synthetic as rp  # noqa: E402

BOX = 1.0          # edge of the box, metres; it stands on the floor


def box_centres(n):
    """The box's centre per scan: an inner loop, 0.7 rad ahead of the sensor."""
    a = 2 * np.pi * np.arange(n) / max(n, 120) + 0.7
    return np.stack([5.0 * np.cos(a), 3.0 * np.sin(a), np.full(n, BOX / 2)], axis=1)


def scan_with_box(world, pose, centre, seed, noise=0.01):
    """synth.make_scan with the box in the way: (points (n, 4) f32 in the sensor frame, ring ids)."""
    rng = np.random.default_rng(seed)
    dirs, ring = synth.beam_dirs()
    R = synth.quat_to_matrix(np.asarray(pose[3:], np.float64))
    rng_m, kind = synth.raycast(world, R, pose[:3], dirs, rng)
    d, o = dirs @ R.T, np.asarray(pose[:3], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (centre - BOX / 2 - o) / d, (centre + BOX / 2 - o) / d
        near, far = np.minimum(t0, t1).max(axis=1), np.maximum(t0, t1).min(axis=1)
    hit = (near <= far) & (near > 0) & (near < rng_m)
    rng_m = np.where(hit, near, rng_m)
    kind = np.where(hit, 4, kind)
    rng_m = rng_m + rng.normal(0, noise, rng_m.shape)
    ok = np.isfinite(rng_m) & (rng_m >= 0.3) & (rng_m <= 100.0) & (kind >= 0)
    pts = np.zeros((int(ok.sum()), 4), np.float32)
    pts[:, :3] = (dirs[ok] * rng_m[ok, None]).astype(np.float32)
    return pts, ring[ok].copy()


def is_ghost(pts, centres, world, grow=0.1):
    """Stored points inside any position of the box (grown by `grow`), above the floor and off every pole."""
    p = pts[:, :3].astype(np.float64)
    inside = np.zeros(len(p), bool)
    for c in centres:
        inside |= (np.abs(p - c) <= BOX / 2 + grow).all(axis=1)
    off_pole = np.ones(len(p), bool)
    for px, py in world.poles:
        off_pole &= np.hypot(p[:, 0] - px, p[:, 1] - py) > synth.POLE_R + 0.2
    return inside & (p[:, 2] > 0.1) & off_pole


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=120)
    ap.add_argument("--every", type=int, default=5, help="carve with every k-th scan")
    ap.add_argument("--margin-abs", type=float, default=None)
    ap.add_argument("--margin-rel", type=float, default=None)
    ap.add_argument("--window-col", type=int, default=None)
    ap.add_argument("--window-row", type=int, default=None)
    a = ap.parse_args()
    from msf_loam_amd import capi
    kw = {k: v for k, v in (("margin_abs", a.margin_abs), ("margin_rel", a.margin_rel), ("window_col", a.window_col), ("window_row", a.window_row))
          if v is not None}
    cfg = capi.carve_config(**kw)
    world = synth.World(ground_half=45.0)
    truth = rp.trajectory(a.scans)
    centres = box_centres(a.scans)
    h = capi.Handle(0)
    stores = {"corner": capi.Grid(h, 3.0, 0.2), "surf": capi.Grid(h, 3.0, 0.4)}
    scans = []
    for k in range(a.scans):                                                         # pass 1
        pts, ring = scan_with_box(world, truth[k], centres[k], synth.SEED + 7000 + k)
        scans.append(pts)
        f = h.extract_features(pts, ring)
        for name, key in (("corner", "less_sharp"), ("surf", "less_flat")):
            cloud = h.voxel_downsample(f["full"][f[key]], stores[name].leaf)
            stores[name].insert_scan(h.transform_cloud(cloud, truth[k]))
    out = {"scans": a.scans, "carve_every": a.every,
           "config": {k: getattr(cfg, k) for k, _ in capi.CarveConfig._fields_}}
    for name, g in stores.items():
        before = g.dump()
        ghosts_before = int(is_ghost(before, centres, world).sum())
        static_lost = removed = 0
        for k in range(0, a.scans, a.every):                                         # pass 2
            info, gone = g.carve(scans[k], truth[k], cfg, keep_removed=True)
            removed += info.n_points_removed
            static_lost += int((~is_ghost(gone, centres, world)).sum())
        after = g.dump()
        out[name] = {"points_before": len(before), "ghosts_before": ghosts_before, "points_after": len(after),
                     "ghosts_after": int(is_ghost(after, centres, world).sum()), "removed": removed, "static_lost": static_lost}
        g.close()
    h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
