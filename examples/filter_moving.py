#!/usr/bin/env python3
"""Keep what moves out of the map: msfl_grids_scan_novelty on the synthetic room of clean_map.py.

The sensor drives clean_map.py's loop while its 1 m box moves ahead of it.  The corner and the surf store are built at the true
poses exactly as clean_map.py's pass 1 builds them, three ways:

  unfiltered      every scan's features go in: the box leaves its trail of ghost points.
  feature_stores  from scan `--label-from` on, each scan is labelled against corner + surf (msfl_grids_scan_novelty) and the returns
                  IN_FRONT of the map are masked before the extraction.
  full_store      the same, labelled against a third store that holds the full clouds at a 0.4 m leaf (what passed the mask).

Printed as one JSON line, per variant: ghost points and stored points per store (ghosts as clean_map.is_ghost counts them), the
static returns the mask withheld, and the share of the box's returns labelled IN_FRONT.  A return counts as the box's when it lies
within 5 cm of the box's faces at that scan.  `prototype_cpu` repeats the figures of the numpy prototype this rule was chosen on
(atan2 pixels, the full clouds voxel-averaged at 0.4 m, the box never let into the map): an indication, not a result of this library.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from msf_loam_amd import synth  # noqa: E402
import clean_map as cm  # noqa: E402
import replay_synthetic as rp  # noqa: E402

PROTOTYPE_CPU = {"setting": "numpy, 60 scans, labels from scan 10, 720 x 16, atan2 pixels, full clouds at 0.4 m, box never in the map",
                 "rows": [{"window": [1, 1], "min_support": 1, "box_in_front_share": 0.94, "static_in_front_share": 0.016},
                          {"window": [2, 1], "min_support": 1, "box_in_front_share": 0.96, "static_in_front_share": 0.0039},
                          {"window": [2, 1], "min_support": 2, "box_in_front_share": 0.95, "static_in_front_share": 0.0038},
                          {"window": [3, 1], "min_support": 2, "box_in_front_share": 0.96, "static_in_front_share": 0.0020}]}


def on_box(world_pts, centre, grow=0.05):
    """Returns of the box: within `grow` of its faces (the range noise is 1 cm) and off the floor."""
    p = world_pts[:, :3].astype(np.float64)
    return (np.abs(p - centre) <= cm.BOX / 2 + grow).all(axis=1) & (p[:, 2] > 0.03)


def build(h, capi, scans, truth, centres, world, variant, cfg, label_from):
    """One variant's stores and counts.  variant: "unfiltered", "feature_stores" or "full_store"."""
    stores = {"corner": capi.Grid(h, 3.0, 0.2), "surf": capi.Grid(h, 3.0, 0.4)}
    full = capi.Grid(h, 3.0, 0.4) if variant == "full_store" else None
    n_box = n_box_front = n_static = n_static_front = 0
    for k, (pts, ring) in enumerate(scans):
        cloud = pts
        if variant != "unfiltered" and k >= label_from:
            against = [full] if full is not None else [stores["corner"], stores["surf"]]
            out = capi.grids_scan_novelty(against, pts, truth[k], cfg)
            front = out["cls"] == capi.NOV_IN_FRONT
            box = on_box(h.transform_cloud(pts, truth[k]), centres[k])
            n_box += int(box.sum()); n_box_front += int((box & front).sum())
            n_static += int((~box).sum()); n_static_front += int((~box & front).sum())
            cloud = out["masked"]
        if full is not None:
            kept = cloud[np.isfinite(cloud[:, 0])]
            full.insert_scan(h.transform_cloud(kept, truth[k]))
        f = h.extract_features(cloud, ring)
        for name, key in (("corner", "less_sharp"), ("surf", "less_flat")):
            c = h.voxel_downsample(f["full"][f[key]], stores[name].leaf)
            stores[name].insert_scan(h.transform_cloud(c, truth[k]))
    res = {"static_withheld": n_static_front, "static_returns": n_static, "box_returns": n_box, "box_in_front": n_box_front,
           "box_in_front_share": (n_box_front / n_box) if n_box else None}
    for name, g in stores.items():
        dump = g.dump()
        res[name] = {"ghosts": int(cm.is_ghost(dump, centres, world).sum()), "points": len(dump), "sha256": hashlib.sha256(dump.tobytes()).hexdigest()}
        g.close()
    if full is not None:
        res["full_points"] = full.size()[0]
        full.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=120)
    ap.add_argument("--label-from", type=int, default=10, help="first scan that is labelled; the scans before it seed the map")
    ap.add_argument("--window-col", type=int, default=None)
    ap.add_argument("--window-row", type=int, default=None)
    ap.add_argument("--min-support", type=int, default=None)
    a = ap.parse_args()
    from msf_loam_amd import capi
    kw = {k: v for k, v in (("window_col", a.window_col), ("window_row", a.window_row), ("min_support", a.min_support)) if v is not None}
    cfg = capi.novelty_config(**kw)
    world = synth.World(ground_half=45.0)
    truth = rp.trajectory(a.scans)
    centres = cm.box_centres(a.scans)
    scans = [cm.scan_with_box(world, truth[k], centres[k], synth.SEED + 7000 + k) for k in range(a.scans)]
    h = capi.Handle(0)
    out = {"scans": a.scans, "label_from": a.label_from,
           "config": dict({k: getattr(cfg.image, k) for k, _ in capi.CarveConfig._fields_}, min_support=cfg.min_support, keep_classes=cfg.keep_classes)}
    for variant in ("unfiltered", "feature_stores", "full_store"):
        out[variant] = build(h, capi, scans, truth, centres, world, variant, cfg, a.label_from)
    out["prototype_cpu"] = PROTOTYPE_CPU
    h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
