#!/usr/bin/env python3
"""Scan segmentation on one outdoor sweep (msfl_segment_scan, docs/kernels/segment.md).

About a fifth of an outdoor sweep comes back from inside canopy and bushes.  The segmentation lays the sweep into its range image,
takes the ground out by the slope between neighbouring beams, clusters the rest and drops the clusters too small to be a surface.
This example prints
  * the class of every return against what it really hit (synth.make_scan(with_kind=True): ground, wall, pole, volume);
  * feature extraction and msfl_match_scan2map on the raw cloud and on the masked cloud: feature counts, the error of the
    registered pose against the true one, milliseconds per call.
--json: one JSON line with the same figures at the end.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from msf_loam_amd import capi, synth  # noqa: E402

KINDS = ("ground", "wall", "pole", "volume")


def register(h, pts, ring, guess, truth, reps):
    """Extraction, voxel filter and scan-to-map of one cloud: counts, pose error, ms per extraction and per registration."""
    f = h.extract_features(pts, ring)
    corner = h.voxel_downsample(f["full"][f["less_sharp"]], 0.2)
    surf = h.voxel_downsample(f["full"][f["less_flat"]], 0.4)
    s, pose, info = h.match_scan2map(corner, surf, guess)
    t0 = time.perf_counter()
    for _ in range(reps):
        h.extract_features(pts, ring)
    t1 = time.perf_counter()
    for _ in range(reps):
        h.match_scan2map(corner, surf, guess)
    t2 = time.perf_counter()
    dt, dr = synth.pose_error(pose, truth)
    return dict(n_full=len(f["full"]), n_sharp=len(f["sharp"]), n_less_sharp=len(f["less_sharp"]), n_flat=len(f["flat"]), n_less_flat=len(f["less_flat"]),
                n_corner_ds=len(corner), n_surf_ds=len(surf), status=int(s), n_edge=list(info.n_edge), n_plane=list(info.n_plane),
                error_m=float(dt), error_deg=float(np.rad2deg(dr)), extract_ms=1e3 * (t1 - t0) / reps, match_ms=1e3 * (t2 - t1) / reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", choices=["room", "outdoor"], default="outdoor")
    ap.add_argument("--pose", type=int, default=0, help="which of the world's own poses the sweep is taken from")
    ap.add_argument("--reps", type=int, default=5, help="timed repetitions of every call")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    world = synth.World(kind="outdoor") if a.world == "outdoor" else synth.World(ground_half=45.0)
    truth = synth.world_poses(world, a.pose + 1)[a.pose]
    pts, ring, kind = synth.make_scan(world, truth, synth.SEED + 77, with_kind=True)
    mc, ms = synth.make_map(world)
    guess = synth.perturb_pose(truth, np.random.default_rng(5))
    h = capi.Handle(0)
    out = h.segment_scan(pts, ring)
    t0 = time.perf_counter()
    for _ in range(a.reps):
        h.segment_scan(pts, ring)
    seg_ms = 1e3 * (time.perf_counter() - t0) / a.reps
    cls, info = out["cls"], out["info"]
    by_kind = {KINDS[k]: {name: int(np.sum(cls[kind == k] == c)) for c, name in enumerate(capi.SEG_CLASS_NAMES)} for k in range(4)}
    counts = {name: int(info["n_class"][c]) for c, name in enumerate(capi.SEG_CLASS_NAMES)}
    print("%d returns, %d pixels, %d components, %d segments, %d kept; %.3f ms per msfl_segment_scan (host arrays)"
          % (len(pts), info["n_pixels"], info["n_components"], info["n_segments"], info["n_kept"], seg_ms))
    print("%-8s" % "hit" + "".join("%10s" % n for n in capi.SEG_CLASS_NAMES))
    for k in KINDS:
        print("%-8s" % k + "".join("%10d" % by_kind[k][n] for n in capi.SEG_CLASS_NAMES))
    h.set_map(mc, ms)
    raw = register(h, pts, ring, guess, truth, a.reps)
    masked = register(h, out["masked"], ring, guess, truth, a.reps)
    for name, r in (("raw", raw), ("masked", masked)):
        print("%-7s features %d sharp / %d less sharp / %d flat / %d less flat, %d + %d after the voxel filter; pose error %.4f m %.3f deg; "
              "extraction %.3f ms, scan-to-map %.3f ms" % (name, r["n_sharp"], r["n_less_sharp"], r["n_flat"], r["n_less_flat"], r["n_corner_ds"],
                                                          r["n_surf_ds"], r["error_m"], r["error_deg"], r["extract_ms"], r["match_ms"]))
    h.close()
    if a.json:
        print(json.dumps({"world": a.world, "n_points": len(pts), "class_counts": counts, "by_kind": by_kind, "segment_ms": seg_ms,
                          "n_pixels": int(info["n_pixels"]), "n_components": int(info["n_components"]), "n_segments": int(info["n_segments"]),
                          "raw": raw, "masked": masked}))


if __name__ == "__main__":
    main()
