#!/usr/bin/env python3
"""Cost of msfl_segment_scans next to the feature extraction on the same clouds, in one process.

  * batch : --scans (1 024) sweeps of the 16-beam synthetic sensor in the outdoor world (--distinct different sweeps, repeated), resident
            on the device, one msfl_segment_scans call without `info` (stream-ordered; the wall clock runs to msfl_synchronize);
  * sweep : one 64 x 2 048 image in one scan of about 120 k points, device memory, and the same through host arrays with `info`;
  * yardstick : msfl_extract_features_batch on the same device clouds.
Prints one JSON line (median, 10th and 90th percentile in ms) and writes it to --out (default profiles/segment_cost.json).
"""
import argparse
import ctypes as C
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from msf_loam_amd import capi, synth


def _spread(v):
    v = 1e3 * np.asarray(v)
    return {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90))}


def _timed(fn, sync, reps):
    out = []
    for i in range(reps + 3):
        sync()
        t0 = time.perf_counter(); fn(); sync(); t1 = time.perf_counter()
        if i >= 3:                                                       # the first calls allocate
            out.append(t1 - t0)
    return _spread(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_cost.json"))
    a = ap.parse_args()
    import torch
    import segment_cases as sc
    torch.zeros(1, device="cuda:0")
    h = capi.Handle(0)
    world = synth.World(kind="outdoor")
    poses = synth.world_poses(world, a.distinct)
    sweeps = [synth.make_scan(world, poses[k], synth.SEED + 600 + k) for k in range(a.distinct)]
    pts = np.concatenate([sweeps[b % a.distinct][0] for b in range(a.scans)])
    ring = np.concatenate([sweeps[b % a.distinct][1] for b in range(a.scans)])
    off = np.concatenate([[0], np.cumsum([len(sweeps[b % a.distinct][0]) for b in range(a.scans)])]).astype(np.int32)
    n = len(pts)
    dev = "cuda:0"
    d_pts, d_ring = torch.from_numpy(pts).to(dev), torch.from_numpy(ring.view(np.int16)).to(dev)
    d_cls = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_seg = torch.zeros(n, dtype=torch.int32, device=dev)
    d_masked = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    cfg = capi.SegmentConfig()
    gc.collect(); gc.disable()
    res = {"scans": a.scans, "points": int(n), "distinct_sweeps": a.distinct}
    res["segment_batch"] = _timed(lambda: h.segment_scans_device(d_pts, d_ring, off, cfg, d_cls, d_seg, d_masked), h.synchronize, a.reps)
    res["segment_batch_classes_only"] = _timed(lambda: h.segment_scans_device(d_pts, d_ring, off, cfg, d_cls), h.synchronize, a.reps)
    info = np.zeros(a.scans, capi.SEGMENT_INFO_DTYPE)
    h.segment_scans_device(d_pts, d_ring, off, cfg, d_cls, d_seg, d_masked, info)
    res["class_fractions"] = {name: float(info["n_class"][:, c].sum() / n) for c, name in enumerate(capi.SEG_CLASS_NAMES)}

    # the yardstick: extraction of the same resident clouds
    o = {k: torch.zeros(n, dtype=dt, device=dev) for k, dt in (("ring", torch.int16), ("curvature", torch.float32), ("label", torch.uint8), ("sharp", torch.int32),
                                                               ("less_sharp", torch.int32), ("flat", torch.int32), ("less_flat", torch.int32))}
    o["full"] = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    cnt = torch.zeros((5, a.scans), dtype=torch.int32, device=dev)
    status = torch.zeros(a.scans, dtype=torch.int32, device=dev)
    f = capi.FeaturesBatch()
    f.full_pts, f.full_ring, f.curvature, f.label = (o[k].data_ptr() for k in ("full", "ring", "curvature", "label"))
    f.sharp_idx, f.less_sharp_idx, f.flat_idx, f.less_flat_idx = (o[k].data_ptr() for k in ("sharp", "less_sharp", "flat", "less_flat"))
    f.n_full, f.n_sharp, f.n_less_sharp, f.n_flat, f.n_less_flat = (cnt[k].data_ptr() for k in range(5))

    def extract(src):
        s = h.lib.msfl_extract_features_batch(h.h, a.scans, capi._vp(src), capi._vp(d_ring), capi._vp(off), C.byref(f), capi._vp(status), capi.MEM_DEVICE)
        assert s == capi.OK, s
    res["extract_batch_raw"] = _timed(lambda: extract(d_pts), h.synchronize, a.reps)
    res["extract_batch_masked"] = _timed(lambda: extract(d_masked), h.synchronize, a.reps)

    big_pts, big_ring, big_cfg = sc.random_image(164, 64, 2048)
    c_big = capi.SegmentConfig(**vars(big_cfg))
    b_pts, b_ring = torch.from_numpy(big_pts).to(dev), torch.from_numpy(big_ring.view(np.int16)).to(dev)
    m = len(big_pts)
    b_off = np.array([0, m], np.int32)
    torch.cuda.synchronize()
    res["sweep_64x2048_points"] = int(m)
    res["segment_sweep_64x2048_device"] = _timed(lambda: h.segment_scans_device(b_pts, b_ring, b_off, c_big, d_cls, d_seg, d_masked), h.synchronize, a.reps)
    res["segment_sweep_64x2048_host_with_info"] = _timed(lambda: h.segment_scans(big_pts, big_ring, b_off, c_big), lambda: None, a.reps)
    res["segment_sweep_16x1800_device"] = _timed(lambda: h.segment_scans_device(d_pts, d_ring, off[:2], cfg, d_cls, d_seg, d_masked), h.synchronize, a.reps)
    h.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
