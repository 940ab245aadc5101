"""Throughput of msfl_score_poses_batch / msfl_score_poses at the bench shape, against the 5-NN launch of the same session.
    python tools/score_throughput.py [--scans 1024] [--map-points 200000] [--reloc 100000] [--features product|direct]

  bench shape     the bench batch (--scans scans of ~5 k features, one hypothesis each = --scans hypotheses) against the
                  200 k-point map, at max_dist 1.0 and 0.3, poses = the batch's perturbed guesses (what the matcher's first
                  association pass sees) and = the true poses
  reloc shape     one scan x --reloc hypotheses (a position x yaw lattice round the truth), max_dist 1.0
  yardstick       the 5-NN launch of bench.py's step (msfl_set_map + msfl_match_scan2map_batch) in this process:
                  msfl_get_timing ms_assoc / launches_assoc, per query (every launch visits all features of the batch)

Times are HIP events on the handle's stream round back-to-back calls (the records' init launch and the offset upload
included), after a warm-up of 20 steps / calls for the clock ramp.  One JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from msf_loam_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--scans", type=int, default=1024)
ap.add_argument("--map-points", type=int, default=200000)
ap.add_argument("--reloc", type=int, default=100000)
ap.add_argument("--features", choices=["product", "direct"], default="product")
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--reps", type=int, default=50)
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("score_throughput.py needs a GPU (no CPU fallback)")
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
h = capi.Handle(0)
inp = bench.build_inputs(args.scans, args.map_points, 0, bench.product_extractor(h) if args.features == "product" else None)
B = len(inp["guesses"])
co, so = inp["corner_off"], inp["surf_off"]
n_feat = int(co[-1] + so[-1])
stream = torch.cuda.current_stream(dev)
h.set_stream(stream.cuda_stream)
d = {k: torch.from_numpy(np.ascontiguousarray(inp[k])).to(dev) for k in ("map_corner", "map_surf", "corner", "surf", "guesses", "truth")}
n_mc, n_ms = len(inp["map_corner"]), len(inp["map_surf"])
d_poses = torch.zeros((B, 7), dtype=torch.float64, device=dev)
d_status = torch.zeros(B, dtype=torch.int32, device=dev)
po = np.arange(B + 1, dtype=np.int32)


def step():
    d_poses.copy_(d["guesses"])
    h.set_map(d["map_corner"], d["map_surf"], n_mc, n_ms, capi.MEM_DEVICE)
    h.match_scan2map_batch_device(B, d["corner"], co, d["surf"], so, d_poses, d_status)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.warmup):
        fn()
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / reps


def knn_yardstick():
    h.set_timing(2)
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize(dev)
    h.get_timing(reset=True)
    for _ in range(args.reps):
        step()
    torch.cuda.synchronize(dev)
    t = h.get_timing(reset=True)
    h.set_timing(0)
    first = (t.ms_assoc - t.ms_assoc_seeded) / max(t.launches_assoc - t.launches_assoc_seeded, 1)
    return {"ms_per_launch": t.ms_assoc / t.launches_assoc, "ms_per_launch_first_pass": first,
            "ms_per_launch_second_pass": t.ms_assoc_seeded / max(t.launches_assoc_seeded, 1), "launches": t.launches_assoc,
            "ns_per_query": 1e6 * t.ms_assoc / t.launches_assoc / n_feat, "ns_per_query_first_pass": 1e6 * first / n_feat}


out = {"scans": B, "features": n_feat, "features_per_scan": n_feat / max(B, 1), "map_points": n_mc + n_ms, "feature_source": args.features}
out["knn5"] = knn_yardstick()
h.set_map(d["map_corner"], d["map_surf"], n_mc, n_ms, capi.MEM_DEVICE)
d_scores = torch.zeros(B * capi.POSE_SCORE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
out["score_bench_shape"] = {}
for name in ("guesses", "truth"):
    for max_dist in (1.0, 0.3):
        ms = timed(lambda: h.score_poses_batch_device(B, d["corner"], co, d["surf"], so, d[name], po, max_dist, d_scores), args.reps)
        rec = d_scores.cpu().numpy().view(capi.POSE_SCORE_DTYPE)
        out["score_bench_shape"]["%s_%.1f" % (name, max_dist)] = {
            "ms_per_call": ms, "ns_per_query": 1e6 * ms / n_feat, "ratio_to_knn5_launch": ms / out["knn5"]["ms_per_launch"],
            "ratio_to_knn5_first_pass": ms / out["knn5"]["ms_per_launch_first_pass"],
            "mean_fitness": float(rec["inliers"].sum() / n_feat)}
out["knn5_again"] = knn_yardstick()          # the yardstick once more after the scoring calls: the spread of the session

if args.reloc > 0:
    c0, s0, truth = inp["corner"][co[0]:co[1]], inp["surf"][so[0]:so[1]], inp["truth"][0]
    n_yaw = 40
    side = int(np.ceil(np.sqrt(args.reloc / n_yaw)))
    g = (np.arange(side) - side // 2) * 0.4
    hyp = []
    for j in range(n_yaw):
        a = np.pi * j / n_yaw
        q = synth.quat_mul(np.array([0.0, 0.0, np.sin(a), np.cos(a)]), truth[3:])
        X, Y = np.meshgrid(g, g, indexing="ij")
        block = np.tile(np.r_[truth[:3], q / np.linalg.norm(q)], (side * side, 1))
        block[:, 0] += X.ravel(); block[:, 1] += Y.ravel()
        hyp.append(block)
    hyp = np.concatenate(hyp)[:args.reloc]
    H, F1 = len(hyp), len(c0) + len(s0)
    d_c0, d_s0, d_h = torch.from_numpy(c0).to(dev), torch.from_numpy(s0).to(dev), torch.from_numpy(hyp).to(dev)
    d_sc = torch.zeros(H * capi.POSE_SCORE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    ms = timed(lambda: h.score_poses_device(d_c0, len(c0), d_s0, len(s0), d_h, H, 1.0, d_sc), 5)
    rec = d_sc.cpu().numpy().view(capi.POSE_SCORE_DTYPE)
    fit = capi.fitness(rec, len(c0), len(s0))
    out["score_reloc_shape"] = {"hypotheses": H, "features": F1, "ms_per_call": ms, "ns_per_query": 1e6 * ms / (H * F1),
                                "hypotheses_per_s": H / (1e-3 * ms), "ratio_to_knn5_query": 1e6 * ms / (H * F1) / out["knn5"]["ns_per_query"],
                                "best_is_truth": bool(np.argmax(fit) == int(np.argmin(np.abs(hyp[:, :3] - truth[:3]).sum(1) + np.abs(hyp[:, 3:] - truth[3:]).sum(1)))),
                                "best_fitness": float(fit.max()), "median_fitness": float(np.median(fit))}
h.close()
print(json.dumps(out))
