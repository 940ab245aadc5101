"""Throughput and quality of msfl_search_poses, against msfl_score_poses on the same poses in the same session.
    python tools/search_throughput.py [--map-points 200000] [--warmup 20] [--reps 50] [--no-quality] [--only-search N]

  reloc shape   one scan of the bench batch (~5 k product features) against the 200 k-point map; lattice 51 x 49 positions x 40
                yaws = 99 960 hypotheses at pitch 0.4 m round the truth (an odd lattice: 2 half + 1 per axis, so the 50 x 50 x 40
                of tools/score_throughput.py is not one), yaw step pi / 40 as there
  yardstick     msfl_score_poses(max_dist 1.0) on exactly those 99 960 poses, device-resident
  variants      the same lattice with half[2] = 2 (5 x as many hypotheses), and on the outdoor world's map and scan
  split         the search with one stage's work removed is not a public call, so the per-stage split comes from a kernel trace
                of `--only-search N` (N back-to-back calls and nothing else); docs/kernels/search.md says how
  quality       room, outdoor, corridor at the fixture shape (pitch 0.5, 24 yaws, 9 x 9, guess (1.2, -0.9) m and 34 degrees off):
                the rank in the coarse order of the hypothesis msfl_score_poses ranks first, and how many of 16 candidates the
                matcher brings to the pose it reaches from the truth itself (within 1 cm and 0.1 degree)

Times are HIP events on the handle's stream round back-to-back calls after a warm-up.  One JSON line."""
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
ap.add_argument("--map-points", type=int, default=200000)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--no-quality", action="store_true")
ap.add_argument("--only-search", type=int, default=0, help="run N calls of the reloc shape and nothing else (for a kernel trace)")
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("search_throughput.py needs a GPU (no CPU fallback)")
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
h = capi.Handle(0)
inp = bench.build_inputs(8, args.map_points, 0, bench.product_extractor(h))
stream = torch.cuda.current_stream(dev)
h.set_stream(stream.cuda_stream)


def timed(fn, reps, warmup):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warmup):
        fn()
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / reps


def lattice_poses(guess, cfg):
    """pose(a, k) of every hypothesis in index order (include/msfl_c_api.h)."""
    n = [2 * x + 1 for x in cfg.half]
    out = np.zeros((cfg.n_yaw, n[2], n[1], n[0], 7))
    for a in range(cfg.n_yaw):
        hy = (cfg.yaw_min + a * cfg.yaw_step) * 0.5
        q = synth.quat_mul(np.array([0.0, 0.0, np.sin(hy), np.cos(hy)]), guess[3:])
        out[a, ..., 3:] = q / np.linalg.norm(q)
    for axis, ax_n in enumerate(n):
        shape = [1, 1, 1, 1]; shape[3 - axis] = ax_n
        out[..., axis] = guess[axis] + cfg.step * (np.arange(ax_n) - cfg.half[axis]).reshape(shape)
    return out.reshape(-1, 7)


def shape(name, mc, ms, corner, surf, guess, cfg, reps, with_score=True):
    d_mc, d_ms = torch.from_numpy(mc).to(dev), torch.from_numpy(ms).to(dev)
    d_c, d_s = torch.from_numpy(corner).to(dev), torch.from_numpy(surf).to(dev)
    h.set_map(d_mc, d_ms, len(mc), len(ms), capi.MEM_DEVICE)
    _, geom = capi.search_geometry(guess, cfg, len(corner), len(surf))
    H = int(geom.n_hypotheses)
    d_cand = torch.zeros(16 * capi.POSE_CANDIDATE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_n = torch.zeros(1, dtype=torch.int32, device=dev)
    search = lambda: h.search_poses_device(d_c, len(corner), d_s, len(surf), guess, cfg, d_cand, 16, d_n)
    if args.only_search:
        for _ in range(args.only_search):
            search()
        torch.cuda.synchronize(dev)
        return {}
    ms_search = timed(search, reps, args.warmup)
    r = {"map_points": len(mc) + len(ms), "features": len(corner) + len(surf), "hypotheses": H, "dims": list(geom.dims),
         "volume_bytes_per_kind": int(geom.volume_bytes), "scratch_bytes": int(geom.scratch_bytes), "search_ms_per_call": ms_search,
         "search_ns_per_hypothesis": 1e6 * ms_search / H}
    if with_score:
        d_h = torch.from_numpy(lattice_poses(guess, cfg)).to(dev)
        d_sc = torch.zeros(H * capi.POSE_SCORE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        ms_score = timed(lambda: h.score_poses_device(d_c, len(corner), d_s, len(surf), d_h, H, 1.0, d_sc), 5, 2)
        r.update({"score_ms_per_call": ms_score, "search_over_score": ms_search / ms_score})
    print(name, r, file=sys.stderr)
    return r


def world_case(kind):
    world = synth.World(ground_half=synth.ground_half_for_target(50000)) if kind == "room" else synth.World(kind=kind)
    mc, ms = synth.make_map(world)
    truth = (synth.random_poses(1, synth.SEED + 5) if kind == "room" else synth.world_poses(world, 1, synth.SEED + 5))[0]
    pts, _, k = synth.make_scan(world, truth, synth.SEED + 6, with_kind=True)
    corner, surf = synth.direct_features(pts, k)
    return mc, ms, corner, surf, truth


def quality(kind):
    mc, ms, corner, surf, truth = world_case(kind)
    guess = np.array(truth)
    guess[0] += 1.2; guess[1] -= 0.9
    hy = -np.deg2rad(34.0) / 2.0
    q = synth.quat_mul(np.array([0.0, 0.0, np.sin(hy), np.cos(hy)]), truth[3:])
    guess[3:] = q / np.linalg.norm(q)
    rng = float(np.ceil(np.percentile(np.linalg.norm(np.concatenate([corner, surf])[:, :3], axis=1), 99)))
    cfg = capi.SearchConfig(half=(4, 4, 0), range=rng)
    h.set_map(mc, ms)
    exact = h.score_poses(corner, surf, lattice_poses(guess, cfg), 1.0)
    best = int(np.lexsort((np.arange(len(exact)), exact["sum_sq_q32"].sum(1), -exact["inliers"].sum(1).astype(np.int64)))[0])
    every = h.search_poses(corner, surf, guess, capi.SearchConfig(half=(4, 4, 0), range=rng, nms_cells=0, nms_yaws=0), capacity=1024)
    peaks = h.search_poses(corner, surf, guess, cfg, capacity=1024)
    rank = lambda rec: int(np.flatnonzero(rec["h"] == best)[0]) + 1 if (rec["h"] == best).any() else None
    res = h.relocalize(corner, surf, guess, cfg, n_candidates=16, max_dist=1.0, n_refine=16, min_fitness=0.5)
    ref, _, _ = h.match_scan2map_batch(corner, [0, len(corner)], surf, [0, len(surf)], [truth])
    err = [synth.pose_error(r["pose"], ref[0]) for r in res]
    good = int(sum(dt < 0.01 and np.rad2deg(dr) < 0.1 for dt, dr in err))
    dt0, dr0 = synth.pose_error(res[0]["pose"], truth)
    return {"features": len(corner) + len(surf), "range": rng, "exact_best_h": best, "its_rank_among_all_hypotheses": rank(every),
            "its_rank_among_peaks": rank(peaks), "peaks": len(peaks), "candidates_refined": len(res), "refined_to_the_truths_own_pose": good,
            "best_total": int(peaks[0]["hits"].sum()), "accepted_first": int(res[0]["accepted"]), "first_dt_m": dt0, "first_dr_deg": float(np.rad2deg(dr0))}


co, so = inp["corner_off"], inp["surf_off"]
c0, s0, truth = np.ascontiguousarray(inp["corner"][co[0]:co[1]]), np.ascontiguousarray(inp["surf"][so[0]:so[1]]), inp["truth"][0]
rng0 = float(np.ceil(np.percentile(np.linalg.norm(np.concatenate([c0, s0])[:, :3], axis=1), 99)))
reloc = dict(step=0.4, n_yaw=40, yaw_step=np.pi / 40, yaw_wraps=0, range=rng0)
out = {"range": rng0}
out["reloc_shape"] = shape("reloc", inp["map_corner"], inp["map_surf"], c0, s0, truth, capi.SearchConfig(half=(25, 24, 0), **reloc), args.reps)
if not args.only_search:
    out["reloc_shape_z5"] = shape("reloc z5", inp["map_corner"], inp["map_surf"], c0, s0, truth, capi.SearchConfig(half=(25, 24, 2), **reloc), 10,
                                  with_score=False)
    mc, ms, corner, surf, t_out = world_case("outdoor")
    r_out = float(np.ceil(np.percentile(np.linalg.norm(np.concatenate([corner, surf])[:, :3], axis=1), 99)))
    out["reloc_shape_outdoor"] = shape("outdoor", mc, ms, corner, surf, t_out,
                                       capi.SearchConfig(half=(25, 24, 0), **dict(reloc, range=r_out)), args.reps)
    if not args.no_quality:
        out["quality"] = {kind: quality(kind) for kind in ("room", "outdoor", "corridor")}
h.close()
print(json.dumps(out))
