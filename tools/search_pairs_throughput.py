"""Throughput of msfl_search_pairs at the shape of tools/score_pairs_throughput.py: P (map, scan) pairs with P different ~34 k-point
maps, device resident, one lattice search per pair.
    python tools/search_pairs_throughput.py [--pairs 256] [--map-points 30000] [--score-pairs 16] [--out profiles/search_pairs_throughput.json]

In one process:
  search_pairs      msfl_search_pairs on the resident pair index: pitch 0.5 m, half {6, 6, 0}, 24 yaws, range = the scans'
                    99th-percentile feature range, 16 candidates per pair
  loop              what it replaces: msfl_set_map + msfl_search_poses per pair, then one msfl_set_pair_maps to restore the index
  score_pairs       msfl_score_pairs on the same hypotheses (the whole lattice of every pair), for the first --score-pairs pairs
  --only-search N   N calls of search_pairs and nothing else (for a kernel trace)

Times are HIP events on the handle's stream round --reps back-to-back calls after --warmup calls.  Writes one
JSON object to --out and prints it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from msf_loam_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=256)
ap.add_argument("--map-points", type=int, default=30000)
ap.add_argument("--score-pairs", type=int, default=16, help="pairs whose whole lattice msfl_score_pairs grades (it is the slow yardstick)")
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--only-search", type=int, default=0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_pairs_throughput.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("search_pairs_throughput.py needs a GPU (no CPU fallback)")
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
P = args.pairs
rng = np.random.default_rng(12)
mcs, mss, cs, ss, guesses = [], [], [], [], []
for p in range(P):                                       # the pairs of tools/score_pairs_throughput.py
    w = synth.World(seed=synth.SEED + 700 + p, ground_half=synth.ground_half_for_target(args.map_points))
    mc, ms = synth.make_map(w, seed=synth.SEED + 1700 + p)
    truth = synth.random_poses(1, synth.SEED + 2700 + p)[0]
    pts, ring, kind = synth.make_scan(w, truth, synth.SEED + 3700 + p, with_kind=True)
    c, s = synth.direct_features(pts, kind)
    mcs.append(mc); mss.append(ms); cs.append(c); ss.append(s); guesses.append(synth.perturb_pose(truth, rng))
cat = lambda ls: (np.concatenate(ls), np.cumsum([0] + [len(a) for a in ls]).astype(np.int32))   # noqa: E731
(mc, mco), (ms, mso), (c, co), (s, so) = cat(mcs), cat(mss), cat(cs), cat(ss)
guesses = np.array(guesses)
reach = np.linalg.norm(np.concatenate([c, s])[:, :3], axis=1)
cfg = capi.SearchConfig(step=0.5, half=(6, 6, 0), n_yaw=24, range=float(np.ceil(np.percentile(reach[np.isfinite(reach)], 99))))
_, geom = capi.search_geometry(guesses[0], cfg, int(np.diff(co).max()), int(np.diff(so).max()))
H, K = int(geom.n_hypotheses), 16
h = capi.Handle(0)
stream = torch.cuda.current_stream(dev)
h.set_stream(stream.cuda_stream)
d = {k: torch.from_numpy(v).to(dev) for k, v in dict(mc=mc, ms=ms, c=c, s=s).items()}
REC = capi.POSE_CANDIDATE_DTYPE.itemsize
d_cand, d_n = torch.zeros(P * K * REC, dtype=torch.uint8, device=dev), torch.zeros(P, dtype=torch.int32, device=dev)
d_cand_loop, d_n_loop = torch.zeros(P * K * REC, dtype=torch.uint8, device=dev), torch.zeros(P, dtype=torch.int32, device=dev)


def timed(fn, reps=args.reps, warmup=args.warmup):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warmup):
        fn()
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / reps


set_maps = lambda: h.set_pair_maps_device(P, d["mc"], mco, d["ms"], mso)   # noqa: E731
search = lambda: h.search_pairs_device(P, d["c"], co, d["s"], so, guesses, cfg, d_cand, K, d_n)   # noqa: E731


def loop():
    for p in range(P):
        h.set_map(d["mc"][mco[p]:mco[p + 1]], d["ms"][mso[p]:mso[p + 1]], int(mco[p + 1] - mco[p]), int(mso[p + 1] - mso[p]), capi.MEM_DEVICE)
        h.search_poses_device(d["c"][co[p]:co[p + 1]], int(co[p + 1] - co[p]), d["s"][so[p]:so[p + 1]], int(so[p + 1] - so[p]), guesses[p], cfg,
                              d_cand_loop[p * K * REC:(p + 1) * K * REC], K, d_n_loop[p:p + 1])
    set_maps()


set_maps()
if args.only_search:
    for _ in range(args.only_search):
        search()
    torch.cuda.synchronize(dev)
    h.close()
    raise SystemExit(0)
ms_search = timed(search)
ms_loop = timed(loop, max(args.reps // 10, 3), 2)
ms_set = timed(set_maps)
# the chunk size follows from the budget in msfl_api_search.inc (256 MiB; a pair takes its volumes, table, counts, keys)
f_max = int((np.diff(co) + np.diff(so)).max())
per_pair = 2 * (1 + cfg.dilate) * int(geom.volume_bytes) + 16 * cfg.n_yaw * f_max + 16 * H + REC * K + 8
chunk = int(os.environ.get("MSFL_SEARCH_CHUNK_PAIRS", 0)) or max(1, (256 << 20) // per_pair)
out = {"pairs": P, "map_points_total": int(len(mc) + len(ms)), "map_points_per_pair": int((len(mc) + len(ms)) / P),
       "features_total": int(len(c) + len(s)), "step": cfg.step, "half": list(cfg.half), "n_yaw": cfg.n_yaw, "range": cfg.range,
       "hypotheses_per_pair": H, "dims": list(geom.dims), "volume_bytes_per_kind": int(geom.volume_bytes), "scratch_bytes_per_pair": per_pair,
       "chunk_pairs": min(chunk, P), "chunks": -(-P // min(chunk, P)), "warmup": args.warmup, "reps": args.reps,
       "search_pairs_ms_per_call": ms_search, "search_pairs_us_per_pair": 1e3 * ms_search / P,
       "search_pairs_ns_per_hypothesis": 1e6 * ms_search / (P * H),
       "loop_set_map_search_poses_restore_ms": ms_loop, "set_pair_maps_ms": ms_set, "loop_over_search_pairs": ms_loop / ms_search,
       "candidates_equal_the_loop": bool(d_cand.cpu().numpy().tobytes() == d_cand_loop.cpu().numpy().tobytes()
                                         and np.array_equal(d_n.cpu().numpy(), d_n_loop.cpu().numpy()))}

# the exact scorer on the same hypotheses: the whole lattice of the first Q pairs
Q = max(1, min(args.score_pairs, P))
n = [2 * x + 1 for x in cfg.half]
lat = np.zeros((Q, cfg.n_yaw, n[2], n[1], n[0], 7))
for p in range(Q):
    for a in range(cfg.n_yaw):
        hy = (cfg.yaw_min + a * cfg.yaw_step) * 0.5
        q = synth.quat_mul(np.array([0.0, 0.0, np.sin(hy), np.cos(hy)]), guesses[p, 3:])
        lat[p, a, ..., 3:] = q / np.linalg.norm(q)
    for axis, ax_n in enumerate(n):
        shape = [1, 1, 1, 1]; shape[3 - axis] = ax_n
        lat[p, ..., axis] = guesses[p, axis] + cfg.step * (np.arange(ax_n) - cfg.half[axis]).reshape(shape)
d_h = torch.from_numpy(lat.reshape(-1, 7)).to(dev)
po = np.concatenate([np.arange(Q + 1) * H, np.full(P - Q, Q * H)]).astype(np.int32)      # the other pairs get no pose
d_sc = torch.zeros(Q * H * capi.POSE_SCORE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
ms_score = timed(lambda: h.score_pairs_device(P, d["c"], co, d["s"], so, d_h, po, 1.0, d_sc), 3, 1)
out.update({"score_pairs_pairs": Q, "score_pairs_ms_per_call": ms_score, "score_pairs_us_per_pair": 1e3 * ms_score / Q,
            "score_over_search_per_pair": (ms_score / Q) / (ms_search / P)})
h.close()
text = json.dumps(out, indent=1)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text + "\n")
print(json.dumps(out))
