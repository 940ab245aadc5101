"""Throughput of the resident pair maps at the shape of docs/kernels/pairs.md: P (map, scan) pairs with P different ~34 k-point maps,
device resident, one hypothesis per pair and then 16.
    python tools/score_pairs_throughput.py [--pairs 256] [--map-points 30000] [--out profiles/score_pairs_throughput.json]

In one process, per hypothesis count:
  loop                  msfl_set_map + msfl_score_poses per pair: what grading P results against their own maps took before
  set_and_score         msfl_set_pair_maps + msfl_score_pairs
  score_resident        msfl_score_pairs on the resident index
and once:
  match_pairs_batch     index build + registrations (msfl_get_timing's index build reported next to it)
  match_pairs_resident  the registrations against the resident index

Times are HIP events on the handle's stream round --reps back-to-back calls after --warmup calls; the two
registration forms include the copy that resets their poses.  Writes one JSON object to --out and prints it."""
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
ap.add_argument("--hypotheses", type=int, nargs="+", default=[1, 16])
ap.add_argument("--max-dist", type=float, default=1.0)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_pairs_throughput.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("score_pairs_throughput.py needs a GPU (no CPU fallback)")
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
P = args.pairs
rng = np.random.default_rng(12)
mcs, mss, cs, ss, guesses, truths = [], [], [], [], [], []
for p in range(P):                                       # the pairs of tools/pairs_throughput.py
    w = synth.World(seed=synth.SEED + 700 + p, ground_half=synth.ground_half_for_target(args.map_points))
    mc, ms = synth.make_map(w, seed=synth.SEED + 1700 + p)
    truth = synth.random_poses(1, synth.SEED + 2700 + p)[0]
    pts, ring, kind = synth.make_scan(w, truth, synth.SEED + 3700 + p, with_kind=True)
    c, s = synth.direct_features(pts, kind)
    mcs.append(mc); mss.append(ms); cs.append(c); ss.append(s); guesses.append(synth.perturb_pose(truth, rng)); truths.append(truth)
cat = lambda ls: (np.concatenate(ls), np.cumsum([0] + [len(a) for a in ls]).astype(np.int32))   # noqa: E731
(mc, mco), (ms, mso), (c, co), (s, so) = cat(mcs), cat(mss), cat(cs), cat(ss)
guesses = np.array(guesses)
h = capi.Handle(0)
stream = torch.cuda.current_stream(dev)
h.set_stream(stream.cuda_stream)
d = {k: torch.from_numpy(v).to(dev) for k, v in dict(mc=mc, ms=ms, c=c, s=s, g=guesses).items()}
d_poses = torch.empty_like(d["g"]); d_status = torch.zeros(P, dtype=torch.int32, device=dev)
REC = capi.POSE_SCORE_DTYPE.itemsize


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.warmup):
        fn()
    a.record(stream)
    for _ in range(args.reps):
        fn()
    b.record(stream)
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / args.reps


out = {"pairs": P, "map_points_total": int(len(mc) + len(ms)), "map_points_per_pair": int((len(mc) + len(ms)) / P),
       "features_total": int(len(c) + len(s)), "max_dist": args.max_dist, "warmup": args.warmup, "reps": args.reps, "scoring": {}}
set_maps = lambda: h.set_pair_maps_device(P, d["mc"], mco, d["ms"], mso)   # noqa: E731
for n_hyp in args.hypotheses:
    # hypothesis 0 of a pair is its perturbed guess, the others are further perturbations of its truth
    hyp = np.array([[guesses[p]] + [synth.perturb_pose(truths[p], rng) for _ in range(n_hyp - 1)] for p in range(P)]).reshape(P * n_hyp, 7)
    d_h = torch.from_numpy(hyp).to(dev)
    po = (np.arange(P + 1) * n_hyp).astype(np.int32)
    d_rec = torch.zeros(P * n_hyp * REC, dtype=torch.uint8, device=dev)
    d_rec_loop = torch.zeros(P * n_hyp * REC, dtype=torch.uint8, device=dev)
    score = lambda: h.score_pairs_device(P, d["c"], co, d["s"], so, d_h, po, args.max_dist, d_rec)   # noqa: E731

    def loop():
        for p in range(P):
            h.set_map(d["mc"][mco[p]:mco[p + 1]], d["ms"][mso[p]:mso[p + 1]], int(mco[p + 1] - mco[p]), int(mso[p + 1] - mso[p]), capi.MEM_DEVICE)
            h.score_poses_device(d["c"][co[p]:co[p + 1]], int(co[p + 1] - co[p]), d["s"][so[p]:so[p + 1]], int(so[p + 1] - so[p]),
                                 d_h[p * n_hyp:(p + 1) * n_hyp], n_hyp, args.max_dist, d_rec_loop[p * n_hyp * REC:(p + 1) * n_hyp * REC])

    def set_and_score():
        set_maps(); score()

    ms_loop = timed(loop)
    ms_both = timed(set_and_score)
    set_maps()
    ms_resident = timed(score)
    rec, rec_loop = d_rec.cpu().numpy().view(capi.POSE_SCORE_DTYPE), d_rec_loop.cpu().numpy().view(capi.POSE_SCORE_DTYPE)
    n_feat = np.repeat((np.diff(co) + np.diff(so)).astype(np.float64), n_hyp)
    out["scoring"]["%d_per_pair" % n_hyp] = {
        "hypotheses": int(P * n_hyp), "queries": int(n_feat.sum()),
        "loop_set_map_score_poses_ms": ms_loop, "set_pair_maps_score_pairs_ms": ms_both, "score_pairs_resident_ms": ms_resident,
        "loop_over_set_and_score": ms_loop / ms_both, "loop_over_resident": ms_loop / ms_resident,
        "resident_ps_per_query": 1e9 * ms_resident / n_feat.sum(),
        "records_equal_the_loop": bool(rec.tobytes() == rec_loop.tobytes()), "mean_fitness": float((rec["inliers"].sum(1) / n_feat).mean())}


def batch():
    d_poses.copy_(d["g"])
    h.match_pairs_batch_device(P, d["mc"], mco, d["ms"], mso, d["c"], co, d["s"], so, d_poses, d_status)


def resident():
    d_poses.copy_(d["g"])
    h.match_pairs_resident_device(P, d["c"], co, d["s"], so, d_poses, d_status)


ms_batch = timed(batch)
poses_batch = d_poses.cpu().numpy().copy()
ms_res = timed(resident)                                  # on the index the last batch call left
poses_res = d_poses.cpu().numpy().copy()
h.set_timing(1); h.get_timing(reset=True)
batch(); torch.cuda.synchronize(dev)
t = h.get_timing(reset=True); h.set_timing(0)
err = np.array([synth.pose_error(poses_res[p], truths[p]) for p in range(P)])
out["registration"] = {"match_pairs_batch_ms": ms_batch, "match_pairs_resident_ms": ms_res,
                       "index_build_both_kinds_ms": t.ms_index, "batch_minus_index_build_ms": ms_batch - t.ms_index,
                       "kernels_ms": {"knn": t.ms_assoc, "fit": t.ms_fit, "solve": t.ms_solve},
                       "poses_equal": bool(np.array_equal(poses_batch, poses_res)), "status_ok": int((d_status.cpu().numpy() == 0).sum()),
                       "max_pose_error_vs_truth_m_rad": [float(err[:, 0].max()), float(err[:, 1].max())]}
h.close()
text = json.dumps(out, indent=1)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text + "\n")
print(json.dumps(out))
