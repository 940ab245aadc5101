"""Throughput of the place database (msfl_places_*) at the bench shape.
    python tools/place_throughput.py [--scans 1024] [--entries 10000] [--queries 64] [--out profiles/place_throughput.json]

  add         ms per msfl_places_add of the bench's --scans VLP-16 scans (device-resident points, one call)
  yardstick   msfl_extract_features_batch over the same points in the same process (bench.py's stages.extract): both read the
              same raw points once
  query       ms per msfl_places_query of --queries scans against --entries entries (the scans' own descriptors, then rolled
              and thinned copies through msfl_places_add_descriptors), at n_prefilter 0 and 50, k = 10

Times are HIP events on the stream round back-to-back calls after a warm-up for the clock ramp.  One
JSON line, also written to --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from msf_loam_amd import capi, synth
from msf_loam_amd.pipeline import BatchPipeline

ap = argparse.ArgumentParser()
ap.add_argument("--scans", type=int, default=1024)
ap.add_argument("--entries", type=int, default=10000)
ap.add_argument("--queries", type=int, default=64)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_throughput.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("place_throughput.py needs a GPU (no CPU fallback)")
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
stream = torch.cuda.current_stream(dev)

# the bench's scans (bench.build_inputs: same world, poses and seeds), without its map and features
world = synth.World(ground_half=synth.ground_half_for_target(200000))
poses = synth.random_poses(args.scans, synth.SEED + 2)
raw = [synth.make_scan(world, poses[i], synth.SEED + 100 + i) for i in range(args.scans)]
pts = np.concatenate([p for p, _ in raw])
ring = np.concatenate([r for _, r in raw])
off = np.cumsum([0] + [len(p) for p, _ in raw]).astype(np.int32)
d_pts = torch.from_numpy(pts).to(dev)


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


out = {"scans": args.scans, "points": int(off[-1]), "points_per_scan": float(off[-1]) / args.scans}

h = capi.Handle(0)
h.set_stream(stream.cuda_stream)
pipe = BatchPipeline(h, pts, ring, off, dev)
out["extract_ms"] = timed(pipe.extract, args.reps, args.warmup)

# add: a database that holds one batch; every repetition refills it from empty (a fresh object per call would time hipMalloc)
total = args.scans * (args.warmup + args.reps)
pl = capi.Places(0, capacity=total)
pl.set_stream(stream.cuda_stream)
out["add_ms"] = timed(lambda: pl.add_device(d_pts, off), args.reps, args.warmup)
out["add_ns_per_point"] = 1e6 * out["add_ms"] / float(off[-1])
out["add_to_extract"] = out["add_ms"] / out["extract_ms"]
desc = pl.get(0, args.scans)
pl.close()

rng = np.random.default_rng(5)
extra = []
while len(desc) + len(extra) < args.entries:
    d = desc[int(rng.integers(len(desc)))]
    extra.append(np.roll(d, int(rng.integers(60)), axis=1) * (rng.uniform(size=d.shape) < rng.uniform(0.5, 1.0)))
db = capi.Places(0, capacity=args.entries)
db.set_stream(stream.cuda_stream)
db.add_descriptors(np.concatenate([desc, np.asarray(extra, np.float32).reshape(-1, *desc.shape[1:])])[:args.entries])
Q, K = args.queries, 10
q_off = off[:Q + 1]
d_out = torch.zeros(Q * K * capi.PLACE_MATCH_DTYPE.itemsize, dtype=torch.uint8, device=dev)
out["entries"], out["queries"], out["k"] = db.size(), Q, K
for npre in (0, 50):
    ms = timed(lambda: db.query_device(d_pts, q_off, d_out, n_prefilter=npre, k=K), max(args.reps // 4, 3), 3)
    rec = d_out.cpu().numpy().view(capi.PLACE_MATCH_DTYPE).reshape(Q, K)
    pairs = Q * (db.size() if npre == 0 else min(npre, db.size()))
    out["query_prefilter_%d" % npre] = {"ms": ms, "pairs": pairs, "us_per_pair": 1e3 * ms / pairs,
                                        "own_scan_first": float(np.mean(rec["index"][:, 0] == np.arange(Q)))}
db.close()
h.close()
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
