"""CPU model of the deferred 5-NN walk (knn5_grid_k32<.., DEFER>, docs/kernels/scan2map.md "Capped row visits") on the bench map:
per wavefront of 64 voxel-ordered surf queries, the trip count (pair-iterations: the sum over the nine row positions of the longest
lane, plus the overflow loop), candidates per query, wave-level insertion passes, visited positions and deferred ranges, for the plain
walk and for each cap set, with the overflow as one flat loop and entry by entry.  Pass 1 is at a perturbed pose, pass 2 at the true one.

  python tools/sim/knn_defer_model.py [--scans 6] [--waves 16] [--depth 4] [--caps 8,4,4,1,1,1,1,1,1 ...]

The walk itself is tests/knn_defer_model.py (the restatement the CPU test checks against brute force)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from msf_loam_amd import synth                      # noqa: E402
from tests import knn_defer_model as dm             # noqa: E402
from tests import knn_grid_model as gm              # noqa: E402

DEFAULT_CAPS = ("8,4,4,1,1,1,1,1,1", "6,4,4,1,1,1,1,1,1", "6,4,4,2,2,2,2,2,2", "8,4,4,2,2,2,2,2,2", "8,5,5,3,3,3,3,3,3", "4,4,4,2,2,2,2,2,2")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=6)
    ap.add_argument("--waves", type=int, default=16, help="wavefronts sampled per scan")
    ap.add_argument("--depth", type=int, default=dm.SHIPPED_DEPTH)
    ap.add_argument("--caps", nargs="*", default=list(DEFAULT_CAPS))
    args = ap.parse_args()
    world = synth.World(ground_half=synth.ground_half_for_target(200000))         # the bench map
    _, ms = synth.make_map(world)
    ix = dm.Index(ms, gm.desc_of(ms))
    rng = np.random.default_rng(3)
    truth = synth.random_poses(args.scans, synth.SEED + 5)
    settings = [("plain", None, True)]
    for c in args.caps:
        caps = tuple(int(v) for v in c.split(","))
        settings += [("(%s) flat" % c, caps, True), ("(%s) entry-wise" % c, caps, False)]
    keys = ("trips", "cand", "passes", "visited", "most_deferred")
    tot = {(s[0], p): dict.fromkeys(keys, 0.0) for s in settings for p in (1, 2)}
    n_waves = 0
    for T in truth:
        pts, _ = synth.make_scan(world, T, synth.SEED + 6)
        sub = synth.voxel_downsample_np(pts, 0.4)[:, :3]           # voxel order, like the filter's output
        for p, pose in ((1, synth.perturb_pose(T, rng)), (2, T)):
            R = synth.quat_to_matrix(pose[3:])
            qs = (sub @ R.T + pose[:3]).astype(np.float32)[:64 * args.waves]
            qs = qs[:len(qs) // 64 * 64]
            su = dm.setup(ix, qs)
            d2 = [gm.l2_simple(ix.pts, q).tolist() for q in qs]
            for name, caps, flat in settings:
                for w0 in range(0, len(qs), 64):
                    lanes = [dm.walk(ix, su, i, d2[i], 1.0, caps, args.depth, trace=True)[1] for i in range(w0, w0 + 64)]
                    trips, passes, visited, most = dm.wave_stats(lanes, flat)
                    t = tot[(name, p)]
                    t["trips"] += trips; t["passes"] += passes; t["visited"] += visited; t["most_deferred"] += most
                    t["cand"] += sum(s["cand"] for s in lanes) / 64.0
            n_waves += (p == 1) * (len(qs) // 64)
    print("bench map, %d wavefronts of 64 surf queries from %d scans, stack depth %d; per wavefront (candidates: per query)" % (n_waves, args.scans, args.depth))
    print("%-34s | %-42s | %s" % ("setting", "pass 1: trips  cand  passes  visited  defer", "pass 2: trips  cand  passes  visited  defer"))
    for name, _, _ in settings:
        row = "%-34s" % name
        for p in (1, 2):
            t = tot[(name, p)]
            row += " | %13.1f %5.1f %7.1f %8.1f %6.1f" % tuple(t[k] / n_waves for k in keys)
        print(row)


if __name__ == "__main__":
    main()
