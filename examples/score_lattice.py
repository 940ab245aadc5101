"""Score a position x yaw lattice of pose hypotheses for one scan against a resident map (msfl_score_poses), and optionally
refine the best few with the matcher.  A demonstration of how the scoring primitive composes; it is not a relocaliser: the
library's own lattice search, top-k and acceptance are msfl_search_poses / msfl_relocalize (examples/relocalize.py,
docs/kernels/search.md), whose coarse stage ranks such a lattice at a fraction of this exact walk's time.

    python examples/score_lattice.py [--world room|outdoor|corridor] [--half 3.0] [--step 0.5] [--yaws 24] [--refine 5]

The scan is ray-cast at a true pose; the lattice is centred on a guess displaced from it by --offset metres.  Printed: the ten
best hypotheses with fitness, rmse and their distance from the truth, and, with --refine N, what msfl_match_scan2map_batch makes
of the best N and how the refined poses score."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from msf_loam_amd import capi, synth


def yawed(pose, yaw, dx, dy):
    out = np.array(pose, np.float64)
    out[0] += dx; out[1] += dy
    q = synth.quat_mul(np.array([0.0, 0.0, np.sin(yaw / 2.0), np.cos(yaw / 2.0)]), out[3:])
    out[3:] = q / np.linalg.norm(q)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", choices=["room", "outdoor", "corridor"], default="room")
    ap.add_argument("--map-points", type=int, default=50000, help="room world: points of the map")
    ap.add_argument("--half", type=float, default=3.0, help="half width of the position lattice, metres")
    ap.add_argument("--step", type=float, default=0.5, help="pitch of the position lattice, metres")
    ap.add_argument("--yaws", type=int, default=24, help="yaw hypotheses per position (full turn)")
    ap.add_argument("--offset", type=float, nargs=2, default=(1.2, -0.9), help="displacement of the lattice centre from the truth")
    ap.add_argument("--max-dist", type=float, default=1.0)
    ap.add_argument("--refine", type=int, default=0, help="register the best N hypotheses and score the results")
    args = ap.parse_args()

    world = synth.World(ground_half=synth.ground_half_for_target(args.map_points)) if args.world == "room" else synth.World(kind=args.world)
    map_corner, map_surf = synth.make_map(world)
    truth = (synth.random_poses(1, synth.SEED + 5) if args.world == "room" else synth.world_poses(world, 1, synth.SEED + 5))[0]
    pts, _, kind = synth.make_scan(world, truth, synth.SEED + 6, with_kind=True)
    corner, surf = synth.direct_features(pts, kind)

    g = np.arange(-args.half, args.half + 1e-9, args.step)
    poses = np.array([yawed(truth, 2.0 * np.pi * j / args.yaws + np.deg2rad(4.0), args.offset[0] + dx, args.offset[1] + dy)
                      for dx in g for dy in g for j in range(args.yaws)])

    h = capi.Handle(0)
    h.set_map(map_corner, map_surf)
    rec = h.score_poses(corner, surf, poses, args.max_dist)
    fit, rmse = capi.fitness(rec, len(corner), len(surf)), capi.rmse(rec)
    at_truth = h.score_poses(corner, surf, [truth], args.max_dist)
    print("%s world: map %d + %d points, scan %d + %d features, %d hypotheses (%d positions x %d yaws)"
          % (args.world, len(map_corner), len(map_surf), len(corner), len(surf), len(poses), len(g) ** 2, args.yaws))
    print("at the true pose: fitness %.4f, rmse %.3f m" % (capi.fitness(at_truth, len(corner), len(surf))[0], capi.rmse(at_truth)[0]))
    order = np.lexsort((rmse, -fit))
    print("rank  fitness  rmse [m]  |dt| [m]  |dr| [deg]")
    for r, i in enumerate(order[:10]):
        dt, dr = synth.pose_error(poses[i], truth)
        print("%4d  %.4f   %.3f     %.3f     %.2f" % (r + 1, fit[i], rmse[i], dt, np.rad2deg(dr)))
    if args.refine > 0:
        best = order[:args.refine]
        n = len(best)
        co, so = np.arange(n + 1, dtype=np.int32) * len(corner), np.arange(n + 1, dtype=np.int32) * len(surf)
        refined, status, _ = h.match_scan2map_batch(np.tile(corner, (n, 1)), co, np.tile(surf, (n, 1)), so, poses[best])
        again = h.score_poses(corner, surf, refined, args.max_dist)
        print("refined by msfl_match_scan2map_batch:")
        print("rank  status  fitness before -> after   rmse [m] before -> after   |dt| [m]  |dr| [deg]")
        for r, i in enumerate(best):
            dt, dr = synth.pose_error(refined[r], truth)
            print("%4d  %6d  %.4f -> %.4f          %.3f -> %.3f              %.3f     %.2f"
                  % (r + 1, status[r], fit[i], capi.fitness(again, len(corner), len(surf))[r], rmse[i], capi.rmse(again)[r], dt, np.rad2deg(dr)))
    h.close()


if __name__ == "__main__":
    main()
