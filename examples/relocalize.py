"""Relocalise one scan in a saved map from a guess metres and tens of degrees off (msfl_search_poses / msfl_relocalize).

    python examples/relocalize.py [--map PREFIX] [--world room|outdoor|corridor] [--offset 1.2 -0.9] [--yaw-off 34]
                                  [--step 0.5] [--half 6 6 0] [--yaws 24] [--candidates 16] [--refine 5] [--min-fitness 0.5] [--places]

--map PREFIX loads PREFIX.corner.npz / PREFIX.surf.npz (msf_loam_amd/mapio.py; examples/replay_synthetic.py --save-map writes them);
without it the world's sampled map is used.  The scan is ray-cast at a true pose of the world; the guess is that pose moved by
--offset and turned by --yaw-off.  Printed: the coarse candidates (hit counts), their exact scores, what the matcher makes of the
best --refine and the accepted pose with its distance from the truth.

--places: the lattice is not centred on the displaced guess but on the best entry of a place database (capi.Places) built from
twelve scans on a 2 m grid round the true pose, turned by that entry's place_yaw: the chain "a candidate place" -> "a registered pose".
The coarse stage replaces the exact walk of examples/score_lattice.py over the whole lattice (docs/kernels/search.md)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from msf_loam_amd import capi, synth


def yawed(pose, yaw, dx=0.0, dy=0.0):
    out = np.array(pose, np.float64)
    out[0] += dx; out[1] += dy
    q = synth.quat_mul(np.array([0.0, 0.0, np.sin(yaw / 2.0), np.cos(yaw / 2.0)]), out[3:])
    out[3:] = q / np.linalg.norm(q)
    return out


def place_guess(world, pts, truth):
    """The pose of the database entry that matches the scan best, turned by the match's yaw.  The database: twelve scans on a 2 m
    grid round the true pose, each at another heading."""
    drive = [yawed(truth, 0.7 * k, 2.0 * (k % 4) - 3.0, 2.0 * (k // 4) - 2.0) for k in range(12)]
    places = capi.Places(0)
    for k, pose in enumerate(drive):
        places.add(synth.make_scan(world, pose, synth.SEED + 41 + k)[0])
    m = places.query(pts, k=1)[0][0]
    n_sector = places.n_sector
    places.close()
    print("best place: entry %d, shift %d of %d sectors, distance %.4f" % (m["index"], m["shift"], n_sector, m["distance"]))
    return yawed(drive[int(m["index"])], float(capi.place_yaw(int(m["shift"]), n_sector)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", default=None, metavar="PREFIX")
    ap.add_argument("--world", choices=["room", "outdoor", "corridor"], default="room")
    ap.add_argument("--offset", type=float, nargs=2, default=(1.2, -0.9))
    ap.add_argument("--yaw-off", type=float, default=34.0, help="degrees")
    ap.add_argument("--step", type=float, default=0.5)
    ap.add_argument("--half", type=int, nargs=3, default=(6, 6, 0))
    ap.add_argument("--yaws", type=int, default=24)
    ap.add_argument("--candidates", type=int, default=16)
    ap.add_argument("--refine", type=int, default=5)
    ap.add_argument("--max-dist", type=float, default=1.0)
    ap.add_argument("--min-fitness", type=float, default=0.5)
    ap.add_argument("--places", action="store_true")
    args = ap.parse_args()

    world = synth.World(ground_half=synth.ground_half_for_target(50000)) if args.world == "room" else synth.World(kind=args.world)
    if args.map:
        from msf_loam_amd import mapio
        map_corner, map_surf = (mapio.read_map("%s.%s.npz" % (args.map, side))[3] for side in ("corner", "surf"))
    else:
        map_corner, map_surf = synth.make_map(world)
    truth = (synth.random_poses(1, synth.SEED + 5) if args.world == "room" else synth.world_poses(world, 1, synth.SEED + 5))[0]
    pts, _, kind = synth.make_scan(world, truth, synth.SEED + 6, with_kind=True)
    corner, surf = synth.direct_features(pts, kind)
    guess = place_guess(world, pts, truth) if args.places else yawed(truth, -np.deg2rad(args.yaw_off), *args.offset)
    reach = float(np.ceil(np.percentile(np.linalg.norm(np.concatenate([corner, surf])[:, :3], axis=1), 99)))
    cfg = capi.SearchConfig(step=args.step, half=args.half, n_yaw=args.yaws, yaw_step=2.0 * np.pi / args.yaws, range=reach)
    _, geom = capi.search_geometry(guess, cfg, len(corner), len(surf))
    dt, dr = synth.pose_error(guess, truth)
    print("%s world: map %d + %d points, scan %d + %d features; guess %.2f m / %.1f deg off; %d hypotheses, volume %d x %d x %d voxels (%.1f MB a kind)"
          % (args.world, len(map_corner), len(map_surf), len(corner), len(surf), dt, np.rad2deg(dr), geom.n_hypotheses, geom.dims[0], geom.dims[1],
             geom.dims[2], geom.volume_bytes / 1e6))

    h = capi.Handle(0)
    h.set_map(map_corner, map_surf)
    cand = h.search_poses(corner, surf, guess, cfg, capacity=args.candidates)
    exact = h.score_poses(corner, surf, cand["pose"], args.max_dist)
    fit = capi.fitness(exact, len(corner), len(surf))
    print("rank  hits corner + surf   a   kx  ky  kz   exact fitness  |dt| [m]  |dr| [deg]")
    for r, c in enumerate(cand):
        dt, dr = synth.pose_error(c["pose"], truth)
        print("%4d  %5d + %5d      %3d  %3d %3d %3d   %.4f         %.3f     %.2f" % (r + 1, c["hits"][0], c["hits"][1], c["a"], c["kx"], c["ky"], c["kz"],
                                                                                  fit[r], dt, np.rad2deg(dr)))
    res = h.relocalize(corner, surf, guess, cfg, n_candidates=args.candidates, max_dist=args.max_dist, n_refine=min(args.refine, args.candidates),
                       min_fitness=args.min_fitness)
    print("refined (msfl_relocalize):")
    print("rank  from h  status  fitness before -> after   |dt| [m]  |dr| [deg]  accepted")
    for r, x in enumerate(res):
        dt, dr = synth.pose_error(x["pose"], truth)
        print("%4d  %6d  %6d  %.4f -> %.4f          %.4f    %.3f      %d" % (r + 1, x["candidate"]["h"], x["status"],
              capi.fitness(res["coarse"][r:r + 1], len(corner), len(surf))[0], capi.fitness(res["refined"][r:r + 1], len(corner), len(surf))[0],
              dt, np.rad2deg(dr), x["accepted"]))
    if len(res) and res[0]["accepted"]:
        print("accepted pose:", np.array2string(res[0]["pose"], precision=4))
    else:
        print("no candidate reached the fitness", args.min_fitness)
    h.close()


if __name__ == "__main__":
    main()
