"""Loop-closure candidates from the place database (msfl_places_*), verified and refined with the pieces the library already had.

    python examples/loop_candidates.py [--scans 151] [--gap 50] [--prefilter 0]

A figure of eight through the synthetic room: the path comes back over its starting point after --scans scans, heading some 84
degrees off its first heading.  Every scan goes through the device-resident SLAM step (keep_clouds), its full cloud is added to a
capi.Places, and the scan is queried against the entries more than --gap scans older.  The best candidate of the run becomes a
pose guess: the stored map pose of the matched scan, turned by the yaw the column shift stands for.  msfl_score_poses grades the
guess against the map the session built, msfl_match_scan2map refines it, and the refined pose is graded again.  A demonstration of
how the primitives compose; examples/close_loop.py goes on from here to the pose graph.  No acceptance policy lives in the library."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from msf_loam_amd import capi, synth


def figure_of_eight(n):
    poses = []
    for k in range(n):
        t = np.pi * k / (n - 1)
        x, y = 9.0 * np.sin(t), 5.0 * np.sin(2.0 * t)
        yaw = np.arctan2(10.0 * np.cos(2.0 * t), 9.0 * np.cos(t))
        poses.append(np.r_[x, y, 1.8 + 0.02 * np.sin(3.0 * t), synth.quat_from_euler(0.01 * np.sin(2.0 * t), 0.01 * np.cos(t), yaw)])
    return np.array(poses)


def turned(pose, yaw):
    """pose * Rz(yaw): the same position, the heading turned about the scan's own z axis."""
    q = synth.quat_mul(pose[3:], np.array([0.0, 0.0, np.sin(yaw / 2.0), np.cos(yaw / 2.0)]))
    return np.r_[pose[:3], q / np.linalg.norm(q)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=151)
    ap.add_argument("--gap", type=int, default=50, help="a scan is only compared with entries more than this many scans older")
    ap.add_argument("--prefilter", type=int, default=0, help="n_prefilter of the query (0: compare every candidate)")
    ap.add_argument("--max-dist", type=float, default=1.0)
    args = ap.parse_args()

    world = synth.World()
    truth = figure_of_eight(args.scans)
    scans = [synth.make_scan(world, truth[k], synth.SEED + 7000 + k) for k in range(args.scans)]
    slam = capi.Slam(0, max_scan_points=max(len(p) for p, _ in scans), max_rings=16, pose_odom2map=truth[0], keep_clouds=1)
    places = capi.Places(0, capacity=max(args.scans, 1))
    pose_map, feats, best = [], None, None
    for k, (pts, ring) in enumerate(scans):
        r = slam.add_scan(pts, ring)
        pose_map.append(np.array(r.pose_map[:]))
        cl = slam.clouds(k)
        assert places.add(cl["full_scan"]) == k
        if k > args.gap:
            m = places.query_entries(k, max_index=k - args.gap, n_prefilter=args.prefilter, k=1)[0, 0]
            if m["index"] >= 0 and (best is None or m["distance"] < best[1]["distance"]):
                best, feats = (k, m.copy()), (cl["full_scan"][cl["less_sharp"]], cl["full_scan"][cl["less_flat"]])
    if best is None:
        raise SystemExit("no scan had a candidate: --scans must exceed --gap + 1")
    k, m = best
    j, yaw = int(m["index"]), float(capi.place_yaw(m["shift"], places.n_sector))
    guess = turned(pose_map[j], yaw)
    print("scan %d looks like scan %d: distance %.4f over %d columns, shift %d = yaw %+.1f deg, ring_key_d2 %d"
          % (k, j, m["distance"], m["n_columns"], m["shift"], np.degrees(yaw), m["ring_key_d2"]))
    print("  true offset between the two visits: %.2f m, %+.1f deg" % (np.linalg.norm(truth[k][:3] - truth[j][:3]),
                                                                         np.degrees(synth.pose_error(truth[j], truth[k])[1])))

    grid_c, grid_s = slam.grids()
    h = capi.Handle(0)
    h.set_map(grid_c.dump(), grid_s.dump())
    corner, surf = h.voxel_downsample(feats[0], 0.2), h.voxel_downsample(feats[1], 0.4)
    before = h.score_poses(corner, surf, [guess], args.max_dist)
    status, refined, _ = h.match_scan2map(corner, surf, guess)
    after = h.score_poses(corner, surf, [refined], args.max_dist)
    for name, pose, rec in (("guess", guess, before), ("refined", np.asarray(refined), after)):
        dt, dr = synth.pose_error(pose, truth[k])
        print("  %-8s fitness %.4f, rmse %.3f m; from the truth %.3f m, %.2f deg"
              % (name, capi.fitness(rec, len(corner), len(surf))[0], capi.rmse(rec)[0], dt, np.degrees(dr)))
    print("  the session's own pose of scan %d (no loop closed): from the truth %.3f m" % (k, np.linalg.norm(pose_map[k][:3] - truth[k][:3])))
    print("  match_scan2map status %d" % status)
    h.close()
    places.close()
    slam.close()


if __name__ == "__main__":
    main()
