"""Closing a loop end to end: places -> score -> match -> pose graph -> corrected trajectory.

    python examples/close_loop.py [--scans 151] [--gap 50] [--every 1] [--max-distance 0.1] [--min-fitness 0.99] [--weights scalar|information]
                                  [--gate distance|mahalanobis] [--gate-bound 16.81]
                                  [--closure-map session|submap] [--submap-half-width 5] [--rebuild-map PATH]
                                  [--closure-loss KIND:A] [--closure-yaws N | --closure-search [HALF_WIDTH PITCH]]

The figure of eight of examples/loop_candidates.py.  Every scan goes through the device-resident SLAM step (keep_clouds) and into a
capi.Places.  The odometry the graph starts from is made to drift: the session's consecutive relative poses with a yaw bias and
noise on every step, integrated from the first pose.  Every --every-th scan is queried against the entries more than --gap scans
older; the candidate becomes a pose guess (the matched scan's map pose turned by the shift's yaw), msfl_score_poses grades it,
msfl_match_scan2map refines it, and a candidate with descriptor distance <= --max-distance whose refined pose has fitness >=
--min-fitness and lies within 1.5 m of the guess becomes a long edge whose measurement is the matched scan's map pose^-1 times
the refined pose (the room repeats itself, so looser rules let wrong closures in; on this path only its end closes).  capi.PoseGraph optimises the chain (first node fixed) and the absolute
trajectory error against the truth is printed before and after.  --weights information: the refinement runs with set_uncertainty, a
closure becomes the information edge of its registration (capi.edge_from_uncertainty: the registration's information matrix scaled by its
variance factor, without the directions it counts degenerate) in place of the hand-picked sr = 0.005 / st = 0.05, and the chi-square of
every closure is printed after the optimisation.  --gate mahalanobis replaces the 1.5 m rule: the chain is optimised with the odometry
alone first, the joint marginal of the two nodes of a candidate (PoseGraph.marginals) gives the predicted covariance Sigma_rel of their
relative pose (capi.relative_covariance), and the candidate passes when e^T (Sigma_rel + Sigma_z)^-1 e <= --gate-bound, e being the
measured relative pose against the predicted one in the edge's tangent and Sigma_z the closure's own covariance (the inverse of the
weights it would enter the graph with); the distance is printed for every candidate.  --closure-map submap measures a closure against
a submap instead of the session's (drifted) map: every scan becomes a keyframe of a capi.Keyframes, and ALL candidates (k, j) are
verified by one compose (the keyframes j-w .. j+w, w = --submap-half-width, laid down in j's frame at relative_pose(pose_map[j],
pose_map[i])) and one match_pairs_batch from the guess Rz(yaw) at the origin, whose result is the measurement itself; the acceptance
rules are the same, evaluated against the submap: ONE score_pairs call grades every result against its own submap, on the pair
index the match_pairs_batch left resident.  --closure-yaws N (with --closure-map submap; 0 = off) does not trust the descriptor's yaw
to its sector: set_pair_maps indexes the submaps once, score_pairs grades N yaws spread over the sector around the descriptor's per
candidate, the best one becomes the guess and match_pairs_resident registers from it on the same index.  --closure-search [HALF_WIDTH
PITCH] (with --closure-map submap, not with --closure-yaws; default 2 m at 0.5 m) does not trust the zero translation between the two
visits either: set_pair_maps indexes the submaps once, ONE search_pairs call counts hits over a position x yaw lattice round Rz(yaw)
at the origin per candidate (+-HALF_WIDTH in x and y at PITCH, five yaws over the descriptor's sector), ONE score_pairs call grades all
lattice candidates of all pairs exactly (a ragged pose_off), the best per pair by msfl_relocalize's order (exact inliers descending,
fixed-point sum ascending, candidate order) becomes the guess, and match_pairs_resident registers from it on the same index; the
1.5 m rule then compares against the searched guess.  The library has no msfl_relocalize over pairs: this is the chain.  --rebuild-map PATH lays the keyframes down again at the optimised poses
(Keyframes.insert into two fresh map stores) and saves them as PATH_corner.npz / PATH_surf.npz (mapio.save_grid).  --closure-loss KIND:A (geman_mcclure:1, cauchy:1, soft_l_one:2, huber:0.5, none) gives every closure edge a loss of its
own (PoseGraph.set_losses) while the odometry chain stays at the graph's Huber loss, in both weight modes: a redescending loss switches
a closure that contradicts the rest off inside the solve, and after the optimisation every closure's weight rho'(|r|^2)
(PoseGraph.weights; 1: kept, near 0: switched off) is printed next to its chi-square.  A demonstration;
the acceptance rule here is the example's, not the library's."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from msf_loam_amd import capi, mapio, synth


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


def drifting(pose_map, rng, yaw_bias=0.004, sigma_t=0.01, sigma_r=0.002):
    """Relative poses of the session with a yaw bias and noise on every step, and the trajectory they integrate to."""
    rel, out = [], [np.array(pose_map[0])]
    for a, b in zip(pose_map[:-1], pose_map[1:]):
        z = capi.relative_pose(a, b)
        z[:3] += rng.normal(0.0, sigma_t, 3)
        w = np.r_[rng.normal(0.0, sigma_r, 2), yaw_bias + rng.normal(0.0, sigma_r)] * 0.5
        q = synth.quat_mul(z[3:], np.r_[w, 1.0])
        z[3:] = q / np.linalg.norm(q)
        rel.append(z)
        p, qa = out[-1][:3], out[-1][3:]
        qn = synth.quat_mul(qa, z[3:])
        out.append(np.r_[p + synth.quat_to_matrix(qa) @ z[:3], qn / np.linalg.norm(qn)])
    return np.array(rel), np.array(out)


def closure_information(weights, j, k, pose_j, refined, unc):
    """L^T L of the edge a closure would enter the graph with: the registration's, or the hand-picked sr = 0.005 / st = 0.05."""
    if weights == "information":
        status, rec = capi.edge_from_uncertainty(j, k, pose_j, refined, unc, unc["sigma2"] if unc["sigma2"] > 0.0 else 1.0)
        if status != capi.OK:
            return None
        L = rec["sqrt_information"][0]
        return L.T @ L
    return np.diag(np.r_[np.full(3, 1.0 / 0.05 ** 2), np.full(3, 1.0 / (2.0 * 0.005) ** 2)])


def mahalanobis(g, x, j, k, z, info):
    """e^T (Sigma_rel + Sigma_z)^-1 e of the measured relative pose z of nodes (j, k) against the graph's current poses x, through the
    information form info - info (Sigma_rel^-1 + info)^-1 info, which also holds for a rank-deficient info = Sigma_z^-1."""
    S, sm = g.marginals([(j, j), (j, k), (k, k)])
    if sm.singular:
        return np.inf
    status, rel_cov = capi.relative_covariance(x[j], x[k], S[0], S[1], S[2])
    if status != capi.OK:
        return np.inf
    pred = capi.relative_pose(x[j], x[k])
    qe = synth.quat_mul(np.r_[-z[3:6], z[6]], pred[3:])
    e = np.r_[pred[:3] - z[:3], 2.0 * np.sign(qe[3]) * qe[:3]]
    W = info - info @ np.linalg.solve(np.linalg.inv(rel_cov) + info, info)
    return float(e @ W @ e)


def ate(poses, truth):
    return float(np.sqrt(np.mean(np.sum((np.asarray(poses)[:, :3] - truth[:, :3]) ** 2, axis=1))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=151)
    ap.add_argument("--gap", type=int, default=50, help="a scan is only compared with entries more than this many scans older")
    ap.add_argument("--every", type=int, default=1, help="query every n-th scan")
    ap.add_argument("--max-distance", type=float, default=0.1, help="descriptor distance up to which a candidate is verified")
    ap.add_argument("--max-dist", type=float, default=1.0)
    ap.add_argument("--min-fitness", type=float, default=0.99)
    ap.add_argument("--weights", choices=("scalar", "information"), default="scalar", help="how a closure edge is weighted")
    ap.add_argument("--min-eigenvalue", type=float, default=150.0, help="information: eigenvalues of a registration below this are degenerate")
    ap.add_argument("--gate", choices=("distance", "mahalanobis"), default="distance",
                    help="accept a verified candidate within 1.5 m of its guess, or by its Mahalanobis distance against the odometry graph's marginals")
    ap.add_argument("--gate-bound", type=float, default=16.81, help="mahalanobis: the chi-square bound (16.81: 99 %% at 6 degrees of freedom)")
    ap.add_argument("--closure-map", choices=("session", "submap"), default="session",
                    help="verify a candidate against the session's whole map, or against the submap of the scans around the matched one")
    ap.add_argument("--submap-half-width", type=int, default=5, help="submap: the keyframes j-w .. j+w around the matched scan j")
    ap.add_argument("--rebuild-map", metavar="PATH", default=None, help="rebuild both map stores at the optimised poses: PATH_corner.npz, PATH_surf.npz")
    ap.add_argument("--closure-yaws", type=int, default=0,
                    help="submap: score this many yaws round the descriptor's per candidate against its submap and register from the best (0: off)")
    ap.add_argument("--closure-search", type=float, nargs="*", default=None, metavar="M",
                    help="submap: search a position x yaw lattice per candidate first (search_pairs): half-width and pitch in metres (default 2 0.5)")
    ap.add_argument("--closure-loss", metavar="KIND:A", default=None,
                    help="the loss of every closure edge, e.g. geman_mcclure:1 (kinds: %s); default: the graph's Huber loss" % ", ".join(capi.GRAPH_LOSS_NAMES[1:]))
    args = ap.parse_args()
    if args.closure_yaws < 0 or (args.closure_yaws > 0 and args.closure_map != "submap"):
        ap.error("--closure-yaws: a count >= 0, with --closure-map submap")
    if args.closure_search is not None:
        if args.closure_map != "submap" or args.closure_yaws > 0:
            ap.error("--closure-search: with --closure-map submap, and not with --closure-yaws")
        if len(args.closure_search) not in (0, 2) or any(not v > 0.0 for v in args.closure_search):
            ap.error("--closure-search: no value, or a positive half-width and a positive pitch")
        args.closure_search = tuple(args.closure_search) or (2.0, 0.5)
    closure_loss = None
    if args.closure_loss:
        kind, _, a = args.closure_loss.partition(":")
        if kind not in capi.GRAPH_LOSS_NAMES:
            ap.error("--closure-loss: unknown kind %r" % kind)
        closure_loss = (capi.GRAPH_LOSS_NAMES.index(kind), float(a or 0.0))

    world = synth.World()
    truth = figure_of_eight(args.scans)
    scans = [synth.make_scan(world, truth[k], synth.SEED + 7000 + k) for k in range(args.scans)]
    slam = capi.Slam(0, max_scan_points=max(len(p) for p, _ in scans), max_rings=16, pose_odom2map=truth[0], keep_clouds=1)
    places = capi.Places(0, capacity=max(args.scans, 1))
    pose_map, candidates = [], []
    keep = args.closure_map == "submap" or args.rebuild_map is not None
    hk = capi.Handle(0) if keep else None
    kf = capi.Keyframes(hk, max_keyframes=args.scans) if keep else None      # every scan a keyframe, filtered at 0.2 / 0.4 m like the map's inserts
    for k, (pts, ring) in enumerate(scans):
        r = slam.add_scan(pts, ring)
        pose_map.append(np.array(r.pose_map[:]))
        cl = slam.clouds(k)
        assert places.add(cl["full_scan"]) == k
        if kf is not None:
            assert kf.add(cl["full_scan"], cl["full_scan"], corner_idx=cl["less_sharp"], surf_idx=cl["less_flat"]) == k
        if k > args.gap and k % args.every == 0:
            m = places.query_entries(k, max_index=k - args.gap, k=1)[0, 0]
            if m["index"] >= 0 and m["distance"] <= args.max_distance:
                candidates.append((k, m.copy(), cl["full_scan"][cl["less_sharp"]], cl["full_scan"][cl["less_flat"]]))

    rel, drifted = drifting(pose_map, np.random.default_rng(synth.SEED))
    grid_c, grid_s = slam.grids()
    submap = args.closure_map == "submap"
    h = hk if submap else capi.Handle(0)
    if not submap:
        h.set_map(grid_c.dump(), grid_s.dump())
    if args.weights == "information":
        h.set_uncertainty(max(len(candidates), 1) if submap else 1, args.min_eigenvalue)
    n = args.scans
    identity = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    if submap and candidates:
        # every candidate at once: submap p = the keyframes around j laid down in j's frame, scan k registered against it from the
        # guess Rz(yaw) at the origin; the result is the measured T_j^-1 T_k itself
        w = args.submap_half_width
        keys, member_off, guesses = [], [0], []
        for k, m, _, _ in candidates:
            j = int(m["index"])
            keys += list(range(max(j - w, 0), min(j + w, n - 1) + 1))
            member_off.append(len(keys))
            guesses.append(turned(identity, float(capi.place_yaw(m["shift"], places.n_sector))))
        member_poses = [capi.relative_pose(pose_map[int(candidates[p][1]["index"])], pose_map[i])
                        for p in range(len(candidates)) for i in keys[member_off[p]:member_off[p + 1]]]
        sub_c, sub_co, sub_s, sub_so = kf.compose(member_off, keys, member_poses, 0.2, 0.4)
        feats = [kf.get(k) for k, _, _, _ in candidates]
        co = np.cumsum([0] + [len(c) for c, _ in feats]).astype(np.int32)
        so = np.cumsum([0] + [len(s) for _, s in feats]).astype(np.int32)
        all_c, all_s = np.concatenate([c for c, _ in feats]), np.concatenate([s for _, s in feats])
        if args.closure_yaws > 0:
            # the submaps indexed once; N yaws over the descriptor's sector scored per candidate, the registration starts from the best
            h.set_pair_maps(sub_c, sub_co, sub_s, sub_so)
            N, sector = args.closure_yaws, 2.0 * np.pi / places.n_sector
            offsets = (np.arange(N) - (N - 1) / 2.0) * sector / N
            lattice = np.array([turned(gs, d) for gs in guesses for d in offsets])
            rec = h.score_pairs(all_c, co, all_s, so, lattice, np.arange(len(candidates) + 1) * N, args.max_dist)
            for p, (c, s) in enumerate(feats):
                fit = capi.fitness(rec[p * N:(p + 1) * N], len(c), len(s))
                best = int(np.lexsort((np.abs(offsets), -fit))[0])           # the fittest; among equals the one nearest the descriptor's
                print("scan %3d ~ scan %3d: yaw %+6.1f deg of %d scored (fitness %.3f; the descriptor's own %.3f)"
                      % (candidates[p][0], int(candidates[p][1]["index"]), np.degrees(offsets[best]), N, fit[best], fit[int(np.argmin(np.abs(offsets)))]))
                guesses[p] = lattice[p * N + best]
            sub_z, sub_status, _ = h.match_pairs_resident(all_c, co, all_s, so, guesses)
        elif args.closure_search:
            # the submaps indexed once; one lattice search over all pairs, one exact score of all its candidates, the registration
            # starts from each pair's best (msfl_relocalize's chain, over pairs)
            h.set_pair_maps(sub_c, sub_co, sub_s, sub_so)
            half_width, pitch = args.closure_search
            N, sector = 5, 2.0 * np.pi / places.n_sector
            reach = np.concatenate([np.linalg.norm(all_c[:, :3], axis=1), np.linalg.norm(all_s[:, :3], axis=1)])
            cells = int(np.ceil(half_width / pitch))
            cfg = capi.SearchConfig(step=pitch, half=(cells, cells, 0), n_yaw=N, yaw_min=-(N - 1) / 2.0 * sector / N, yaw_step=sector / N, yaw_wraps=0,
                                    range=float(np.percentile(reach[np.isfinite(reach)], 99)))
            found = h.search_pairs(all_c, co, all_s, so, guesses, cfg, capacity=8)
            pose_off = np.cumsum([0] + [len(f) for f in found]).astype(np.int32)
            rec = h.score_pairs(all_c, co, all_s, so, np.concatenate([f["pose"] for f in found]).reshape(-1, 7), pose_off, args.max_dist)
            for p, (c, s) in enumerate(feats):
                r, f = rec[pose_off[p]:pose_off[p + 1]], found[p]
                if len(f) == 0:
                    print("scan %3d ~ scan %3d: search found no peak, the descriptor's guess stays" % (candidates[p][0], int(candidates[p][1]["index"])))
                    continue
                best = int(np.lexsort((np.arange(len(r)), r["sum_sq_q32"].sum(1), -r["inliers"].sum(1).astype(np.int64)))[0])
                fit = capi.fitness(r, len(c), len(s))
                print("scan %3d ~ scan %3d: search node (%+d, %+d) x %.2f m, yaw %+5.1f deg, %d hits, candidate %d of %d (fitness %.3f; the first one's %.3f)"
                      % (candidates[p][0], int(candidates[p][1]["index"]), f["kx"][best], f["ky"][best], pitch,
                         np.degrees(cfg.yaw_min + f["a"][best] * cfg.yaw_step), f["hits"][best].sum(), best, len(f), fit[best], fit[0]))
                guesses[p] = f["pose"][best].copy()
            sub_z, sub_status, _ = h.match_pairs_resident(all_c, co, all_s, so, guesses)
        else:
            sub_z, sub_status, _ = h.match_pairs_batch(sub_c, sub_co, sub_s, sub_so, all_c, co, all_s, so, guesses)
        sub_unc = h.uncertainty(len(candidates)) if args.weights == "information" else None
        # every result graded against its own submap at once, on the index the registration left resident
        sub_score = h.score_pairs(all_c, co, all_s, so, sub_z, np.arange(len(candidates) + 1), args.max_dist)
    g = capi.PoseGraph(0, max_nodes=n, max_edges=n + len(candidates), max_fixes=1)
    g.add_nodes(drifted)
    g.set_fixed(0)
    g.add_edges(g.edges(np.arange(n - 1), np.arange(1, n), rel, sr=0.01, st=0.1))
    if args.gate == "mahalanobis":                    # the odometry alone: what the graph predicts before any closure
        s = g.optimize()
        predicted = g.poses()
        print("odometry graph: %s after %d iterations; the gate reads its marginals" % (capi.GRAPH_TERMINATION[s.termination], s.iterations))
    closures = []
    for p, (k, m, sharp, flat) in enumerate(candidates):
        j, yaw = int(m["index"]), float(capi.place_yaw(m["shift"], places.n_sector))
        if submap:
            # the pair's registration and its score against its own submap, in j's frame, ran above
            (corner, surf), base, guess = feats[p], identity, guesses[p]
            status, refined = int(sub_status[p]), sub_z[p]
            unc = sub_unc[p] if args.weights == "information" else None
            score = sub_score[p:p + 1]
        else:
            corner, surf = h.voxel_downsample(sharp, 0.2), h.voxel_downsample(flat, 0.4)
            base, guess = pose_map[j], turned(pose_map[j], yaw)
            status, refined, _ = h.match_scan2map(corner, surf, guess)
            unc = h.uncertainty(1)[0] if args.weights == "information" else None
            score = h.score_poses(corner, surf, [refined], args.max_dist)
        fit = capi.fitness(score, len(corner), len(surf))[0]
        z = capi.relative_pose(base, np.asarray(refined))
        if args.gate == "mahalanobis":
            info = closure_information(args.weights, j, k, base, np.asarray(refined, np.float64), unc) if status == 0 else None
            d2 = mahalanobis(g, predicted, j, k, z, info) if info is not None else np.inf
            print("scan %3d ~ scan %3d: Mahalanobis distance %.3g against the bound %.3g" % (k, j, d2, args.gate_bound))
            ok = status == 0 and fit >= args.min_fitness and d2 <= args.gate_bound
        else:
            ok = status == 0 and fit >= args.min_fitness and np.linalg.norm(np.asarray(refined)[:3] - guess[:3]) <= 1.5
        dt, dr = synth.pose_error(z, capi.relative_pose(truth[j], truth[k]))
        print("scan %3d ~ scan %3d: distance %.3f, yaw %+6.1f deg, refined fitness %.3f -> %s (measurement off the truth by %.3f m, %.2f deg)"
              % (k, j, m["distance"], np.degrees(yaw), fit, "edge" if ok else "dropped", dt, np.degrees(dr)))
        if ok:
            closures.append((j, k, z, unc, np.asarray(refined, np.float64), base))

    if args.gate == "mahalanobis":
        g.set_poses(drifted)
    if closures and args.weights == "scalar":
        g.add_edges(g.edges([c[0] for c in closures], [c[1] for c in closures], np.array([c[2] for c in closures]), sr=0.005, st=0.05))
    for j, k, _, unc, refined, base in closures if args.weights == "information" else []:
        status, rec = capi.edge_from_uncertainty(j, k, base, refined, unc, unc["sigma2"] if unc["sigma2"] > 0.0 else 1.0)
        if status != capi.OK:
            raise SystemExit("scan %d ~ scan %d: the registration left no usable uncertainty record" % (k, j))
        print("scan %3d ~ scan %3d: information edge of rank %d, sigma2 %.3g, sqrt of the kept eigenvalues / sigma2: %s"
              % (k, j, 6 - unc["n_degenerate"], unc["sigma2"], np.array2string(np.linalg.norm(rec["sqrt_information"][0], axis=1), precision=1)))
        g.add_edges_info(rec)
    closure_kind = capi.GRAPH_FACTOR_EDGE_INFO if args.weights == "information" else capi.GRAPH_FACTOR_EDGE
    first_closure = 0 if args.weights == "information" else n - 1         # scalar closures follow the chain's n - 1 edges
    if closure_loss and closures:
        g.set_losses(closure_kind, closure_loss, first=first_closure, n=len(closures))
        print("%d closure edges under the loss %s; the chain stays at Huber %g" % (len(closures), args.closure_loss, g.config.huber_delta))
    s = g.optimize()
    print("%d closure edges (%d of them long: both ends free, more than one apart); %s after %d iterations (%d CG iterations, %d unconverged); cost %.4g -> %.4g"
          % (len(closures), s.n_long_edges, capi.GRAPH_TERMINATION[s.termination], s.iterations, s.cg_iterations, s.cg_unconverged, s.initial_cost, s.final_cost))
    print("ATE against the truth: session %.3f m, drifting odometry %.3f m, after the optimisation %.3f m"
          % (ate(pose_map, truth), ate(drifted, truth), ate(g.poses(), truth)))
    if closure_loss and closures:
        chi, w = g.chi2(closure_kind, first_closure, len(closures)), g.weights(closure_kind, first_closure, len(closures))
        for (j, k, _, _, _, _), c, wk in zip(closures, chi, w):
            print("closure scan %3d ~ scan %3d: chi-square %.3g, weight %.3g under %s" % (k, j, c, wk, args.closure_loss))
    elif args.weights == "information":
        for (j, k, _, _, _, _), c in zip(closures, g.chi2(capi.GRAPH_FACTOR_EDGE_INFO)):
            print("closure scan %3d ~ scan %3d: chi-square %.3g (6 degrees of freedom under the model)" % (k, j, c))
    if args.rebuild_map is not None:
        # the corrected trajectory gets its map: every keyframe laid down again at its optimised pose, one insert per keyframe
        new_c, new_s = capi.Grid(hk, 3.0, 0.2), capi.Grid(hk, 3.0, 0.4)
        status, n_done = kf.insert(np.arange(n), g.poses(), new_c, new_s)
        for name, grid, old in (("corner", new_c, grid_c), ("surf", new_s, grid_s)):
            cells, points = mapio.save_grid("%s_%s.npz" % (args.rebuild_map, name), grid)
            print("rebuilt %s map: %d keyframes, %d cells, %d points (the session's store: %d points) -> %s_%s.npz"
                  % (name, n_done, cells, points, old.size()[0], args.rebuild_map, name))
        # and at the session's own poses: is that the session's map?
        own_c, own_s = capi.Grid(hk, 3.0, 0.2), capi.Grid(hk, 3.0, 0.4)
        kf.insert(np.arange(n), pose_map, own_c, own_s)
        for name, grid, old in (("corner", own_c, grid_c), ("surf", own_s, grid_s)):
            a, b = grid.dump(), old.dump()
            same_cells = np.array_equal(grid.dump_cells()[:, :3], old.dump_cells()[:, :3])
            print("rebuilt at the session's own poses, %s: %d points against the session's %d, %s, %s"
                  % (name, len(a), len(b), "the same cells" if same_cells else "other cells", "equal bit for bit" if np.array_equal(a, b) else "not equal"))
    g.close()
    if hk is not None and hk is not h:
        hk.close()
    h.close()
    places.close()
    slam.close()


if __name__ == "__main__":
    main()
