#!/usr/bin/env python3
"""Sequential odometry + mapping replay on a synthetic trajectory (the stand-in for BASELINE
configs[2], `nsh_indoor_outdoor.bag`, which is not available offline).

Per scan, like MSF_LOAM's LaserOdometry::AddLaserScan -> LaserMapping::Run (laser_odometry.cc:69-95,
laser_mapping.cc:138-258), LiDAR-only:
    extract features (stage A) -> MatchScan2Scan against the previous scan (stage B)
    -> pose_odom chain -> voxel down-sample (0.2 / 0.4 m) -> MatchScan2Map against the accumulated
    map (stage C) -> TransformUpdate -> insert the scan's features into the map.
The map store is the device-resident HybridGrid replacement (msfl_grid_*):
InsertScan2Map / GetSurroundedCloud as in laser_mapping.cc:273-278,330-338.  `backend` is either the
GPU library or, in tests, the CPU oracle driven through the same loop, so the two trajectories can
be compared pose by pose.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from msf_loam_amd import synth  # noqa: E402


def compose(a, b):
    """Rigid3d operator* (rigid_transform.h:105-111)."""
    Ra = synth.quat_to_matrix(a[3:])
    q = synth.quat_mul(a[3:], b[3:])
    return np.r_[Ra @ b[:3] + a[:3], q / np.linalg.norm(q)]


def inverse(a):
    qc = np.r_[-a[3:6], a[6]]
    return np.r_[-(synth.quat_to_matrix(qc) @ a[:3]), qc]


def transform_cloud(pose, pts):
    out = pts.copy()
    out[:, :3] = (pts[:, :3].astype(np.float64) @ synth.quat_to_matrix(pose[3:]).T + pose[:3]).astype(np.float32)
    return out


def trajectory(n, seed=synth.SEED + 300):
    """Smooth loop inside the room: ~0.25 m and ~1.5 deg per scan."""
    rng = np.random.default_rng(seed)
    poses = []
    for k in range(n):
        a = 2 * np.pi * k / max(n, 120)
        x, y = 9.0 * np.cos(a), 6.0 * np.sin(a)
        yaw = a + np.pi / 2
        poses.append(np.r_[x, y, 1.8 + 0.02 * np.sin(3 * a), synth.quat_from_euler(0.01 * np.sin(2 * a), 0.01 * np.cos(a), yaw)])
    del rng
    return np.array(poses)


class GpuBackend:
    def __init__(self, device=0):
        from msf_loam_amd import capi
        self.odo, self.mapper = capi.Handle(device), capi.Handle(device)    # two handles, like the reference's two matchers
        self.capi = capi

    def extract(self, pts, ring):
        return self.odo.extract_features(pts, ring)

    def voxel(self, pts, leaf):
        return self.mapper.voxel_downsample(pts, leaf)

    def scan2scan(self, last, cur, pose):
        s, p, _ = self.odo.match_scan2scan(last["full"][last["less_sharp"]], last["ring"][last["less_sharp"]],
                                           last["full"][last["less_flat"]], last["ring"][last["less_flat"]],
                                           cur["full"][cur["sharp"]], cur["full"][cur["flat"]], pose)
        return p

    def scan2map(self, mc, ms, corner, surf, pose):
        self.mapper.set_map(mc, ms)
        s, p, _ = self.mapper.match_scan2map(corner, surf, pose)
        return p

    def new_grids(self):
        return self.capi.Grid(self.mapper, 3.0, 0.2), self.capi.Grid(self.mapper, 3.0, 0.4)   # laser_mapping.cc:44-45,60-68


def synthetic_imu(poses_true, switch_at=50, seed=synth.SEED + 900, samples=45):
    """Per-scan IMU inputs for the replay (msfl_slam_imu): a synthetic pre-integration (45 samples over 0.11 s: a small steady
    rotation + drift, so that the de-skew passes change every point by millimetres), the estimator "initialised" from scan
    `switch_at` on (estimator.h:57: 50 scans), the pre-solved pose = the true pose nudged by a few millimetres (an IMU
    prediction that does not depend on earlier results, so the pipelined form can be fed without waiting)."""
    rng = np.random.default_rng(seed)
    out = []
    for k, pose in enumerate(poses_true):
        sum_dt = np.linspace(0.0, 0.11, samples)
        w = rng.normal(0, 0.02, 3)                                   # rad/s
        acc = rng.normal(0, 0.05, 3)
        v_body = rng.normal(0, 0.03, 3)
        ang = sum_dt[:, None] * w[None, :]
        half = 0.5 * np.linalg.norm(ang, axis=1)
        axis = w / max(np.linalg.norm(w), 1e-12)
        dq = np.c_[np.sin(half)[:, None] * axis[None, :], np.cos(half)]
        dp = v_body[None, :] * sum_dt[:, None] + 0.5 * acc[None, :] * sum_dt[:, None] ** 2
        init = k >= switch_at
        pres = pose.copy()
        pres[:3] += rng.normal(0, 0.004, 3)
        dth = rng.normal(0, 0.001, 3)
        q = synth.quat_mul(pose[3:], np.r_[0.5 * dth, 1.0])
        pres[3:] = q / np.linalg.norm(q)
        out.append(dict(sum_dt=sum_dt, delta_q=dq, delta_p=dp, is_initialized=init, velocity=rng.normal(0, 0.05, 3),
                        gravity=np.array([0.0, 0.0, 0.3]) + rng.normal(0, 0.01, 3), presolved_pose=pres))
    return out


def run(backend, world, poses_true, verbose=False, maps_out=None, scans=None, quirks=False, imu=None, clouds_out=None, new_grids=None,
        map_window=None, window_out=None):
    """new_grids: a factory of the two map stores (corner, surf) to use instead of backend.new_grids().
    map_window: (half_cells, every_n_scans) -> both stores are cropped (their crop(center, half_cells)) around the translation of
    pose_map after the inserts of every every_n_scans-th scan, like msfl_slam_set_map_window; window_out (a list) then receives per
    scan the (corner, surf) crop infos or None.
    quirks: FilterLessFlatLessCornerFeature as the reference executes it (laser_mapping.cc:340-364: the surf cloud cut to its first
    n_less_sharp points).  imu: per-scan dicts (synthetic_imu) -> UndistortScan before the match while not initialised
    (:170-176), the is_initialized matcher branch + DoUndistort before the insert afterwards (:197-211); needs a backend with
    undistort / deskew / scan2map_deskew (the oracle backend of the tests)."""
    # a backend may bring its own Rigid3d algebra (the oracle-driven loop of the tests uses the oracle's quaternion forms)
    compose_ = getattr(backend, "compose", compose)
    inverse_ = getattr(backend, "inverse", inverse)
    transform_ = getattr(backend, "transform", transform_cloud)
    n = len(poses_true)
    odo2first = np.array([0, 0, 0, 0, 0, 0, 1.0])        # pose_scan2world_ (odometry frame = first scan)
    curr2last = np.array([0, 0, 0, 0, 0, 0, 1.0])
    odom2map = poses_true[0].copy()                       # anchor the map frame at the true first pose
    grid_c, grid_s = new_grids() if new_grids is not None else backend.new_grids()   # hybrid_grid_map_corner_ / hybrid_grid_map_surf_
    last = None
    est, t_stage = [], dict(extract=0.0, odometry=0.0, voxel=0.0, surround=0.0, mapping=0.0, insert=0.0)
    for k in range(n):
        pts, ring = scans[k] if scans is not None else synth.make_scan(world, poses_true[k], synth.SEED + 5000 + k)
        t0 = time.perf_counter(); f = backend.extract(pts, ring); t1 = time.perf_counter()
        if last is not None:
            curr2last = backend.scan2scan(last, f, curr2last)                 # laser_odometry.cc:75 (guess = last delta)
            odo2first = compose_(odo2first, curr2last)                        # :79
        t2 = time.perf_counter()
        # ---- mapping thread (LaserMapping::Run): its own copies of the two clouds that reach the pose and the map
        ls, lf = f["full"][f["less_sharp"]], f["full"][f["less_flat"]]
        im = imu[k] if imu is not None else None
        if im is not None and im["sum_dt"] is None:
            im = None
        pre = (im["sum_dt"], im["delta_q"], im["delta_p"]) if im is not None else None
        if im is not None and not im["is_initialized"]:                        # UndistortScan, laser_mapping.cc:170-176
            ls, lf = backend.undistort(pre, ls), backend.undistort(pre, lf)
        if quirks:                                                            # FilterLessFlatLessCornerFeature, :186,340-364
            assert len(ls) <= len(lf), "the reference reads out of bounds here"
            lf = lf[:len(ls)]
        corner = backend.voxel(ls, 0.2)                                       # laser_mapping.cc:264-270
        surf = backend.voxel(lf, 0.4)
        t3 = time.perf_counter()
        pose_map = compose_(odom2map, odo2first)                              # TransformAssociateToMap, laser_mapping.h:55-57
        map_c = grid_c.get_surrounded(ls, pose_map)                           # GetSurroundedCloud on the UN-down-sampled
        map_s = grid_s.get_surrounded(lf, pose_map)                           # feature clouds, laser_mapping.cc:273-278
        t3b = time.perf_counter()
        if len(map_c) > 10 and len(map_s) > 50:                               # gate, laser_mapping.cc:284-285
            if im is not None and im["is_initialized"]:                       # mapping_scan_matcher.cc:28-59: start from the pre-solve
                pose_map = backend.scan2map_deskew(map_c, map_s, corner, surf, pre, im["velocity"], im["gravity"],
                                                   np.array(im["presolved_pose"], np.float64))
            else:
                pose_map = backend.scan2map(map_c, map_s, corner, surf, pose_map)
        t4 = time.perf_counter()
        odom2map = compose_(pose_map, inverse_(odo2first))                    # TransformUpdate, laser_mapping.h:59-61
        if im is not None and im["is_initialized"]:                           # DoUndistort, laser_mapping.cc:197-211 (pose_odom_scan2world_!)
            ls = backend.deskew(pre, ls, odo2first[3:], im["velocity"], im["gravity"])
            lf = backend.deskew(pre, lf, odo2first[3:], im["velocity"], im["gravity"])
        if clouds_out is not None:
            # the data products that reach neither the pose nor the map: cloud_full_res after the scan's IMU passes (UndistortScan
            # :170-176 / DoUndistort :206) and TransformPointCloud(cloud_full_res, pose_map_scan2world_) (:214-217)
            full = f["full"]
            if im is not None and not im["is_initialized"]:
                full = backend.undistort(pre, full)
            elif im is not None:
                full = backend.deskew(pre, full, odo2first[3:], im["velocity"], im["gravity"])
            clouds_out.append(dict(full_scan=full, full_map=transform_(pose_map, full), ring=f["ring"], sharp=f["sharp"], less_sharp=f["less_sharp"],
                                   flat=f["flat"], less_flat=f["less_flat"]))
        grid_c.insert_scan(transform_(pose_map, ls))                          # InsertScan2Map, laser_mapping.cc:330-338
        grid_s.insert_scan(transform_(pose_map, lf))
        if map_window is not None:                                            # the windowed local map: forget what lies outside
            infos = None
            if (k + 1) % map_window[1] == 0:
                infos = (grid_c.crop(pose_map[:3], map_window[0]), grid_s.crop(pose_map[:3], map_window[0]))
            if window_out is not None:
                window_out.append(infos)
        t5 = time.perf_counter()
        last = f
        est.append(pose_map)
        for name, dt in (("extract", t1 - t0), ("odometry", t2 - t1), ("voxel", t3 - t2), ("surround", t3b - t3),
                         ("mapping", t4 - t3b), ("insert", t5 - t4)):
            if k >= 2:
                t_stage[name] += dt
        if verbose and k % 20 == 0:
            print(k, synth.pose_error(pose_map, poses_true[k]), grid_c.size(), grid_s.size(), file=sys.stderr)
    m = max(n - 2, 1)
    if maps_out is not None:
        maps_out["corner"], maps_out["surf"] = grid_c.dump(), grid_s.dump()
    return np.array(est), {k: 1e3 * v / m for k, v in t_stage.items()}


def world_drive(world, kind, n):
    """A drive through the outdoor / corridor world (~0.4 m and a degree or two per scan): down the x = 0 street following the relief, or
    down the corridor's axis (the same drives as tests/common.py:world_drive; wraps around after ~125 scans so that any length stays inside)."""
    poses = []
    for k in range(n):
        if kind == "outdoor":
            kk = k % 250
            kk = kk if kk < 125 else 250 - kk                        # there and back again
            y = -25.0 + 0.4 * kk
            x = 1.2 * np.sin(0.11 * kk)
            yaw = np.pi / 2 - np.arctan(1.2 * 0.11 * np.cos(0.11 * kk) / 0.4) * 0.5
            z = float(world.geom.ground(x, y)) + 1.8 + 0.02 * np.sin(0.5 * kk)
            poses.append(np.r_[x, y, z, synth.quat_from_euler(0.015 * np.sin(0.3 * kk), 0.01 * np.cos(0.2 * kk), yaw)])
        else:
            kk = k % 250
            kk = kk if kk < 125 else 250 - kk
            poses.append(np.r_[-20.0 + 0.4 * kk, 0.3 * np.sin(0.15 * kk), 1.5 + 0.02 * np.sin(0.4 * kk),
                               synth.quat_from_euler(0.01 * np.sin(0.3 * kk), 0.01 * np.cos(0.25 * kk), 0.05 * np.sin(0.2 * kk))])
    return np.array(poses)


def run_slam(world, poses_true, pipelined=False, device=0, scans=None, verbose=False, maps_out=None, quirks=False, imu=None, clouds_out=None,
             uncertainty=None, unc_out=None, priors=None, map_window=None, window_out=None, slam_hook=None, load_map=None, save_map=None,
             degeneracy=None, degen_out=None, reject=None, reject_out=None, start_pose=None):
    """The same loop through the device-resident SLAM step (msfl_slam_add_scan): raw scan in, pose out, one
    synchronisation per scan (pipelined=False) or none until the record is fetched one scan later (pipelined=True: the
    odometry chain of scan k + 1 runs under the mapping chain of scan k, like the reference's two threads).
    uncertainty: a min_eigenvalue turns msfl_slam_set_uncertainty on; unc_out (a list) then receives per scan the (odometry, mapping)
    records of msfl_slam_get_uncertainty.
    priors: per scan None or an (odometry, mapping) pair for msfl_slam_set_next_prior, each None or (pose7, sqrt_information 6 x 6).
    degeneracy: (min_eig_odometry, min_eig_mapping), either None = that matcher off, turns msfl_slam_set_degeneracy on; degen_out (a list)
    then receives per scan the (odometry, mapping) records of msfl_slam_get_degeneracy.
    reject: (odometry, mapping), each None = that matcher off or a capi.OutlierRejection, turns msfl_slam_set_outlier_rejection on; reject_out
    (a list) then receives per scan the (odometry, mapping) records of msfl_slam_get_rejection.
    map_window: (half_cells, every_n_scans) for msfl_slam_set_map_window; window_out (a list) then receives per scan the (corner, surf)
    records of msfl_slam_get_map_window.  slam_hook(slam, k): called before scan k is fed.
    load_map: PREFIX -> PREFIX.corner.npz / PREFIX.surf.npz (msf_loam_amd/mapio.py) are loaded into the session's two stores before the
    first scan (msfl_grid_load_cells: the stores hold the saved cells bit for bit, and scan 0 is registered against them); poses_true[0]
    is then the pose of the first scan in the saved map's frame, unless start_pose (relocalize_start) gives it.  save_map: PREFIX -> the two stores are written there after the run.
    Returns (poses, records, wall-clock ms per scan over the scans after the second)."""
    from msf_loam_amd import capi
    n = len(poses_true)
    if scans is None:
        scans = [synth.make_scan(world, poses_true[k], synth.SEED + 5000 + k) for k in range(n)]
    cap = max(len(p) for p, _ in scans)
    rings = int(max(r.max() for _, r in scans)) + 1
    if os.environ.get("MSFL_REPLAY_DEFAULT_CAPS") == "1":          # msfl_slam_default_config's launch bounds (200 000 points, 128 rings) instead of tight ones
        cap, rings = 200000, 128
    slam = capi.Slam(device, max_scan_points=cap, max_rings=rings, pose_odom2map=poses_true[0] if start_pose is None else start_pose,
                     reference_quirks=1 if quirks else 0, keep_clouds=1 if clouds_out is not None else 0)
    if uncertainty is not None:
        slam.set_uncertainty(True, uncertainty)
    want_unc = uncertainty is not None and unc_out is not None
    if degeneracy is not None:
        slam.set_degeneracy(odometry=degeneracy[0], mapping=degeneracy[1])
    want_degen = degeneracy is not None and degen_out is not None
    if reject is not None:
        slam.set_outlier_rejection(odometry=reject[0], mapping=reject[1])
    want_reject = reject is not None and reject_out is not None
    if map_window is not None:
        slam.set_map_window(map_window[0], map_window[1])
    want_win = window_out is not None
    if load_map is not None:
        from msf_loam_amd import mapio
        for grid, side in zip(slam.grids(), ("corner", "surf")):
            mapio.load_grid("%s.%s.npz" % (load_map, side), grid)
    recs = [None] * n
    t_start = None
    for k in range(n):
        if k == 2:
            t_start = time.perf_counter()
        im = imu[k] if imu is not None else None
        if slam_hook is not None:
            slam_hook(slam, k)
        if priors is not None and priors[k] is not None:
            slam.set_next_prior(odometry=priors[k][0], mapping=priors[k][1])
        if pipelined:
            slam.add_scan(*scans[k], wait=False, imu=im)
            if k >= 1:
                recs[k - 1] = slam.result(k - 1)
                if want_unc:
                    unc_out.append(slam.get_uncertainty(k - 1))
                if want_degen:
                    degen_out.append(slam.get_degeneracy(k - 1))
                if want_reject:
                    reject_out.append(slam.get_rejection(k - 1))
                if want_win:
                    window_out.append(slam.get_map_window(k - 1))
                if clouds_out is not None:
                    clouds_out.append(slam.clouds(k - 1))
        else:
            recs[k] = slam.add_scan(*scans[k], imu=im)
            if want_unc:
                unc_out.append(slam.get_uncertainty(k))
            if want_degen:
                degen_out.append(slam.get_degeneracy(k))
            if want_reject:
                reject_out.append(slam.get_rejection(k))
            if want_win:
                window_out.append(slam.get_map_window(k))
            if clouds_out is not None:
                clouds_out.append(slam.clouds(k))
        if verbose and k % 50 == 0 and recs[max(k - 1, 0)] is not None:
            r = recs[max(k - 1, 0)]
            print(k, list(r.grid_corner)[:3], list(r.grid_surf)[:3], r.status_mapping, file=sys.stderr)
    if pipelined:
        recs[n - 1] = slam.result(n - 1)
        if want_unc:
            unc_out.append(slam.get_uncertainty(n - 1))
        if want_degen:
            degen_out.append(slam.get_degeneracy(n - 1))
        if want_reject:
            reject_out.append(slam.get_rejection(n - 1))
        if want_win:
            window_out.append(slam.get_map_window(n - 1))
        if clouds_out is not None:
            clouds_out.append(slam.clouds(n - 1))
    wall = time.perf_counter() - t_start if t_start is not None else 0.0
    est = np.array([np.array(r.pose_map[:]) for r in recs])
    if maps_out is not None:
        gc_, gs_ = slam.grids()
        maps_out["corner"], maps_out["surf"] = gc_.dump(), gs_.dump()
    if save_map is not None:
        from msf_loam_amd import mapio
        for grid, side in zip(slam.grids(), ("corner", "surf")):
            mapio.save_grid("%s.%s.npz" % (save_map, side), grid)
    slam.close()
    return est, recs, 1e3 * wall / max(n - 2, 1)


def run_slam_segmented(poses_true, scans, device=0, config=None):
    """--segment: every sweep goes to the device once; msfl_segment_scan masks it there (ground and range-image clusters, the rest
    set to NaN) and msfl_slam_add_scan takes the masked device cloud, so no cloud comes back to the host.  The session runs on a
    stream of its own: the read-back of the class counts is the one wait between the handle's stream and the session's.
    Returns (poses, records, ms per scan over the scans after the second, class counts)."""
    import torch
    from msf_loam_amd import capi
    dev = "cuda:%d" % device
    torch.zeros(1, device=dev)
    h = capi.Handle(device)
    cap = max(len(p) for p, _ in scans)
    rings = int(max(r.max() for _, r in scans)) + 1
    slam = capi.Slam(device, max_scan_points=cap, max_rings=rings, pose_odom2map=poses_true[0])
    counts = np.zeros(5, np.int64)
    recs, t_start = [], None
    for k, (pts, ring) in enumerate(scans):
        if k == 2:
            t_start = time.perf_counter()
        d_pts = torch.from_numpy(np.ascontiguousarray(pts)).to(dev)
        d_ring = torch.from_numpy(np.ascontiguousarray(ring).view(np.int16)).to(dev)
        out = h.segment_scan(d_pts, d_ring, config, want_segment=False)
        counts += out["info"]["n_class"]
        recs.append(slam.add_scan_device(out["masked"], d_ring, len(pts)))          # waits for the result: the tensors may go after it
    wall = time.perf_counter() - t_start if t_start is not None else 0.0
    est = np.array([np.array(r.pose_map[:]) for r in recs])
    slam.close(); h.close()
    return est, recs, 1e3 * wall / max(len(scans) - 2, 1), counts


def ate(est, truth):
    return float(np.sqrt(np.mean(np.sum((est[:, :3] - truth[:, :3]) ** 2, axis=1))))


def relocalize_start(prefix, scan, truth0, offset=(1.2, -0.9), yaw_deg=34.0, device=0):
    """The pose of `scan` in the saved map PREFIX.corner.npz / PREFIX.surf.npz, found by msfl_relocalize from a guess `offset` metres
    and yaw_deg degrees off truth0: features through the product's extraction and voxel filter, the map files' points as the
    resident map, the default 13 x 13 x 24 lattice."""
    from msf_loam_amd import capi, mapio
    mc, ms = (mapio.read_map("%s.%s.npz" % (prefix, side))[3] for side in ("corner", "surf"))
    h = capi.Handle(device)
    f = h.extract_features(*scan)
    corner = h.voxel_downsample(f["full"][f["less_sharp"]], 0.2)
    surf = h.voxel_downsample(f["full"][f["less_flat"]], 0.4)
    guess = np.array(truth0, np.float64)
    guess[0] += offset[0]; guess[1] += offset[1]
    hy = -np.deg2rad(yaw_deg) / 2.0
    q = synth.quat_mul(np.array([0.0, 0.0, np.sin(hy), np.cos(hy)]), guess[3:])
    guess[3:] = q / np.linalg.norm(q)
    reach = float(np.ceil(np.percentile(np.linalg.norm(np.concatenate([corner, surf])[:, :3], axis=1), 99)))
    h.set_map(mc, ms)
    res = h.relocalize(corner, surf, guess, capi.SearchConfig(range=reach), n_candidates=16, max_dist=1.0, n_refine=5, min_fitness=0.5)
    h.close()
    if len(res) == 0 or not res[0]["accepted"]:
        raise SystemExit("--relocalize: no candidate reached the fitness 0.5")
    dt, dr = synth.pose_error(res[0]["pose"], truth0)
    print("relocalised scan 0 from a guess %.2f m / %.0f deg off: %.3f m / %.2f deg from the truth, fitness %.3f"
          % (np.hypot(*offset), yaw_deg, dt, np.rad2deg(dr), capi.fitness(res["refined"][:1], len(corner), len(surf))[0]), file=sys.stderr)
    return np.array(res[0]["pose"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=300)
    ap.add_argument("--mode", choices=["slam", "slam-pipelined", "staged"], default="slam",
                    help="slam: msfl_slam_add_scan, one synchronisation per scan; slam-pipelined: results fetched one scan late; "
                         "staged: the round-2 loop of single-stage host-pointer calls")
    ap.add_argument("--dump-poses", default=None, help="write the estimated map poses (n x 7 float64, .npy) here")
    ap.add_argument("--reference-quirks", action="store_true", help="msfl_slam_config.reference_quirks = 1 (surf list truncation of the reference)")
    ap.add_argument("--imu", action="store_true", help="feed a synthetic pre-integration with every scan (UndistortScan, then the is_initialized branch from scan 50)")
    ap.add_argument("--world", choices=["room", "outdoor", "corridor"], default="room",
                    help="room: the SURVEY 8d world and its loop; outdoor / corridor: msf_loam_amd/worlds.py with a drive down the street / the axis (round 5)")
    ap.add_argument("--beams", type=int, choices=[16, 64], default=16, help="64: the KITTI-scale sensor of BASELINE configs[3] (64 x 1 900, -24.8 .. +2 degrees)")
    ap.add_argument("--keep-clouds", action="store_true", help="msfl_slam_config.keep_clouds = 1 and fetch every scan's clouds (what PublishScan would publish)")
    ap.add_argument("--uncertainty", type=float, nargs="?", const=150.0, default=None, metavar="MIN_EIGENVALUE",
                    help="msfl_slam_set_uncertainty: print per scan the smallest eigenvalue of the mapping solve's information matrix, n_degenerate "
                         "at this threshold (default 150) and the weakest direction [dt(3), dtheta(3)]")
    ap.add_argument("--degeneracy", default=None, metavar="MIN_EIG_ODOM,MIN_EIG_MAP",
                    help="msfl_slam_set_degeneracy: both matchers hold the eigen-directions of their entry matrix below the given threshold at the "
                         "guess (solution remapping); prints per scan n_held of the two outer iterations of both matchers")
    ap.add_argument("--reject", default=None, metavar="threshold:T | fraction:F",
                    help="msfl_slam_set_outlier_rejection on both matchers, in front of the last outer iteration's solve: threshold:0.2 rejects "
                         "correspondences whose residual norm exceeds 0.2, fraction:0.15 the 15 %% largest of every scan; prints per scan what went")
    ap.add_argument("--map-window", default=None, metavar="HX,HY,HZ[,N]",
                    help="msfl_slam_set_map_window: crop both map stores to +-HX,HY,HZ cells around the pose after every N-th scan (default 1); "
                         "23,23,23 is the smallest window that takes nothing from the registration of the scan at its centre")
    ap.add_argument("--save-map", default=None, metavar="PREFIX",
                    help="after the run write the two map stores to PREFIX.corner.npz / PREFIX.surf.npz (msfl_grid_dump_cells + msfl_grid_dump)")
    ap.add_argument("--load-map", default=None, metavar="PREFIX",
                    help="before the first scan load PREFIX.corner.npz / PREFIX.surf.npz into the session's stores (msfl_grid_load_cells): "
                         "localise in a saved map; the first true pose anchors the session in the saved map's frame")
    ap.add_argument("--relocalize", action="store_true",
                    help="with --load-map: the session is not anchored at the first true pose but at what msfl_relocalize finds for scan 0 "
                         "in the saved map from a guess 1.5 m and 34 degrees off (examples/relocalize.py shows the search on its own)")
    ap.add_argument("--segment", action="store_true",
                    help="after the run, replay the same scans once more with msfl_segment_scan in front: the masked device cloud goes "
                         "into msfl_slam_add_scan; the JSON line gains a `segment` record (class counts, ATE, ms per scan)")
    args = ap.parse_args()
    if args.mode == "staged" and (args.save_map or args.load_map):
        ap.error("--save-map / --load-map need the slam modes")
    if args.relocalize and not args.load_map:
        ap.error("--relocalize needs --load-map")
    map_window = None
    if args.map_window:
        w = [int(v) for v in args.map_window.split(",")]
        if len(w) not in (3, 4):
            ap.error("--map-window takes HX,HY,HZ[,N]")
        map_window = (tuple(w[:3]), w[3] if len(w) == 4 else 1)
    degeneracy = None
    if args.degeneracy:
        d = [float(v) for v in args.degeneracy.split(",")]
        if len(d) != 2:
            ap.error("--degeneracy takes MIN_EIG_ODOM,MIN_EIG_MAP")
        degeneracy = tuple(d)
    reject = None
    if args.reject:
        from msf_loam_amd import capi
        kind, _, value = args.reject.partition(":")
        if kind not in ("threshold", "fraction") or not value:
            ap.error("--reject takes threshold:T or fraction:F")
        cfg = capi.outlier_rejection(**{kind: float(value)})
        reject = (cfg, cfg)
    if args.world == "room":
        world = synth.World(ground_half=45.0)
        truth = trajectory(args.scans)
    else:
        world = synth.World(kind=args.world)
        truth = world_drive(world, args.world, args.scans)
    if args.mode == "staged":
        est, ms = run(GpuBackend(0), world, truth, verbose=True)
        print(json.dumps({"mode": "staged", "scans": args.scans, "ate_rmse_m": ate(est, truth),
                          "final_error_m_rad": synth.pose_error(est[-1], truth[-1]),
                          "latency_ms_per_scan": ms, "note": "single-scan host-pointer calls (includes PCIe staging)"}))
        return
    kw = dict(n_beams=64, n_az=1900, elev=(-24.8, 2.0)) if args.beams == 64 else {}
    scans = [synth.make_scan(world, truth[k], synth.SEED + 5000 + k, **kw) for k in range(args.scans)]
    import gc
    gc.collect(); gc.disable()
    unc, degen, rejected = [], [], []
    if args.segment:                                       # torch holds the segmented replay's device clouds, and has to initialise first
        import torch
        torch.zeros(1, device="cuda:0")
    start_pose = relocalize_start(args.load_map, scans[0], truth[0]) if args.relocalize else None
    est, recs, ms = run_slam(world, truth, pipelined=args.mode == "slam-pipelined", scans=scans, quirks=args.reference_quirks, start_pose=start_pose,
                             imu=synthetic_imu(truth) if args.imu else None, clouds_out=[] if args.keep_clouds else None,
                             uncertainty=args.uncertainty, unc_out=unc, map_window=map_window, load_map=args.load_map, save_map=args.save_map,
                             degeneracy=degeneracy, degen_out=degen, reject=reject, reject_out=rejected)
    for k, (o, m) in enumerate(rejected):
        print("scan %4d  rejected edges / planes of the last solve: odometry %d of %d / %d of %d  mapping %d of %d / %d of %d" %
              (k, o["n_edge_rejected"][1], o["n_edge_in"][1], o["n_plane_rejected"][1], o["n_plane_in"][1],
               m["n_edge_rejected"][1], m["n_edge_in"][1], m["n_plane_rejected"][1], m["n_plane_in"][1]), file=sys.stderr)
    for k, (o, m) in enumerate(degen):
        print("scan %4d  n_held odometry %s mapping %s  lambda_min of the mapping solves %s" %
              (k, list(o["n_held"]), list(m["n_held"]), np.array2string(m["eigenvalues"][:, 0], precision=2)), file=sys.stderr)
    for k, u in enumerate(unc):
        m = u[1]
        if m["valid"]:
            print("scan %4d  lambda_min %10.2f  n_degenerate %d  weakest %s" % (k, m["eigenvalues"][0], m["n_degenerate"], np.array2string(m["eigenvectors"][0], precision=3, suppress_small=True)), file=sys.stderr)
        else:
            print("scan %4d  no mapping solve" % k, file=sys.stderr)
    last = recs[-1]
    if args.dump_poses:
        np.save(args.dump_poses, est)
    extra = {}
    if args.segment:
        from msf_loam_amd import capi
        seg_cfg = capi.SegmentConfig(n_col=1900, n_row=64, elev_low_deg=-24.8, elev_high_deg=2.0, ground_rows=50) if args.beams == 64 else None
        est_s, recs_s, ms_s, counts = run_slam_segmented(truth, scans, config=seg_cfg)
        extra["segment"] = {"class_counts": {name: int(c) for name, c in zip(capi.SEG_CLASS_NAMES, counts)}, "n_points": int(sum(len(p) for p, _ in scans)),
                            "ate_m": ate(est_s, truth), "final_error_m_rad": synth.pose_error(est_s[-1], truth[-1]), "ms_per_scan_end_to_end": ms_s,
                            "mapping_gate_closed_scans": int(sum(1 for r in recs_s if r.status_mapping != 0)),
                            "mean_features_after_voxel": [float(np.mean([r.n_corner_ds for r in recs_s])), float(np.mean([r.n_surf_ds for r in recs_s]))],
                            "note": "the scan goes to the device once (18 B/pt), is masked there and enters msfl_slam_add_scan as device memory"}
    print(json.dumps({**extra, "mode": args.mode, "world": args.world, "beams": args.beams, "keep_clouds": bool(args.keep_clouds), "scans": args.scans, "reference_quirks": bool(args.reference_quirks), "imu": bool(args.imu),
                      "map_window": args.map_window, "degeneracy": args.degeneracy, "reject": args.reject, "load_map": args.load_map, "save_map": args.save_map,
                      "ate_rmse_m": ate(est, truth),
                      "final_error_m_rad": synth.pose_error(est[-1], truth[-1]), "ms_per_scan_end_to_end": ms,
                      "scans_per_s": 1e3 / ms if ms else None,
                      "map_points": [last.grid_corner[0], last.grid_surf[0]], "map_cells": [last.grid_corner[1], last.grid_surf[1]],
                      "mapping_gate_closed_scans": int(sum(1 for r in recs if r.status_mapping != 0)),
                      "mean_features_after_voxel": [float(np.mean([r.n_corner_ds for r in recs])), float(np.mean([r.n_surf_ds for r in recs]))],
                      "mean_surrounded_map_points": [float(np.mean([r.n_map_corner for r in recs])), float(np.mean([r.n_map_surf for r in recs]))],
                      "note": "raw host scan in (18 B/pt over PCIe), 480-byte record out; wall clock around the calls"}))


if __name__ == "__main__":
    main()
