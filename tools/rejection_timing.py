"""Timed leg of outlier rejection (docs/kernels/rejection.md), feature on against off, and what it buys on displaced features:

  timing   the registration step of bench.py (map index + B scans registered, device resident) in the room world, HIP events around
           it, with the feature off / threshold 0.2 / fraction 0.15 alternated three times (LAST_OUTER, no record sink: the timed
           path writes no records); the added time per step is set against the solve launches of the same process (msfl_get_timing)
  effect   64 room-world registrations in which 10 % of every scan's surf features are displaced 0.3 m along their ray (an object
           that was not there when the map was made): translation / rotation error against the truth, feature off and on

  python tools/rejection_timing.py [scans] [copies] [reps]   default: 256 4 20

Prints one JSON line.  Figures only: nothing here checks a result (tests/test_gpu_rejection.py does).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = {"off": None, "threshold": dict(threshold=0.2), "fraction": dict(fraction=0.15)}


def _pipeline(h, dev, world, truth, copies, seed=7):
    from msf_loam_amd import synth
    from msf_loam_amd.pipeline import BatchPipeline
    rng = np.random.default_rng(seed)
    sweeps = [synth.make_scan(world, truth[i], synth.SEED + 10 + i) for i in range(len(truth))]
    pts, ring, off, guess = [], [], [0], []
    for _ in range(copies):
        for i in range(len(truth)):
            pts.append(sweeps[i][0]); ring.append(sweeps[i][1]); off.append(off[-1] + len(sweeps[i][0]))
            guess.append(synth.perturb_pose(truth[i], rng))
    pipe = BatchPipeline(h, np.concatenate(pts), np.concatenate(ring), np.array(off, np.int32), dev)
    return pipe, np.array(guess)


def _select(h, name, sink=None, capacity=0):
    if LEGS[name] is None:
        h.clear_outlier_rejection()
    elif sink is not None:
        h.set_outlier_rejection_device(sink, capacity, **LEGS[name])
    else:
        h.set_outlier_rejection(n=0, **LEGS[name])


def run(scans=256, copies=4, reps=20):
    import torch
    from msf_loam_amd import capi, synth
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    world = synth.World(ground_half=synth.ground_half_for_target(50000))
    mc, ms = synth.make_map(world)
    h = capi.Handle(0)
    h.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"registrations": scans * copies, "reps": reps}

    # ---- timing ----
    truth = synth.world_poses(world, scans, synth.SEED + 2)
    pipe, guess = _pipeline(h, dev, world, truth, copies)
    pipe.set_map(mc, ms)
    pipe.extract(); pipe.voxel()
    d_guess = torch.from_numpy(guess).to(dev)

    def timed(k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(k):
            pipe.register(d_guess)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / k

    legs = {name: [] for name in LEGS}
    for rnd in range(3):                                   # alternated: drift of the machine shows up as spread, not as a difference
        for name in LEGS:
            _select(h, name)
            timed(2)
            legs[name].append(timed(reps))
    for name in LEGS:
        out["ms_per_step_" + name] = legs[name]
    # the solve launches of the same process, feature off (HIP events per kernel class)
    _select(h, "off")
    h.set_timing(1)
    h.get_timing(reset=True)
    for _ in range(reps):
        pipe.register(d_guess)
    t = h.get_timing(reset=True)
    h.set_timing(0)
    out["ms_solve_per_step_off"] = t.ms_solve / reps
    out["solve_launches_per_step"] = t.launches_solve / reps
    for name in ("threshold", "fraction"):
        out["added_ms_per_step_" + name] = float(np.median(legs[name]) - np.median(legs["off"]))
        out["added_over_solve_" + name] = out["added_ms_per_step_" + name] / out["ms_solve_per_step_off"]

    # ---- effect: 64 registrations, 10 % of the surf features displaced 0.3 m along their ray ----
    n = 64
    truth64 = truth[:n]
    pipe, guess = _pipeline(h, dev, world, truth64, 1, seed=11)
    pipe.set_map(mc, ms)
    pipe.extract(); pipe.voxel()
    rng = np.random.default_rng(99)
    so = np.asarray(pipe.surf_off)
    pick = np.concatenate([so[b] + rng.choice(so[b + 1] - so[b], (so[b + 1] - so[b]) // 10, replace=False) for b in range(n)])
    d_pick = torch.from_numpy(pick.astype(np.int64)).to(dev)
    p = pipe.d_surf[d_pick, :3]
    pipe.d_surf[d_pick, :3] = p - 0.3 * p / p.norm(dim=1, keepdim=True)
    d_guess = torch.from_numpy(guess).to(dev)
    d_rec = torch.zeros(n * capi.REJECTION_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    out["displaced_surf_features"] = int(len(pick))
    for name in LEGS:
        _select(h, name, sink=d_rec if LEGS[name] else None, capacity=n)
        pipe.register(d_guess)
        torch.cuda.synchronize()
        poses = pipe.d_poses.cpu().numpy()
        err = np.array([synth.pose_error(poses[b], truth64[b]) for b in range(n)])
        out["pose_error_" + name] = {"dt_mean_m": float(err[:, 0].mean()), "dt_max_m": float(err[:, 0].max()),
                                     "dr_mean_rad": float(err[:, 1].mean()), "dr_max_rad": float(err[:, 1].max())}
        if LEGS[name]:
            rec = np.frombuffer(d_rec.cpu().numpy().tobytes(), capi.REJECTION_DTYPE)
            out["rejected_" + name] = int(rec["n_edge_rejected"].sum() + rec["n_plane_rejected"].sum())
            out["entering_" + name] = int(rec["n_edge_in"][:, 1].sum() + rec["n_plane_in"][:, 1].sum())
    h.clear_outlier_rejection()
    h.close()
    return out


if __name__ == "__main__":
    print(json.dumps(run(*(int(x) for x in sys.argv[1:4]))))
