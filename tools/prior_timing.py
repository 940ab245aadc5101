"""Timed leg of the pose prior (docs/kernels/prior.md), feature on against off:

  the registration step of bench.py (map index + B scans registered, device resident) in one world, one prior record per
  registration in device memory (msfl_set_pose_prior with MSFL_MEM_DEVICE: read on the handle's stream, nothing synchronised).
  `on` launches lm_solve_prior_kernel, `off` the plain lm_solve_kernel; `zero` launches the prior kernel with all-zero records
  (the explicit skip branch: the cost of staging the record alone).

  python tools/prior_timing.py [room|outdoor|corridor] [scans] [copies] [reps]        default: room 256 4 20 = 1 024 registrations

Prints one JSON line.  Timings only: nothing here checks a result (tests/test_gpu_pose_prior.py does).
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batch(kind="room", scans=256, copies=4, reps=20):
    import torch
    from msf_loam_amd import capi, synth
    from msf_loam_amd.pipeline import BatchPipeline
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    world = synth.World(ground_half=synth.ground_half_for_target(50000)) if kind == "room" else synth.World(kind=kind)
    mc, ms = synth.make_map(world)
    truth = synth.world_poses(world, scans, synth.SEED + 2)
    rng = np.random.default_rng(7)
    pts, ring, off, guess, mean = [], [], [0], [], []
    sweeps = [synth.make_scan(world, truth[i], synth.SEED + 10 + i) for i in range(scans)]
    for _ in range(copies):
        for i in range(scans):
            pts.append(sweeps[i][0]); ring.append(sweeps[i][1]); off.append(off[-1] + len(sweeps[i][0]))
            guess.append(synth.perturb_pose(truth[i], rng))
            mean.append(synth.perturb_pose(truth[i], rng, max_t=0.05, max_deg=0.5))
    B = scans * copies
    h = capi.Handle(0)
    h.set_stream(torch.cuda.current_stream().cuda_stream)
    pipe = BatchPipeline(h, np.concatenate(pts), np.concatenate(ring), np.array(off, np.int32), dev)
    pipe.set_map(mc, ms)
    pipe.extract(); pipe.voxel()
    d_guess = torch.from_numpy(np.array(guess)).to(dev)
    # sqrt_information: 5 cm / 1 degree, diagonal (the cost of the block does not depend on its values)
    L = np.diag([1 / 0.05] * 3 + [1 / np.deg2rad(1.0)] * 3)
    rec = capi.pose_priors(np.array(mean), np.tile(L, (B, 1, 1)))
    zero = capi.pose_priors(np.array(mean), np.zeros((B, 6, 6)))
    d_prior = {"on": torch.from_numpy(np.frombuffer(rec.tobytes(), np.uint8).copy()).to(dev),
               "zero": torch.from_numpy(np.frombuffer(zero.tobytes(), np.uint8).copy()).to(dev)}

    def select(name):
        if name == "off":
            h.clear_pose_prior()
        else:
            h.set_pose_prior_device(d_prior[name], B)

    def timed(k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            pipe.register(d_guess)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / k

    out = {"world": kind, "registrations": B, "reps": reps}
    legs = {"off": [], "on": [], "zero": []}
    for rnd in range(3):                                   # alternated: drift of the box shows up as spread, not as a difference
        for name in ("off", "on", "zero"):
            select(name)
            timed(2)
            legs[name].append(timed(reps))
    poses = {}
    for name in ("off", "on", "zero"):
        select(name)
        pipe.register(d_guess); torch.cuda.synchronize()
        poses[name] = pipe.d_poses.cpu().numpy().copy()
    for name in legs:
        out["ms_per_step_" + name] = legs[name]
    out["zero_bit_identical_to_off"] = bool(np.array_equal(poses["zero"], poses["off"]))
    out["on_moves_the_poses"] = bool(not np.array_equal(poses["on"], poses["off"]))
    h.clear_pose_prior()
    h.close()
    return out


if __name__ == "__main__":
    a = sys.argv[1:]
    print(json.dumps(batch(a[0] if a else "room", *(int(x) for x in a[1:4]))))
