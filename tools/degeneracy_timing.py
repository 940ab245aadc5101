"""Timed leg of the degeneracy-aware solve (docs/kernels/degeneracy.md), feature on against off:

  the registration step of bench.py (map index + B scans registered, device resident) in one world.  `off` launches the plain
  lm_solve_kernel; `none` launches lm_solve_degen_kernel with threshold 0 (nothing is held: the cost of the decomposition at the
  start of every solve alone); `held` launches it with MIN_EIGENVALUE (directions below it are held: the rotation after every
  reduction and the mapped step on top).  No record sink: the timed path writes no records.

  python tools/degeneracy_timing.py [room|outdoor|corridor] [min_eigenvalue] [scans] [copies] [reps]   default: room 150 256 4 20

Prints one JSON line.  Timings only: nothing here checks a result (tests/test_gpu_degeneracy.py does).
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batch(kind="room", min_eigenvalue=150.0, scans=256, copies=4, reps=20):
    import torch
    from msf_loam_amd import capi, synth
    from msf_loam_amd.pipeline import BatchPipeline
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    world = synth.World(ground_half=synth.ground_half_for_target(50000)) if kind == "room" else synth.World(kind=kind)
    mc, ms = synth.make_map(world)
    truth = synth.world_poses(world, scans, synth.SEED + 2)
    rng = np.random.default_rng(7)
    pts, ring, off, guess = [], [], [0], []
    sweeps = [synth.make_scan(world, truth[i], synth.SEED + 10 + i) for i in range(scans)]
    for _ in range(copies):
        for i in range(scans):
            pts.append(sweeps[i][0]); ring.append(sweeps[i][1]); off.append(off[-1] + len(sweeps[i][0]))
            guess.append(synth.perturb_pose(truth[i], rng))
    B = scans * copies
    h = capi.Handle(0)
    h.set_stream(torch.cuda.current_stream().cuda_stream)
    pipe = BatchPipeline(h, np.concatenate(pts), np.concatenate(ring), np.array(off, np.int32), dev)
    pipe.set_map(mc, ms)
    pipe.extract(); pipe.voxel()
    d_guess = torch.from_numpy(np.array(guess)).to(dev)
    d_rec = torch.zeros(B * capi.DEGENERACY_DTYPE.itemsize, dtype=torch.uint8, device=dev)

    def select(name, sink=False):
        if name == "off":
            h.clear_degeneracy()
        elif sink:
            h.set_degeneracy_device(0.0 if name == "none" else min_eigenvalue, d_rec, B)
        else:
            h.set_degeneracy(0.0 if name == "none" else min_eigenvalue, 0)

    def timed(k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            pipe.register(d_guess)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / k

    out = {"world": kind, "registrations": B, "reps": reps, "min_eigenvalue": min_eigenvalue}
    legs = {"off": [], "none": [], "held": []}
    for rnd in range(3):                                   # alternated: drift of the box shows up as spread, not as a difference
        for name in ("off", "none", "held"):
            select(name)
            timed(2)
            legs[name].append(timed(reps))
    poses = {}
    for name in ("off", "none", "held"):
        select(name, sink=True)
        pipe.register(d_guess); torch.cuda.synchronize()
        poses[name] = pipe.d_poses.cpu().numpy().copy()
        if name != "off":
            rec = np.frombuffer(d_rec.cpu().numpy().tobytes(), capi.DEGENERACY_DTYPE)
            out["registrations_with_held_directions_" + name] = int((rec["n_held"].sum(1) > 0).sum())
            out["held_directions_" + name] = int(rec["n_held"].sum())
    for name in legs:
        out["ms_per_step_" + name] = legs[name]
    out["none_bit_identical_to_off"] = bool(np.array_equal(poses["none"], poses["off"]))
    out["held_moves_the_poses"] = bool(not np.array_equal(poses["held"], poses["off"]))
    h.clear_degeneracy()
    h.close()
    return out


if __name__ == "__main__":
    a = sys.argv[1:]
    print(json.dumps(batch(a[0] if a else "room", float(a[1]) if len(a) > 1 else 150.0, *(int(x) for x in a[2:5]))))
