"""Timed legs of the uncertainty output (docs/kernels/uncertainty.md), feature on against off:

  batch   the registration step of bench.py (map index + B scans registered, device resident) in one world, the records going to a
          device sink (msfl_set_uncertainty with MSFL_MEM_DEVICE: asynchronous, nothing synchronised)
  slam    the per-scan SLAM step (examples/replay_synthetic.py), synchronous and pipelined

  python tools/uncertainty_timing.py batch [room|outdoor|corridor] [scans] [copies] [reps]
  python tools/uncertainty_timing.py slam [room|outdoor|corridor] [scans]

Prints one JSON line.  Run the batch leg under `rocprofv3 --kernel-trace --stats` (tools/prof_cmd.sh) for the new kernel's own
time next to lm_solve_kernel's in the same run.  Timings only: nothing here checks a result (tests/test_gpu_uncertainty.py does).
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))


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
    d_unc = torch.zeros(B * capi.UNCERTAINTY_DTYPE.itemsize, dtype=torch.uint8, device=dev)

    def timed(k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            pipe.register(d_guess)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / k

    out = {"leg": "batch", "world": kind, "registrations": B, "reps": reps}
    legs = {"off": [], "on": []}
    for rnd in range(3):                                   # alternated: drift of the box shows up as spread, not as a difference
        for name in ("off", "on"):
            h.set_uncertainty_device(d_unc if name == "on" else None, B, 150.0)
            timed(2)
            legs[name].append(timed(reps))
    h.set_uncertainty_device(d_unc, B, 150.0)
    pipe.register(d_guess); torch.cuda.synchronize()
    u = np.frombuffer(d_unc.cpu().numpy().tobytes(), capi.UNCERTAINTY_DTYPE)
    poses_on = pipe.d_poses.cpu().numpy().copy()
    h.set_uncertainty_device(None, 0)
    pipe.register(d_guess); torch.cuda.synchronize()
    out["ms_per_step_off"], out["ms_per_step_on"] = legs["off"], legs["on"]
    out["poses_bit_identical"] = bool(np.array_equal(poses_on, pipe.d_poses.cpu().numpy()))
    out["valid"] = int(u["valid"].sum())
    out["n_degenerate_histogram"] = np.bincount(u["n_degenerate"][u["valid"] == 1], minlength=7).tolist()
    out["lambda_min_median"] = float(np.median(u["eigenvalues"][u["valid"] == 1, 0]))
    h.close()
    return out


def slam(kind="room", scans=120):
    import replay_synthetic as rp
    from msf_loam_amd import synth
    if kind == "room":
        world = synth.World(ground_half=45.0)
        truth = rp.trajectory(max(scans, 300))[:scans]
    else:
        world = synth.World(kind=kind)
        truth = rp.world_drive(world, kind, scans)
    sweeps = [synth.make_scan(world, truth[k], synth.SEED + 5000 + k) for k in range(scans)]
    out = {"leg": "slam", "world": kind, "scans": scans}
    for pipelined in (False, True):
        key = "pipelined" if pipelined else "synchronous"
        off, on = [], []
        for rnd in range(3):
            off.append(rp.run_slam(world, truth, pipelined=pipelined, scans=sweeps)[2])
            unc = []
            on.append(rp.run_slam(world, truth, pipelined=pipelined, scans=sweeps, uncertainty=150.0, unc_out=unc)[2])
        out["ms_per_scan_" + key + "_off"], out["ms_per_scan_" + key + "_on"] = off, on
    out["mapping_records_valid"] = int(sum(int(u[1]["valid"]) for u in unc))
    out["mapping_n_degenerate_histogram"] = np.bincount([int(u[1]["n_degenerate"]) for u in unc if u[1]["valid"]], minlength=7).tolist()
    return out


if __name__ == "__main__":
    a = sys.argv[1:]
    leg = a[0] if a else "batch"
    kind = a[1] if len(a) > 1 else "room"
    if leg == "batch":
        res = batch(kind, *(int(x) for x in a[2:5]))
    else:
        res = slam(kind, *(int(x) for x in a[2:3]))
    print(json.dumps(res))
