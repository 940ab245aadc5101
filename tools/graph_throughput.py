"""Throughput of the pose-graph solve (msfl_graph_optimize): writes profiles/graph_throughput.json.

    python tools/graph_throughput.py [--sizes 1000 10000 100000] [--long 0 10 100] [--repeats 5] [--info none closures all]

Per (N, long edges): a seeded circle-like drive (tests/graph_numpy.drive) with N - 1 odometry edges, a position fix every 50
poses and the given number of long edges between random distant pairs; poses handed over from device memory.  One warm-up
optimize, then `repeats` timed ones from the same start (set_poses from a device tensor); wall time is the median.  Time per LM
iteration = wall / iterations; per CG iteration = wall / cg_iterations (an upper bound: it carries the linearisation too).  The
block-tridiagonal solve alone is the N-with-0-long-edges row: there every LM iteration holds exactly one factorisation and two
right-hand-side passes.  Yardstick in the same process: scipy's sparse LU (SuperLU, one thread) of the same damped normal equations at
the start poses, factorisation + solve, median of 3.  --info: the same graph with its long edges (closures), or all its edges (all), handed
over as information edges with the isotropic L of the same cost (tests/graph_info_numpy.isotropic_L); with MSFL_LIB set to another
build of the library the plain rows (--info none) compare the two builds.  No acceptance threshold hangs on these numbers."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from msf_loam_amd import capi
from tests import graph_info_numpy as gi
from tests import graph_numpy as gn


def make(n, n_long, seed=5):
    truth, odo, poses, rng = gn.drive(n, seed, radius=max(20.0, n / 60.0), turns=1.15)
    prob = gn.problem(poses)
    gn._chain(prob, odo)
    if n_long:
        i = rng.integers(0, n // 3, n_long)
        j = rng.integers(2 * n // 3, n, n_long)
        gn._closures(prob, truth, rng, list(zip(i.tolist(), j.tolist())))
    gn._gps(prob, truth, rng, np.arange(0, n - 1, 50))
    return prob


def scipy_step_seconds(prob):
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    _, r, J = gn.evaluate_sparse(prob, prob["poses"], gn.Options)
    scale = 1.0 / (1.0 + np.sqrt(np.asarray(J.multiply(J).sum(0)).ravel()))
    Js = J @ sp.diags(scale)
    d = np.clip(np.asarray(Js.multiply(Js).sum(0)).ravel(), 1e-6, 1e32) / 1e4
    H = (Js.T @ Js + sp.diags(d)).tocsc()
    b = -(Js.T @ r)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        spl.splu(H).solve(b)
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 10000, 100000])
    ap.add_argument("--long", type=int, nargs="+", default=[0, 10, 100])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--info", nargs="+", default=["none"], choices=["none", "closures", "all"])
    ap.add_argument("--label", default="this", help="names the build in every row (A/B runs with MSFL_LIB)")
    ap.add_argument("--no-scipy", action="store_true", help="skip the host yardstick")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_throughput.json"))
    args = ap.parse_args()
    rows = []
    for n in args.sizes:
        for k in args.long:
            prob = make(n, k)
            for mode in args.info:
                if mode == "closures" and k == 0:
                    continue
                start = torch.from_numpy(np.ascontiguousarray(prob["poses"])).cuda()
                g = capi.PoseGraph(0, max_nodes=n, max_edges=n + k, max_fixes=n // 50 + 2)
                g.add_nodes(start)
                e = g.edges(prob["ei"], prob["ej"], prob["ez"], prob["esr"], prob["est"])
                as_info = np.zeros(len(e), bool)
                if mode == "closures":
                    as_info[n - 1:] = True                   # the chain's N - 1 edges come first
                elif mode == "all":
                    as_info[:] = True
                g.add_edges(e[~as_info])
                if as_info.any():
                    g.add_edges_info(g.edges_info(e["i"][as_info], e["j"][as_info], e["z"][as_info], gi.isotropic_L(e["sr"][as_info], e["st"][as_info], int(as_info.sum()))))
                g.add_fixes(g.fixes(prob["fi"], prob["fj"], prob["ft"], prob["fp"], prob["fst"]))
                s = g.optimize()
                ts = []
                for _ in range(args.repeats):
                    g.set_poses(start)
                    g.synchronize()
                    t0 = time.perf_counter()
                    s = g.optimize()
                    ts.append(time.perf_counter() - t0)
                wall = float(np.median(ts))
                row = dict(n=n, long_edges=k, build=args.label, information=mode, information_edges=int(as_info.sum()), n_long_counted=s.n_long_edges,
                           termination=capi.GRAPH_TERMINATION[s.termination], iterations=s.iterations,
                           cg_iterations=s.cg_iterations, cg_unconverged=s.cg_unconverged, initial_cost=s.initial_cost, final_cost=s.final_cost,
                           wall_ms=1e3 * wall, wall_ms_min=1e3 * min(ts), wall_ms_max=1e3 * max(ts),
                           ms_per_lm_iteration=1e3 * wall / max(1, s.iterations), ms_per_cg_iteration=1e3 * wall / max(1, s.cg_iterations),
                           scipy_splu_one_step_ms=None if args.no_scipy else 1e3 * scipy_step_seconds(prob))
                print(json.dumps(row), flush=True)
                rows.append(row)
                g.close()
    out = dict(device=torch.cuda.get_device_name(0), host_threads_scipy=1, host_cpus=os.cpu_count(), repeats=args.repeats, rows=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
