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
build of the library the plain rows (--info none) compare the two builds.  --loss KIND:A (geman_mcclure:1, cauchy:0.5, ...): the same
graph with every closure under that loss (msfl_graph_set_losses; rows without a long edge are left out), which runs the per-factor-loss
siblings of the factor kernels; the row says so in `loss`.  No acceptance threshold hangs on these numbers.

    python tools/graph_throughput.py --marginals [--sizes 1000 10000] [--long 0 10] [--nodes 1 16] [--repeats 5]

writes profiles/graph_marginals.json instead: the time of one msfl_graph_marginals call for the marginals of `nodes` nodes spread over the
chain, at the start poses, warm (median of `repeats`), and of the same nodes asked one call each.  Yardstick in the same process:
scipy's sparse LU of the same undamped H = J^T J, factorisation + solve with the same 6 x nodes unit right-hand sides, median of 3."""
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


def scipy_marginals_seconds(prob, nodes):
    import scipy.sparse.linalg as spl
    _, _, J = gn.evaluate_sparse(prob, prob["poses"], gn.Options)
    H = (J.T @ J).tocsc()
    E = np.zeros((H.shape[0], 6 * len(nodes)))
    for q, k in enumerate(nodes):
        E[6 * k + np.arange(6), 6 * q + np.arange(6)] = 1.0
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        spl.splu(H).solve(E)
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def marginals(args):
    rows = []
    for n in args.sizes:
        for k in args.long:
            prob = make(n, k)
            g = capi.PoseGraph(0, max_nodes=n, max_edges=n + k, max_fixes=n // 50 + 2)
            g.add_nodes(torch.from_numpy(np.ascontiguousarray(prob["poses"])).cuda())
            g.add_edges(g.edges(prob["ei"], prob["ej"], prob["ez"], prob["esr"], prob["est"]))
            g.add_fixes(g.fixes(prob["fi"], prob["fj"], prob["ft"], prob["fp"], prob["fst"]))
            for m in args.nodes:
                nodes = np.unique(np.round(np.linspace(0, n - 1, m)).astype(int))
                pairs = np.stack([nodes, nodes], -1)
                _, sm = g.marginals(pairs)
                one, each = [], []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    _, sm = g.marginals(pairs)
                    one.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    for p in pairs:
                        g.marginals(p[None])
                    each.append(time.perf_counter() - t0)
                row = dict(n=n, long_edges=k, nodes=len(nodes), build=args.label, columns=sm.n_columns, cg_iterations=sm.cg_iterations,
                           cg_unconverged=sm.cg_unconverged, singular=sm.singular, min_pivot_ratio=sm.min_pivot_ratio,
                           one_call_ms=1e3 * float(np.median(one)), one_call_ms_min=1e3 * min(one), one_call_ms_max=1e3 * max(one),
                           one_call_per_node_ms=1e3 * float(np.median(each)), one_call_per_node_ms_min=1e3 * min(each), one_call_per_node_ms_max=1e3 * max(each),
                           scipy_splu_ms=None if args.no_scipy else 1e3 * scipy_marginals_seconds(prob, nodes))
                print(json.dumps(row), flush=True)
                rows.append(row)
            g.close()
    out = dict(device=torch.cuda.get_device_name(0), host_threads_scipy=1, host_cpus=os.cpu_count(), repeats=args.repeats, rows=rows)
    path = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "graph_marginals.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


DEFAULT_OUT = os.path.join(ROOT, "profiles", "graph_throughput.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 10000, 100000])
    ap.add_argument("--long", type=int, nargs="+", default=[0, 10, 100])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--info", nargs="+", default=["none"], choices=["none", "closures", "all"])
    ap.add_argument("--loss", default=None, metavar="KIND:A", help="every closure under this loss, e.g. geman_mcclure:1")
    ap.add_argument("--label", default="this", help="names the build in every row (A/B runs with MSFL_LIB)")
    ap.add_argument("--no-scipy", action="store_true", help="skip the host yardstick")
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--marginals", action="store_true", help="time msfl_graph_marginals instead (profiles/graph_marginals.json)")
    ap.add_argument("--nodes", type=int, nargs="+", default=[1, 16], help="marginals: requested nodes per call")
    args = ap.parse_args()
    if args.marginals:
        if args.sizes == [1000, 10000, 100000]:
            args.sizes = [1000, 10000]
        if args.long == [0, 10, 100]:
            args.long = [0, 10]
        return marginals(args)
    rows = []
    loss = None
    if args.loss:
        kind, _, a = args.loss.partition(":")
        loss = (capi.GRAPH_LOSS_NAMES.index(kind), float(a or 0.0))
    for n in args.sizes:
        for k in args.long:
            prob = make(n, k)
            for mode in args.info:
                if (mode == "closures" or loss) and k == 0:
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
                if loss:                                         # the closures: the last k edges of their kind
                    if mode == "none":
                        g.set_losses(capi.GRAPH_FACTOR_EDGE, loss, first=n - 1, n=k)
                    else:
                        g.set_losses(capi.GRAPH_FACTOR_EDGE_INFO, loss, first=int(as_info.sum()) - k, n=k)
                s = g.optimize()
                ts = []
                for _ in range(args.repeats):
                    g.set_poses(start)
                    g.synchronize()
                    t0 = time.perf_counter()
                    s = g.optimize()
                    ts.append(time.perf_counter() - t0)
                wall = float(np.median(ts))
                row = dict(n=n, long_edges=k, build=args.label, information=mode, information_edges=int(as_info.sum()), loss=args.loss, n_long_counted=s.n_long_edges,
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
