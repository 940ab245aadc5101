"""Seeded pose-graph problems at the structural limits of the device solve (docs/kernels/graph.md), on top of tests/graph_numpy.py.

TEST INFRASTRUCTURE.  graph_numpy is imported, not edited; its CASES (a) .. (h) stay what they are.

Three families (CASES lists them in this order):

    ladder, direct solve  n<N>:   a chain of N nodes, no fixed node, one position fix per 50 poses, no long factor, at the sizes where
                                  the cyclic reduction changes shape: 1 .. 3 blocks, 255 / 256 / 257 (one partial sum per 256 free
                                  nodes), 1 023 / 1 024 / 1 025 (the one-workgroup form against one launched level), 2 047 / 2 048 /
                                  2 049 (one launched level against two) and 4 097 (three: 4 097 -> 2 049 -> 1 025 -> 513).
                                  n1 is NOT a one-node graph: a fix must join two different nodes (add_fixes refuses i == j, see
                                  tests/test_gpu_graph.py::test_refusals_leave_the_graph_unchanged), so it is two nodes, node 0 fixed,
                                  one edge and one fix: F = 1.  Its one free pose starts 0.37 m / 0.2 rad off, since an edge alone
                                  is met exactly by the start poses and the solve would end before its first step.
                                  n2 and n3 carry TWO fixes ((0, 1) twice; (0, 1) and (1, 2)).  With the one fix of the rule the
                                  optimum has no residual (12 or 18 unknowns against 9 or 15 rows): the final cost is 8e-18 and 4e-14,
                                  rounding noise on which the model's own two solvers differ by 6.5e-5 and 1.5e-7 relative (1e-2 on
                                  the last candidate cost), so no solver can meet the suite's 1e-9 relative cost bar there.  The
                                  second fix leaves a residual (final cost 1e-3 .. 1e-2) and changes nothing else: same F, same levels.
    ladder, CG path       cg<N>:  N nodes, node 0 fixed (F = N - 1 = 1 023, 1 024, 1 025, 2 048, 2 049), two closures from near the
                                  start of the drive to near its end: the right-hand-side half of the reduction with 0, 1 and 2
                                  launched levels under PCG.
    structure             span, ends, runs, reversed, signs (and signs_twin), all_but_one, hub_across_fixed (and
                                  hub_across_fixed_twin): about 40 nodes each, fixed nodes and factors placed where the free-node
                                  numbering differs from the node numbering.  Each carries position fixes, so that the solve moves
                                  the poses.

Every case meets three conditions, which tests/test_graph_structure_model.py asserts and tests/golden/make_graph_structure_golden.py
refuses to write without: the model's two step solvers agree on termination, iterations and accept list; the model accepts at least
two steps; its solution moves some free pose by at least 1 cm.  A case that misses one gets another seed, never a looser bound.
"""
import functools

import numpy as np

try:
    from tests import graph_numpy as gn
except ImportError:                        # run as a script from tests/golden
    import graph_numpy as gn

LADDER = (1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097)
CG_LADDER = (1024, 1025, 1026, 2049, 2050)
STRUCTURE = ("span", "ends", "runs", "reversed", "signs", "signs_twin", "all_but_one", "hub_across_fixed", "hub_across_fixed_twin")
CASES = tuple("n%d" % n for n in LADDER) + tuple("cg%d" % n for n in CG_LADDER) + STRUCTURE
DENSE_LIMIT = 300                          # nodes up to which the dense variant runs (above: the sparse solve under two orderings)
N_STRUCT = 40

SEEDS = dict(span=201, ends=202, runs=203, reversed=204, signs=205, signs_twin=205, all_but_one=206, hub_across_fixed=207,
             hub_across_fixed_twin=207)
SEEDS.update({"n%d" % n: 300 + k for k, n in enumerate(LADDER)})
SEEDS.update({"cg%d" % n: 400 + k for k, n in enumerate(CG_LADDER)})

# what the structure must come out as: free nodes and long factors per case (the ladders: F = N, or N - 1 on the CG path; 0 or 2)
EXPECT = dict(span=(37, 0), ends=(38, 1), runs=(35, 0), reversed=(40, 0), signs=(36, 2), signs_twin=(36, 2), all_but_one=(1, 0),
              hub_across_fixed=(40, 1), hub_across_fixed_twin=(39, 0))
EXPECT.update({"n%d" % n: (max(1, n), 0) for n in LADDER})
EXPECT.update({"cg%d" % n: (n - 1, 2) for n in CG_LADDER})


def _noise(rng, n=1):
    return np.concatenate([rng.normal(0, 0.01, (n, 3)), gn._small_rot(rng, n, 0.001)], -1)


def _measured(truth, rng, i, j):
    """T_i^-1 T_j of the truth with a closure's noise on it."""
    return gn.pose_mul(gn.relative_pose(truth[i], truth[j])[None], _noise(rng))[0]


def _fix_over(prob, truth, rng, i, j, t):
    """A position fix between any two nodes i, j (graph_numpy._gps only joins k and k + 1)."""
    p = (1.0 - t) * truth[i, :3] + t * truth[j, :3] + rng.normal(0, 0.01, 3)
    gn.add_fixes(prob, i, j, t, p)


def _ladder(n, seed):
    if n == 1:
        truth, odo, poses, rng = gn.drive(2, seed)
        prob = gn.problem(poses, [True, False])
        gn._chain(prob, odo)
        # the start pose of the one free node is off by more than the odometry's noise, so that the solve has a way to go
        prob["poses"][1] = gn.pose_mul(prob["poses"][1][None], np.array([[0.3, -0.2, 0.1, 0.0, 0.0, np.sin(0.1), np.cos(0.1)]]))[0]
        gn._gps(prob, truth, rng, [0])
        return prob
    truth, odo, poses, rng = gn.drive(n, seed)
    prob = gn.problem(poses)
    gn._chain(prob, odo)
    at = np.arange(0, n - 1, 50)
    if n <= 3:
        at = np.array([0, n - 2])          # n2, n3: a second fix, see the module docstring
    gn._gps(prob, truth, rng, at)
    return prob


def _cg(n, seed):
    truth, odo, poses, rng = gn.drive(n, seed)
    fixed = np.zeros(n, bool); fixed[0] = True
    prob = gn.problem(poses, fixed)
    gn._chain(prob, odo)
    gn._closures(prob, truth, rng, [(5, n - 20), (30, n - 3)])
    return prob


def _structure(name):
    n = N_STRUCT
    truth, odo, poses, rng = gn.drive(37 if name.startswith("signs") else n, SEEDS[name])
    n = len(poses)
    fixed = np.zeros(n, bool)
    if name == "span":
        # (9, 12) and (19, 21) join free neighbours: nodes 10, 11 and 20 between them are fixed.  Chain factors, all three.
        fixed[[10, 11, 20]] = True
        prob = gn.problem(poses, fixed)
        gn._chain(prob, odo)
        gn.add_edges(prob, 9, 12, _measured(truth, rng, 9, 12))
        gn.add_edges(prob, 19, 21, _measured(truth, rng, 19, 21))
        _fix_over(prob, truth, rng, 9, 12, 0.35)
        gn._gps(prob, truth, rng, [0, 15, 30, 38])
    elif name == "ends":
        fixed[[0, n - 1]] = True
        prob = gn.problem(poses, fixed)
        gn._chain(prob, odo)
        gn._closures(prob, truth, rng, [(5, 33)])
        gn._gps(prob, truth, rng, [8, 20, 30])
    elif name == "runs":
        # two runs of fixed nodes; the chain's edge (20, 21) and a fix over the same two nodes have both ends fixed
        fixed[[0, 1, 2, 20, 21]] = True
        prob = gn.problem(poses, fixed)
        gn._chain(prob, odo)
        gn.add_edges(prob, 21, 20, _measured(truth, rng, 21, 20))
        _fix_over(prob, truth, rng, 20, 21, 0.5)
        gn._gps(prob, truth, rng, [2, 5, 12, 19, 30, 37])
    elif name == "reversed":
        # every third step of the odometry as (k + 1, k) with the inverse measurement, and a reversed duplicate of the forward edge (7, 8)
        prob = gn.problem(poses, fixed)
        k = np.arange(n - 1)
        back = k % 3 == 0
        gn.add_edges(prob, np.where(back, k + 1, k), np.where(back, k, k + 1), np.where(back[:, None], gn.pose_inv(odo), odo))
        gn.add_edges(prob, 8, 7, _measured(truth, rng, 8, 7))
        gn._gps(prob, truth, rng, [0, 13, 26, 38])
    elif name.startswith("signs"):
        # graph_numpy's case (b) in shape; `signs` hands every second pose over as -q, the same rotation
        fixed[0] = True
        prob = gn.problem(poses, fixed)
        gn._chain(prob, odo)
        gn._closures(prob, truth, rng, [(2, 33), (10, 36)])
        gn._gps(prob, truth, rng, [6, 20, 30])
        if name == "signs":
            prob["poses"][1::2, 3:] *= -1
    elif name == "all_but_one":
        fixed[:] = True; fixed[17] = False
        prob = gn.problem(poses, fixed)
        gn._chain(prob, odo)
        prob["poses"][17] = gn.pose_mul(prob["poses"][17][None], np.array([[0.2, 0.1, -0.1, 0.0, 0.0, np.sin(0.08), np.cos(0.08)]]))[0]
        gn._gps(prob, truth, rng, [16, 17])
    else:
        # (14, 16): two apart in the free numbering while node 15 between them is free (long); one apart once it is fixed (chain)
        fixed[15] = name == "hub_across_fixed_twin"
        prob = gn.problem(poses, fixed)
        gn._chain(prob, odo)
        gn.add_edges(prob, 14, 16, _measured(truth, rng, 14, 16))
        gn._gps(prob, truth, rng, [3, 20, 33])
    return prob


@functools.lru_cache(maxsize=None)
def _make(name):
    if name in STRUCTURE:
        return _structure(name)
    if name.startswith("cg"):
        return _cg(int(name[2:]), SEEDS[name])
    return _ladder(int(name[1:]), SEEDS[name])


def make_case(name):
    """A fresh copy of the problem (the arrays are the caller's to change)."""
    return {k: np.array(v) for k, v in _make(name).items()}


def n_nodes(name):
    return len(_make(name)["poses"])


def global_levels(n_free):
    """Levels of the reduction that run as launches of their own: those above the first of at most 1 024 blocks."""
    k = 0
    while n_free > 1024:
        n_free = (n_free + 1) // 2
        k += 1
    return k


class OneStep(gn.Options):
    max_num_iterations = 1


def solve(name, opt=gn.Options):
    """(x, trace, same, d_case): the reference variant's result, whether the two variants agree on the trace, and their pose distance.
    Up to DENSE_LIMIT nodes the variants are dense (the reference) and sparse, above it the sparse solve under COLAMD (the reference)
    and in natural order."""
    prob = _make(name)
    if len(prob["poses"]) <= DENSE_LIMIT:
        xa, ta = gn.solve_dense(prob, opt)
        xb, tb = gn.solve_sparse(prob, opt)
    else:
        xa, ta = gn.solve_sparse(prob, opt)
        xb, tb = gn.solve_sparse(prob, opt, permc_spec="NATURAL")
    same = (ta.termination, ta.iterations, ta.successful_steps, ta.accepted) == (tb.termination, tb.iterations, tb.successful_steps, tb.accepted)
    return xa, ta, same, gn.pose_distance(xa, xb)


def moved(prob, x):
    """How far the solution took the free pose it moved most (metres or radians, graph_numpy.pose_distance)."""
    free = ~np.asarray(prob["fixed"], bool)
    return gn.pose_distance(prob["poses"][free], x[free])
