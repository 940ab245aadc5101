"""Writes tests/golden/graph_structure_model_v1.npz: what the model (tests/graph_numpy.py) gives for the cases of
tests/graph_structure_cases.py, the pose graph at its structural limits.

    python tests/golden/make_graph_structure_golden.py

The problems themselves are not stored (graph_structure_cases.make_case builds them from their seeds).  Per case: `x_<case>` the expected
poses, `tr_<case>` = [termination code, iterations, successful steps], `acc_<case>` the accept list, `cand_<case>` the candidate cost of
every iteration, `cost_<case>` = [initial, final], `d_<case>` the largest pose difference between the model's two exact step solvers
(dense and sparse up to 300 nodes; the sparse solve under COLAMD and in natural order above), `moved_<case>` how far the solution took
the free pose it moved most, and `shape_<case>` = [nodes, free nodes, long factors].

The poses of all cases are 1.2 MB of float64, which do not compress, and no committed file may pass 1 MiB: `x_<case>` is left out for the
cases in LIVE_X, whose solution the tests get from the model as they run (1 s each) and whose trace they still hold against the
stored one.  The script refuses a case that misses one of the three conditions of graph_structure_cases, or whose d_case exceeds 1e-6.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import graph_numpy as gn  # noqa: E402
import graph_structure_cases as sc  # noqa: E402

TERMINATION = ("empty", "gradient", "max_iterations", "min_radius", "invalid_steps", "parameter", "function")
LIVE_X = ("n4097", "cg2050")


def main():
    out = {}
    for name in sc.CASES:
        prob = sc.make_case(name)
        x, tr, same, d = sc.solve(name)
        shape = [len(prob["poses"]), int((~prob["fixed"]).sum()), gn.n_long(prob)]
        far = sc.moved(prob, x)
        print("%-22s nodes %4d free %4d long %d  %-14s it %2d ok %2d cost %.6g -> %.6g  moved %.3g  d_case %.3g" %
              (name, shape[0], shape[1], shape[2], tr.termination, tr.iterations, tr.successful_steps, tr.initial_cost, tr.final_cost, far, d))
        assert same, "case %s: the two variants disagree on the trace; change its seed" % name
        assert tr.successful_steps >= 2, "case %s: fewer than two accepted steps; change its seed" % name
        assert far >= 0.01, "case %s: no free pose moves by 1 cm; change its seed" % name
        assert d <= 1e-6, "case %s: d_case %.3g" % (name, d)
        assert tuple(shape[1:]) == sc.EXPECT[name], "case %s: %s free nodes / long factors" % (name, shape[1:])
        if name not in LIVE_X:
            out["x_" + name] = x
        out["tr_" + name] = np.array([TERMINATION.index(tr.termination), tr.iterations, tr.successful_steps], np.int32)
        out["acc_" + name] = np.array(tr.accepted, np.int32)
        out["cand_" + name] = np.array(tr.cost)
        out["cost_" + name] = np.array([tr.initial_cost, tr.final_cost])
        out["d_" + name] = np.float64(d)
        out["moved_" + name] = np.float64(far)
        out["shape_" + name] = np.array(shape, np.int32)
    path = os.path.join(HERE, "graph_structure_model_v1.npz")
    np.savez_compressed(path, **out)
    print("%d bytes" % os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
