"""Writes tests/golden/graph_model_v1.npz: the parity cases (a) .. (h) of tests/test_gpu_graph.py, the model's result for each and
d_case, the largest pose difference between two exact step solvers of the model (tests/graph_numpy.py).

    python tests/golden/make_graph_golden.py

Per case: the problem arrays, `x_<case>` the expected poses, `tr_<case>` = [termination code, iterations, successful steps],
`acc_<case>` the accept list, `cost_<case>` = [initial, final], `d_<case>`.  The two variants are `dense` and `sparse`; for (g),
too large for the dense one, they are the sparse solve under two column orderings (COLAMD and NATURAL).  The script refuses to
write a case on which the two variants disagree on the trace, or whose d_case exceeds 1e-6 (the outlier case (f) excepted).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import graph_numpy as gn  # noqa: E402

TERMINATION = ("empty", "gradient", "max_iterations", "min_radius", "invalid_steps", "parameter", "function")
KEYS = ("poses", "fixed", "ei", "ej", "ez", "esr", "est", "fi", "fj", "ft", "fp", "fst")


def run_case(name):
    prob = gn.make_case(name)
    if name == "g":
        xa, ta = gn.solve_sparse(prob)
        xb, tb = gn.solve_sparse(prob, permc_spec="NATURAL")
    else:
        xb, tb = gn.solve_dense(prob)
        xa, ta = gn.solve_sparse(prob)
    same = (ta.termination, ta.iterations, ta.successful_steps, ta.accepted) == (tb.termination, tb.iterations, tb.successful_steps, tb.accepted)
    ref_x, ref_t = (xa, ta) if name == "g" else (xb, tb)
    return prob, ref_x, ref_t, same, gn.pose_distance(xa, xb)


def main():
    out = {}
    for name in gn.CASES:
        prob, x, tr, same, d = run_case(name)
        print("%s: %-14s it %2d ok %2d accepted %s cost %.6g -> %.6g  long %d  d_case %.3g" %
              (name, tr.termination, tr.iterations, tr.successful_steps, tr.accepted, tr.initial_cost, tr.final_cost, gn.n_long(prob), d))
        assert same, "case %s: the two variants disagree on the trace; change its seed" % name
        assert name == "f" or d <= 1e-6, "case %s: d_case %.3g" % (name, d)
        for k in KEYS:
            out["%s_%s" % (k, name)] = prob[k]
        out["x_" + name] = x
        out["tr_" + name] = np.array([TERMINATION.index(tr.termination), tr.iterations, tr.successful_steps], np.int32)
        out["acc_" + name] = np.array(tr.accepted, np.int32)
        out["cost_" + name] = np.array([tr.initial_cost, tr.final_cost])
        out["d_" + name] = np.float64(d)
    np.savez_compressed(os.path.join(HERE, "graph_model_v1.npz"), **out)


if __name__ == "__main__":
    main()
