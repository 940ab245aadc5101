"""Writes tests/golden/graph_info_model_v1.npz: the parity cases of tests/test_gpu_graph_info.py ((i), (ii), (iii), (v) and the three
corridor forms of (iv)), the model's result for each (tests/graph_info_numpy.py) and d_case, the largest pose difference between its
dense and its sparse step solver.

    python tests/golden/make_graph_info_golden.py

Per case: the problem arrays, `x_<case>` the expected poses, `tr_<case>` = [termination code, iterations, successful steps],
`acc_<case>` the accept list, `cost_<case>` = [initial, final], `d_<case>`; for the corridor also `truth_iv` and `ate_iv` = the ATE of
the odometry alone and of the three forms after the optimisation.  The script refuses to write a case on which the two solvers disagree
on the trace, or whose d_case exceeds 1e-6.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import graph_info_numpy as gi  # noqa: E402

TERMINATION = ("empty", "gradient", "max_iterations", "min_radius", "invalid_steps", "parameter", "function")


def main():
    out = {}
    ates = []
    for name in gi.CASES:
        prob = gi.make_case(name)
        xd, td = gi.solve_dense(prob)
        xs, ts = gi.solve_sparse(prob)
        d = gi.gn.pose_distance(xd, xs)
        print("%-12s %-14s it %2d ok %2d accepted %s cost %.6g -> %.6g  long %d  d_case %.3g" %
              (name, td.termination, td.iterations, td.successful_steps, td.accepted, td.initial_cost, td.final_cost, gi.n_long(prob), d))
        assert (td.termination, td.iterations, td.successful_steps, td.accepted) == (ts.termination, ts.iterations, ts.successful_steps, ts.accepted), \
            "case %s: the two solvers disagree on the trace; change its seed" % name
        assert d <= 1e-6, "case %s: d_case %.3g" % (name, d)
        for k in gi.KEYS:
            out["%s_%s" % (k, name)] = prob[k]
        out["x_" + name] = xd
        out["tr_" + name] = np.array([TERMINATION.index(td.termination), td.iterations, td.successful_steps], np.int32)
        out["acc_" + name] = np.array(td.accepted, np.int32)
        out["cost_" + name] = np.array([td.initial_cost, td.final_cost])
        out["d_" + name] = np.float64(d)
        if name.startswith("iv_"):
            ates.append(gi.ate(xd, gi.corridor(None)[1]))
    prob, truth = gi.corridor(None)
    out["truth_iv"] = truth
    out["ate_iv"] = np.array([gi.ate(prob["poses"], truth)] + ates)
    print("corridor ATE: odometry %.3f m, plain %.3f m, isotropic %.3f m, rank 5 %.3f m" % tuple(out["ate_iv"]))
    chi = gi.chi2(gi.make_case("v"), out["x_v"])[2]
    print("case v: chi-square of the four closures at the solved poses", chi[-4:])
    np.savez_compressed(os.path.join(HERE, "graph_info_model_v1.npz"), **out)


if __name__ == "__main__":
    main()
